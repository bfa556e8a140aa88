"""Row softmax on a BSR pattern (mispmm_softmax_bsr_f32 and its backward) and the autograd functions built on it (block_softmax,
block_sparse_attention), on the GPU, against the numpy restatements and the bounds of tests/_softmax_bsr_ref.py.

Worst |err| / bound printed on an MI355X (`-s` prints every one): forward fp32 out 0.186, bf16 out
0.993 (the 2^-8 term is twice the rounding to bf16 itself); backward 0.117 and 0.993; worst |row sum - 1| / (L u) 0.168;
block_sparse_attention against the composed tolerance: out 0.709, dq 0.111, dk 0.185, dv 0.457.
tests/test_gpu_softmax_tight.py holds the same kernels to a derived tolerance without this slack, to exact tie rows and to offset rows."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, formats, ops  # noqa: E402

from _sddmm_bsr_ref import bound as sddmm_bsr_bound, from_bits, to_bits  # noqa: E402
from _sddmm_bsr_ref import full_mantissa as bf16_full_mantissa  # noqa: E402
from _softmax_bsr_ref import (HELD, assert_inside, backward, bf16_round, bwd_bound, causal_mask, forward, full_mantissa,  # noqa: E402
                              fwd_bound, layout, lengths, pattern, random_mask, row_sums, scores, to_rows, z_values)

pytestmark = pytest.mark.gpu

PATTERNS = ["edges16", "edges32", "ragged16", "ragged32"]
SCALES = (1.0, 0.125, 0.3)
SENTINELS = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def device_bsr(name):
    p = pattern(name)
    u32 = lambda a: dev(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))   # noqa: E731
    return ops.DeviceBSR(p.num_rows, p.num_cols, p.block_row_size, p.block_col_size, p.num_blocks, u32(p.block_row_ptrs),
                         u32(p.block_col_idxs), torch.empty(0, device="cuda"))      # the values are never read


@functools.lru_cache(maxsize=None)
def case(name, kind, scale, with_mask):
    """(scores, mask, exact softmax, T) on the host, shared by the tests; read-only."""
    s = scores(kind, name)
    mask = random_mask(name) if with_mask else None
    exact, t = forward(name, z_values(s, mask, scale))
    return s, mask, exact, t


def host(out):
    """A result as float32 on the host, whichever out type."""
    a = out.cpu().numpy()
    return from_bits(a) if a.dtype == np.int16 else a


def same_bits(got, want, what):
    got, want = got.cpu().numpy(), (want.cpu().numpy() if isinstance(want, torch.Tensor) else want)
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    differ = got.view(bits) != want.view(bits)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} elements differ, first at {np.argwhere(differ)[:3].tolist()}"


def expect_tag(name, prefix, out_bf16, last):
    p = pattern(name)
    bs = p.block_row_size
    path = "held" if p.num_blocks <= HELD[bs] else "walk"
    tag = capi.last_kernel()
    assert tag == f"{prefix}<b{bs},{'bf16' if out_bf16 else 'f32'},{path},C{HELD[bs]},{last}>", tag


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("name", PATTERNS)
def test_forward_within_the_stated_bounds_and_rows_sum_to_one(name, kind, with_mask):
    a, length = device_bsr(name), lengths(name)
    for scale in SCALES:
        s, mask, exact, t = case(name, kind, scale, with_mask)
        sd, md = dev(s), (dev(mask) if with_mask else None)
        for out_bf16 in (False, True):
            out = ops.softmax_bsr(a, sd, scale=scale, mask=md, out_bf16=out_bf16)
            expect_tag(name, "softmax_bsr", out_bf16, "mask" if with_mask else "nomask")
            assert out.shape == s.shape and out.dtype == (torch.int16 if out_bf16 else torch.float32)
            got = host(out)
            what = f"forward {name} {kind} scale={scale} {capi.last_kernel()}"
            assert_inside(got, exact, fwd_bound(out_bf16, length, t, exact), what)
            if not out_bf16:
                sums, lens = row_sums(name, got)
                off = np.abs(sums - 1).astype(np.float64)
                print(f"{what}: max |row sum - 1| / (L u) = {float(np.max(off / (lens * 2.0 ** -24))):.3g}")
                assert np.all(off <= lens * 2.0 ** -24), f"{what}: rows {np.argwhere(off > lens * 2.0 ** -24)[:4].ravel().tolist()} do not sum to 1 within L u"


@pytest.mark.parametrize("bs", [16, 32])
def test_the_tag_shows_held_up_to_c_blocks_and_walk_beyond(bs):
    """A launch whose pattern has no more than C blocks cannot hold a longer block row: `held`; any other says `walk`.  A block
    row alone gives the bits it gives among the others of edges16 / edges32: nothing but its own length decides its sums."""
    name = f"edges{bs}"
    p, c = pattern(name), HELD[bs]
    ptrs = p.block_row_ptrs.astype(np.int64)
    s = scores("narrow", name)
    whole = ops.softmax_bsr(device_bsr(name), dev(s), scale=0.3).cpu().numpy()
    assert ",walk," in capi.last_kernel()
    for n in (1, c - 1, c, c + 1, 2 * c + 1):
        r = int(np.argwhere(np.diff(ptrs) == n)[0, 0])
        alone = ops.DeviceBSR(bs, n * bs, bs, bs, n, dev(np.array([0, n], np.int32)), dev(np.arange(n, dtype=np.int32)), torch.empty(0, device="cuda"))
        part = dev(s[ptrs[r]:ptrs[r + 1]])
        got = ops.softmax_bsr(alone, part, scale=0.3)
        assert f",{'held' if n <= c else 'walk'},C{c}," in capi.last_kernel(), capi.last_kernel()
        same_bits(got, whole[ptrs[r]:ptrs[r + 1]], f"a block row of {n} blocks alone")
        ds = ops.softmax_bsr_bwd(alone, got, part, scale=0.3)
        assert capi.last_kernel().startswith(f"softmax_bsr_bwd<b{bs},f32,{'held' if n <= c else 'walk'},C{c},"), capi.last_kernel()
        assert ds.shape == part.shape


@pytest.mark.parametrize("name", PATTERNS)
def test_exactness_anchors(name):
    a, length = device_bsr(name), lengths(name)
    row_ptrs, idx = layout(name)
    # equal scores: exp2(0) = 1 per term, the sum L is exact, the quotient is the correctly rounded fl32(1 / L)
    eq = dev(scores("equal", name))
    want = (np.float32(1.0) / length.astype(np.float32)).astype(np.float32)
    same_bits(ops.softmax_bsr(a, eq, scale=0.3), want, "equal scores, fp32")
    same_bits(ops.softmax_bsr(a, eq, scale=0.3, out_bf16=True), to_bits(bf16_round(want)), "equal scores, bf16")
    # every matrix row with all but one element masked: that element is exactly 1, the others exactly +0
    rng = np.random.default_rng(12)
    starts, lens = row_ptrs[:-1][np.diff(row_ptrs) > 0], np.diff(row_ptrs)[np.diff(row_ptrs) > 0]
    keep = idx[starts + rng.integers(0, lens)]
    mask = np.full(length.shape, -np.inf, np.float32)
    mask.reshape(-1)[keep] = rng.uniform(-2, 2, keep.shape[0]).astype(np.float32)
    want = np.zeros(length.shape, np.float32)
    want.reshape(-1)[keep] = 1.0
    s = dev(scores("wide", name))
    same_bits(ops.softmax_bsr(a, s, scale=0.3, mask=dev(mask)), want, "one unmasked element per row, fp32")
    same_bits(ops.softmax_bsr(a, s, scale=0.3, mask=dev(mask), out_bf16=True), to_bits(want), "one unmasked element per row, bf16")
    # a masked element beside finite ones is exactly +0
    mask = random_mask(name)
    for out_bf16 in (False, True):
        got = ops.softmax_bsr(a, s, scale=0.125, mask=dev(mask), out_bf16=out_bf16).cpu().numpy()
        hidden = np.isneginf(mask)
        assert hidden.sum() > mask.size // 8 and not got.view(np.uint16 if out_bf16 else np.uint32)[hidden].any(), "a masked element is not +0"


@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("name", PATTERNS)
def test_special_values_stay_in_their_matrix_row(name, out_bf16):
    """A NaN, a +Inf and an all -Inf row, each written into ONE matrix row of the first block row, of a block row of C + 1
    blocks (where the pattern has one) and of the last non-empty one: exactly that matrix row is NaN, every other element --
    the other rows of the same blocks included -- keeps the bits of the clean run."""
    p, a = pattern(name), device_bsr(name)
    bs = p.block_row_size
    ptrs = p.block_row_ptrs.astype(np.int64)
    counts = np.diff(ptrs)
    filled = np.argwhere(counts > 0).ravel()
    targets = [int(filled[0]), int(filled[-1])] + [int(r) for r in np.argwhere(counts == HELD[bs] + 1).ravel()[:1]]
    assert name.startswith("ragged") or len(targets) == 3
    s = scores("narrow", name)
    mask = dev(random_mask(name))
    clean = ops.softmax_bsr(a, dev(s), scale=0.3, mask=mask, out_bf16=out_bf16).cpu().numpy()
    nan_of = lambda x: np.isnan(from_bits(x) if out_bf16 else x)   # noqa: E731
    assert not nan_of(clean).any()
    for t, r in enumerate(targets):
        i = (5 * t + 3) % bs
        for what in ("nan", "+inf", "all -inf"):
            sp = s.copy()
            if what == "nan":
                sp[ptrs[r] + counts[r] // 2, i, bs - 1] = np.nan
            elif what == "+inf":
                sp[ptrs[r + 1] - 1, i, 0] = np.inf
            else:
                sp[ptrs[r]:ptrs[r + 1], i, :] = -np.inf
            got = ops.softmax_bsr(a, dev(sp), scale=0.3, mask=mask, out_bf16=out_bf16).cpu().numpy()
            hit = np.zeros(s.shape, bool)
            hit[ptrs[r]:ptrs[r + 1], i, :] = True
            assert np.array_equal(nan_of(got), hit), f"{what} in row {i} of block row {r}: NaN positions differ"
            assert np.array_equal(got[~hit], clean[~hit]), f"{what} in row {i} of block row {r}: another row changed"


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("name", PATTERNS)
def test_backward_within_the_stated_bounds(name, kind):
    a, length = device_bsr(name), lengths(name)
    dp = full_mantissa(np.random.default_rng(10), length.shape)
    dpd = dev(dp)
    for scale in (1.0, 0.3):
        for p_bf16 in (False, True):
            p = ops.softmax_bsr(a, dev(scores(kind, name)), scale=scale, out_bf16=p_bf16)       # p from the library's forward
            ph = host(p)
            exact, cap = backward(name, ph, dp, scale)
            for ds_bf16 in (False, True):
                ds = ops.softmax_bsr_bwd(a, p, dpd, scale=scale, out_bf16=ds_bf16)
                expect_tag(name, "softmax_bsr_bwd", ds_bf16, "p_bf16" if p_bf16 else "p_f32")
                assert ds.shape == dp.shape and ds.dtype == (torch.int16 if ds_bf16 else torch.float32)
                assert_inside(host(ds), exact, bwd_bound(ds_bf16, length, ph, dp, cap, scale, exact),
                              f"backward {name} {kind} scale={scale} {capi.last_kernel()}")
            zero = torch.zeros_like(dpd)
            for ds_bf16 in (False, True):
                ds = ops.softmax_bsr_bwd(a, p, zero, scale=scale, out_bf16=ds_bf16).cpu().numpy()
                assert not ds.view(np.uint16 if ds_bf16 else np.uint32).any(), "the backward of an all-zero dp is not all +0"


def test_forward_and_backward_on_activsg10k():
    """16 x 16, 33100 blocks, block rows of up to 54: most are held, some walk.  bf16 out, against the float64 restatement."""
    name = "ACTIVSg10K"
    a, length = device_bsr(name), lengths(name)
    s, scale = scores("narrow", name), 0.125
    exact, t = forward(name, z_values(s, None, scale), np.float64)
    p = ops.softmax_bsr(a, dev(s), scale=scale, out_bf16=True)
    assert capi.last_kernel() == "softmax_bsr<b16,bf16,walk,C32,nomask>", capi.last_kernel()
    assert_inside(host(p), exact, fwd_bound(True, length, t, exact), f"forward {name}")
    dp = full_mantissa(np.random.default_rng(13), s.shape)
    ds = ops.softmax_bsr_bwd(a, p, dev(dp), scale=scale, out_bf16=True)
    assert capi.last_kernel() == "softmax_bsr_bwd<b16,bf16,walk,C32,p_bf16>", capi.last_kernel()
    ph = host(p)
    ds_exact, cap = backward(name, ph, dp, scale, np.float64)
    assert_inside(host(ds), ds_exact, bwd_bound(True, length, ph, dp, cap, scale, ds_exact), f"backward {name}")


@pytest.mark.parametrize("name", PATTERNS)
def test_sentinels_either_side_of_out_and_ds_stay(name):
    """out and ds as the middle of a longer buffer: the 64 elements before and behind stay, and every element between is
    written (the blocks either side of an empty block row included) with the bits of a run into a buffer of its own."""
    a = device_bsr(name)
    s, dp = dev(scores("narrow", name)), dev(full_mantissa(np.random.default_rng(14), lengths(name).shape))
    count = s.numel()
    for bf16 in (False, True):
        def buffer():
            if bf16:
                return torch.full((count + 2 * SENTINELS,), 0x1234, dtype=torch.int16, device="cuda"), 0x1234
            return torch.full((count + 2 * SENTINELS,), -7.0, device="cuda"), -7.0
        want = ops.softmax_bsr(a, s, scale=0.3, out_bf16=bf16)
        buf, mark = buffer()
        inner = buf[SENTINELS:SENTINELS + count].view(s.shape)
        got = ops.softmax_bsr(a, s, scale=0.3, out_bf16=bf16, out=inner)
        assert got.data_ptr() == inner.data_ptr()
        assert bool((buf[:SENTINELS] == mark).all()) and bool((buf[SENTINELS + count:] == mark).all()), "a sentinel of out was written"
        same_bits(got, want, "out inside a buffer")
        want_ds = ops.softmax_bsr_bwd(a, want, dp, scale=0.3, out_bf16=bf16)
        buf, mark = buffer()
        inner = buf[SENTINELS:SENTINELS + count].view(s.shape)
        got = ops.softmax_bsr_bwd(a, want, dp, scale=0.3, out_bf16=bf16, out=inner)
        assert bool((buf[:SENTINELS] == mark).all()) and bool((buf[SENTINELS + count:] == mark).all()), "a sentinel of ds was written"
        same_bits(got, want_ds, "ds inside a buffer")


@pytest.mark.parametrize("name", ["edges16", "edges32"])
def test_deterministic_and_replays_from_a_graph(name):
    a = device_bsr(name)
    s, mask = dev(scores("narrow", name)), dev(random_mask(name))
    dp = dev(full_mantissa(np.random.default_rng(11), lengths(name).shape))
    p = ops.softmax_bsr(a, s, scale=0.3, mask=mask, out_bf16=True).clone()
    ds = ops.softmax_bsr_bwd(a, p, dp, scale=0.3, out_bf16=True).clone()
    same_bits(ops.softmax_bsr(a, s, scale=0.3, mask=mask, out_bf16=True), p, "second run")
    same_bits(ops.softmax_bsr_bwd(a, p, dp, scale=0.3, out_bf16=True), ds, "second backward run")
    p2, ds2 = torch.empty_like(p), torch.empty_like(ds)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture
        ops.softmax_bsr(a, s, scale=0.3, mask=mask, out_bf16=True, out=p2)
        ops.softmax_bsr_bwd(a, p2, dp, scale=0.3, out_bf16=True, out=ds2)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                   # one stream, one launch after the other: no parallel branches
        ops.softmax_bsr(a, s, scale=0.3, mask=mask, out_bf16=True, out=p2)
        ops.softmax_bsr_bwd(a, p2, dp, scale=0.3, out_bf16=True, out=ds2)
    p2.zero_()
    ds2.zero_()
    g.replay()
    torch.cuda.synchronize()
    same_bits(p2, p, "graph replay")
    same_bits(ds2, ds, "graph replay backward")


def test_empty_patterns_are_no_ops_and_bad_arguments_raise():
    empty = ops.DeviceBSR.from_host(formats.BSR(32, 48, 0, 16, 16, np.zeros(3, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 16, 16), np.float32)))
    none = ops.DeviceBSR.from_host(formats.BSR(0, 48, 0, 16, 16, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 16, 16), np.float32)))
    z = torch.zeros((0, 16, 16), device="cuda")
    for a in (empty, none):
        assert ops.softmax_bsr(a, z).shape == (0, 16, 16) and ops.softmax_bsr(a, z, mask=z, out_bf16=True).dtype == torch.int16
        assert ops.softmax_bsr_bwd(a, z, z).shape == (0, 16, 16) and ops.softmax_bsr_bwd(a, z.to(torch.int16), z, out_bf16=True).dtype == torch.int16
    a = device_bsr("ragged16")
    s = torch.zeros((a.num_blocks, 16, 16), device="cuda")
    for bad in (s.cpu(), s.double(), s[1:], s.reshape(a.num_blocks, 256), s.transpose(1, 2)):
        with pytest.raises(ValueError):
            ops.softmax_bsr(a, bad)
        with pytest.raises(ValueError):
            ops.softmax_bsr(a, s, mask=bad)
        with pytest.raises(ValueError):
            ops.softmax_bsr_bwd(a, s, bad)
    with pytest.raises(ValueError):
        ops.softmax_bsr(a, s, out=torch.empty_like(s, dtype=torch.int16))
    for scale in (0.0, -1.0, float("inf"), float("nan")):          # the library's own refusal, before any launch
        with pytest.raises(capi.MispmmError, match="scale"):
            ops.softmax_bsr(a, s, scale=scale)
        with pytest.raises(capi.MispmmError, match="scale"):
            ops.softmax_bsr_bwd(a, s, s, scale=scale)


# ---- autograd
def bf(v):
    """float32 host array of bf16 numbers -> bfloat16 device tensor (the conversion is exact)."""
    return dev(v).to(torch.bfloat16)


def bits(t):
    return t.view(torch.int16)


@functools.lru_cache(maxsize=None)
def trainable(name):
    return autograd.TrainableBSR.from_host(pattern(name))


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", PATTERNS)
def test_block_softmax_is_the_library_kernel_both_ways(name, out_dtype):
    a = trainable(name)
    out_bf16 = out_dtype == torch.bfloat16
    s = dev(scores("narrow", name)).requires_grad_(True)
    mask = dev(random_mask(name))
    p = autograd.block_softmax(a, s, scale=0.3, mask=mask, out_dtype=out_dtype)
    assert p.dtype == out_dtype and p.grad_fn is not None
    want = ops.softmax_bsr(a.fwd, s.detach(), scale=0.3, mask=mask, out_bf16=out_bf16)
    same_bits(bits(p.detach()) if out_bf16 else p.detach(), want, "block_softmax forward")
    g = dev(bf16_full_mantissa(np.random.default_rng(15), tuple(s.shape)))          # bf16 numbers: exact in either out type
    p.backward(g.to(out_dtype))
    same_bits(s.grad, ops.softmax_bsr_bwd(a.fwd, want, g, scale=0.3), "block_softmax backward")


def hand_chain(a, q, k, v, g, scale, mask, out_bf16):
    """The chain of ops calls block_sparse_attention is documented to make, by hand: (out, dq, dk, dv) as int16 / float32."""
    s = ops.sddmm_bsr_bf16(a.fwd, bits(q), bits(k))
    p = ops.softmax_bsr(a.fwd, s, scale=scale, mask=mask, out_bf16=True)
    out = ops.spmm_bsr_bf16(a.fwd, p, bits(v), out_bf16=out_bf16)
    gb = bits(g.contiguous()) if g.dtype == torch.bfloat16 else ops.f32_to_bf16(g.contiguous())
    dv = ops.spmm_bsr_bf16(a.tpattern, p[a.perm].transpose(1, 2).contiguous(), gb, out_bf16=True)
    dp = ops.sddmm_bsr_bf16(a.fwd, gb, bits(v))
    ds = ops.softmax_bsr_bwd(a.fwd, p, dp, scale=scale, out_bf16=True)
    dq = ops.spmm_bsr_bf16(a.fwd, ds, bits(k), out_bf16=True)
    dk = ops.spmm_bsr_bf16(a.tpattern, ds[a.perm].transpose(1, 2).contiguous(), bits(q), out_bf16=True)
    return out, dq, dk, dv


@functools.lru_cache(maxsize=None)
def attention_operands(name, d, dv):
    p = pattern(name)
    rng = np.random.default_rng(300 + d + 7 * dv)
    return (bf16_full_mantissa(rng, (p.num_rows, d)), bf16_full_mantissa(rng, (p.num_cols, d)), bf16_full_mantissa(rng, (p.num_cols, dv)),
            bf16_full_mantissa(rng, (p.num_rows, dv)))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d,dv", [(8, 64), (64, 8)])
@pytest.mark.parametrize("name", ["ragged16", "ragged32", "edges16"])
def test_block_sparse_attention_is_the_hand_called_chain(name, d, dv, out_dtype, causal):
    a = trainable(name)
    out_bf16 = out_dtype == torch.bfloat16
    qh, kh, vh, gh = attention_operands(name, d, dv)
    q, k, v = (bf(x).requires_grad_(True) for x in (qh, kh, vh))
    g = dev(gh).to(out_dtype)
    mask = dev(causal_mask(name)) if causal else None
    out = autograd.block_sparse_attention(a, q, k, v, mask=mask, out_dtype=out_dtype)
    assert out.dtype == out_dtype and out.shape == (a.fwd.num_rows, dv)
    out.backward(g)
    assert q.grad.dtype == k.grad.dtype == v.grad.dtype == torch.bfloat16
    want = hand_chain(a, q.detach(), k.detach(), v.detach(), g, d ** -0.5, mask, out_bf16)
    for what, got, w in zip(("out", "q.grad", "k.grad", "v.grad"), (out.detach(), q.grad, k.grad, v.grad), want):
        same_bits(bits(got) if got.dtype == torch.bfloat16 else got, w, f"{name} D={d} Dv={dv} {what}")


def with_data(bsr, data):
    return formats.BSR(bsr.num_rows, bsr.num_cols, bsr.nnz, bsr.block_row_size, bsr.block_col_size, bsr.block_row_ptrs, bsr.block_col_idxs, data)


def _dense_attention(bsr, q, k, v, g, scale, mask):
    """float64 dense masked attention with torch.autograd on the pattern (no pattern here repeats a block): (out, dq, dk, dv)
    as numpy arrays.  mask: [num_blocks, bS, bS] or None."""
    shape = (bsr.num_blocks, bsr.block_row_size, bsr.block_row_size)
    stored = torch.from_numpy(with_data(bsr, np.ones(shape)).to_dense() > 0)
    bias = torch.from_numpy(with_data(bsr, np.zeros(shape) if mask is None else mask.astype(np.float64)).to_dense())
    qt, kt, vt = (torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in (q, k, v))
    sc = ((qt @ kt.t()) * scale + bias).masked_fill(~stored, float("-inf"))
    p = torch.softmax(sc, dim=1).masked_fill(~stored.any(dim=1, keepdim=True), 0.0)      # a row without blocks: a zero row
    out = p @ vt
    out.backward(torch.from_numpy(g.astype(np.float64)))
    return out.detach().numpy(), qt.grad.numpy(), kt.grad.numpy(), vt.grad.numpy()


def _attention_tolerances(name, q, k, v, g, scale, mask, out_bf16):
    """Tolerances on (out, dq, dk, dv) of the bf16 chain, composed from the stated bounds by first-order error propagation in
    float64: each kernel's own bound at the exact values plus the bounds of the kernels before it carried through the step's
    derivative.  SDDMM: the bound of mispmm.h; softmax forward and backward: the bounds of mispmm.h; the two products: the
    any-order fp32 dot-product bound g_n S, g_n = n 2^-23 / (1 - n 2^-23), n the number of products of an element; 2^-8
    relative at every rounding to bf16 (P and dS inside their kernels' bounds; grad_out; bf16 outputs and the three
    gradients).  Second-order terms are covered by evaluating every propagated factor at (value + its own error) and by the
    factor 1.01 on the whole."""
    f64 = np.float64
    bsr = pattern(name)
    bs = bsr.block_row_size
    ptrs = bsr.block_row_ptrs.astype(np.int64)
    rows_of = np.repeat(np.arange(ptrs.shape[0] - 1), np.diff(ptrs))
    cols_of = bsr.block_col_idxs.astype(np.int64)
    within = np.arange(bs)
    q, k, v, g = (x.astype(f64) for x in (q, k, v, g))
    r8 = 2.0 ** -8
    dense = lambda blocks: with_data(bsr, blocks).to_dense()                               # noqa: E731
    length = lengths(name).astype(f64)
    row_ptrs, _ = layout(name)
    gamma = lambda n: n * 2.0 ** -23 / (1.0 - n * 2.0 ** -23)                              # noqa: E731
    n_row = np.repeat(np.diff(ptrs) * bs, bs).astype(f64)[:, None]                         # products of an element of A @ X
    n_col = np.repeat(np.bincount(cols_of, minlength=bsr.num_cols // bs) * bs, bs).astype(f64)[:, None]     # ... of A^T @ X

    def sampled(x, y):                                                                     # [num_blocks, bS, bS]: <x_r, y_c>
        return np.einsum("ein,ejn->eij", x[rows_of[:, None] * bs + within], y[cols_of[:, None] * bs + within])

    def per_row(blocks, ufunc=np.add):                                                     # a row's reduction, per element
        vr = to_rows(name, blocks)
        lens = np.diff(row_ptrs)
        red = ufunc.reduceat(vr, row_ptrs[:-1][lens > 0])
        out = np.empty_like(vr)
        out[:] = np.repeat(red, lens[lens > 0])
        flat = np.empty(blocks.size)
        flat[layout(name)[1]] = out
        return flat.reshape(blocks.shape)

    s, s_abs = sampled(q, k), sampled(np.abs(q), np.abs(k))
    e_s = sddmm_bsr_bound(False, q.shape[1], s, s_abs)
    bias = np.zeros_like(s) if mask is None else mask.astype(f64)
    z = scale * s + bias
    finite = np.isfinite(z)
    # z = fl32(fl32(scale) * s^ + mask): the scores' error through the factor, the rounded scale and the fma's rounding
    e_z = np.where(finite, scale * e_s + 2.0 ** -24 * np.abs(scale * s) + 2.0 ** -24 * np.abs(np.where(finite, z, 0.0)), 0.0)
    zr = np.where(finite, z, -np.inf)
    p = forward(name, zr, f64)[0]
    t = forward(name, zr, f64)[1]
    # a score error of at most e per element of a row moves every quotient by a factor within exp(+-2 e)
    e_row = per_row(e_z, np.maximum)
    shift = np.expm1(2 * e_row)
    e_p = p * shift + fwd_bound(True, length, t + 2 * e_row, p * (1 + shift))                # P is rounded to bf16 inside
    ph = p + e_p
    out = dense(p) @ v
    tol_out = gamma(n_row) * (dense(ph) @ np.abs(v)) + dense(e_p) @ np.abs(v)
    e_g = r8 * np.abs(g)                                                                    # grad_out rounded to bf16
    gh = np.abs(g) + e_g
    dv = dense(p).T @ g
    tol_dv = gamma(n_col) * (dense(ph).T @ gh) + dense(e_p).T @ gh + dense(p).T @ e_g
    dp, dp_abs = sampled(g, v), sampled(gh, np.abs(v))
    e_dp = sddmm_bsr_bound(False, v.shape[1], dp, dp_abs) + sampled(e_g, np.abs(v))
    ds = scale * p * (dp - per_row(p * dp))
    # dS = scale p (dP - <p, dP>): the kernel's bound (bf16 out) at the perturbed operands, then the operands' errors through the formula
    dph = np.abs(dp) + e_dp
    cap_h = per_row(ph * dph)
    e_dot = per_row(e_p * dph + ph * e_dp)
    e_ds = (bwd_bound(True, length, ph, dph, cap_h, scale, scale * ph * (dph + cap_h))
            + scale * (e_p * (dph + cap_h) + ph * (e_dp + e_dot)))
    dsh = np.abs(ds) + e_ds
    dq = dense(ds) @ k
    tol_dq = gamma(n_row) * (dense(dsh) @ np.abs(k)) + dense(e_ds) @ np.abs(k)
    dk = dense(ds).T @ q
    tol_dk = gamma(n_col) * (dense(dsh).T @ np.abs(q)) + dense(e_ds).T @ np.abs(q)
    rounded = lambda value, tol: tol + r8 * (np.abs(value) + tol)                          # noqa: E731  a result rounded to bf16
    tols = [rounded(out, tol_out) if out_bf16 else tol_out, rounded(dq, tol_dq), rounded(dk, tol_dk), rounded(dv, tol_dv)]
    return [1.01 * x + 1e-30 for x in tols]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d,dv", [(8, 64), (64, 8)])
@pytest.mark.parametrize("name", ["ragged16", "ragged32", "edges16"])
def test_block_sparse_attention_against_dense_masked_attention(name, d, dv, out_dtype, causal):
    a = trainable(name)
    bsr = pattern(name)
    qh, kh, vh, gh = attention_operands(name, d, dv)
    mask = causal_mask(name) if causal else None
    scale = d ** -0.5
    want = _dense_attention(bsr, qh, kh, vh, gh, scale, mask)
    q, k, v = (bf(x).requires_grad_(True) for x in (qh, kh, vh))
    out = autograd.block_sparse_attention(a, q, k, v, mask=None if mask is None else dev(mask), out_dtype=out_dtype)
    out.backward(dev(gh).to(out_dtype))
    got = [x.detach().float().cpu().numpy() for x in (out, q.grad, k.grad, v.grad)]
    tols = _attention_tolerances(name, qh, kh, vh, gh, scale, mask, out_dtype == torch.bfloat16)
    for what, gv, wv, tol in zip(("out", "dq", "dk", "dv"), got, want, tols):
        err = np.abs(gv.astype(np.float64) - wv)
        print(f"block attention {name} D={d} Dv={dv} {out_dtype} causal={causal} {what}: max |err| / tolerance = {float(np.max(err / tol)):.3g}")
        assert np.all(err <= tol), f"{name} D={d} Dv={dv} {out_dtype}: {what} outside the composed tolerance"


def test_frozen_inputs_skip_their_kernels():
    name = "ragged16"
    a = trainable(name)
    qh, kh, vh, _ = attention_operands(name, 8, 8)
    product = "bsr_mfma_bf16"
    # the tag of the last kernel is kept per thread: run the backward passes on this one
    with torch.autograd.set_multithreading_enabled(False):
        # block_softmax: the backward is the one softmax_bsr_bwd launch
        s = dev(scores("narrow", name)).requires_grad_(True)
        p = autograd.block_softmax(a, s, scale=0.3)
        assert capi.last_kernel().startswith("softmax_bsr<")
        p.sum().backward()
        assert capi.last_kernel().startswith("softmax_bsr_bwd<"), capi.last_kernel()
        assert s.grad is not None
        p = autograd.block_softmax(a, s.detach())
        assert p.grad_fn is None and not p.requires_grad
        # only v trainable: the backward is the product with A^T alone -- no SDDMM for dP, no softmax backward
        q, k, v = bf(qh), bf(kh), bf(vh).requires_grad_(True)
        out = autograd.block_sparse_attention(a, q, k, v)
        assert capi.last_kernel().startswith(product), capi.last_kernel()
        ops.softmax_bsr_bwd(a.fwd, p, p)                                             # leave a tag behind ...
        assert capi.last_kernel().startswith("softmax_bsr_bwd<")
        seen = []
        real_sddmm, real_bwd = ops.sddmm_bsr_bf16, ops.softmax_bsr_bwd
        try:
            ops.sddmm_bsr_bf16 = lambda *args, **kw: (seen.append("sddmm"), real_sddmm(*args, **kw))[1]
            ops.softmax_bsr_bwd = lambda *args, **kw: (seen.append("softmax_bwd"), real_bwd(*args, **kw))[1]
            out.sum().backward()
            assert capi.last_kernel().startswith(product), capi.last_kernel()       # ... which the one product replaces
            assert seen == [] and v.grad is not None and q.grad is None and k.grad is None
            # only q trainable: SDDMM (dP), softmax backward, then the product for dq; nothing for k or v
            q, k, v = bf(qh).requires_grad_(True), bf(kh), bf(vh)
            out = autograd.block_sparse_attention(a, q, k, v)
            del seen[:]                                                              # the forward's own SDDMM
            out.sum().backward()
            assert seen == ["sddmm", "softmax_bwd"] and capi.last_kernel().startswith(product), (seen, capi.last_kernel())
            assert q.grad is not None and k.grad is None and v.grad is None
            # only k trainable: the same two, then the product with A^T
            q, k, v = bf(qh), bf(kh).requires_grad_(True), bf(vh)
            out = autograd.block_sparse_attention(a, q, k, v)
            del seen[:]
            out.sum().backward()
            assert seen == ["sddmm", "softmax_bwd"] and k.grad is not None and q.grad is None and v.grad is None
        finally:
            ops.sddmm_bsr_bf16, ops.softmax_bsr_bwd = real_sddmm, real_bwd
    out = autograd.block_sparse_attention(a, bf(qh), bf(kh), bf(vh))
    assert out.grad_fn is None and not out.requires_grad
    with pytest.raises(ValueError):
        autograd.block_sparse_attention(a, bf(qh).float(), bf(kh), bf(vh))
    with pytest.raises(ValueError):
        autograd.block_softmax(a, dev(scores("narrow", name)).double())
