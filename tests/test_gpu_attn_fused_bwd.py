"""The fused block-sparse attention backward (mispmm_attn_bsr_bwd_bf16, ops.attention_bsr_bwd_bf16,
block_sparse_attention(fused=True, fused_backward=True)) on the GPU.  References and tolerances: tests/_attn_fused_bwd_ref.py --
dq, dk and dv against float64 dense masked attention (torch.autograd in float64) inside bwd_tolerances, the bound derived from
the header's by first-order propagation; nothing is measured into it.  The numerical checks are the functions of
tests/_attn_checks.py, which tests/test_attn_mutants_cpu.py runs deliberately faulty restatements through; the tighter, derived
check on the kernel's own out and lse: tests/test_gpu_attn_tight.py.

Worst |err| / tolerance printed on an MI355X (`-s` prints every one): fp32 gradients dq 0.227,
dk 0.286, dv 0.783; bf16 gradients dq 0.299, dk 0.407, dv 0.781 (dv: the rounding of P to bf16, 2^-9 against the 2^-8 of the bound)."""
import functools
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi_attn_bwd, ops  # noqa: E402

import _attn_checks as checks  # noqa: E402
import _attn_fused_bwd_ref as ref  # noqa: E402
from _attn_checks import Case  # noqa: E402
from _sddmm_bsr_ref import from_bits, to_bits  # noqa: E402
from test_gpu_softmax_bsr import _attention_tolerances, _dense_attention, bf, bits, dev, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINELS = 64


def dbits(v):
    """float32 host array of bf16 numbers -> int16 device tensor of their bits."""
    return dev(to_bits(v))


def host(t):
    a = t.cpu().numpy()
    return from_bits(a) if a.dtype == np.int16 else a


@functools.lru_cache(maxsize=None)
def device(name):
    """(A, A^T, perm as int32) on the device."""
    a, at, perm = ref.bwd_pattern(name)
    return ops.DeviceBSR.from_host(a), ops.DeviceBSR.from_host(at), dev(np.ascontiguousarray(perm, dtype=np.uint32).view(np.int32))


@functools.lru_cache(maxsize=None)
def trainable(name):
    return autograd.TrainableBSR.from_host(ref.bwd_pattern(name)[0])


def dmask(name, kind):
    m = ref.mask_of(name, kind)
    return None if m is None else dev(m)


def exact(name, d, dv, kind):
    """float64 (dq, dk, dv) of head 0 of ref.operands(name, d, dv); read-only."""
    return checks.backward_exact(Case(name, d, dv, kind, src="bwd"))


def forward(name, q, k, v, mask, out_bf16, scale=None):
    return ops.attention_bsr_bf16(device(name)[0], q, k, v, scale=scale, mask=mask, out_bf16=out_bf16, return_lse=True)


def backward(name, q, k, v, out, lse, g, mask, **kw):
    a, at, perm = device(name)
    return ops.attention_bsr_bwd_bf16(a, at, perm, q, k, v, out, lse, g, mask=mask, **kw)


def empty_block_rows(bsr):
    return np.repeat(np.diff(np.asarray(bsr.block_row_ptrs, dtype=np.int64)) == 0, bsr.block_row_size)


def no_bits(t, rows):
    a = t.cpu().numpy()
    return not a.view(np.uint16 if a.dtype == np.int16 else np.uint32)[rows].any()


@pytest.mark.parametrize("kind", ref.MASKS)
@pytest.mark.parametrize("d,dv", ref.WIDTHS)
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_gradients_against_float64_dense_masked_attention(name, d, dv, kind):
    bsr, tbsr, _ = ref.bwd_pattern(name)
    qh, kh, vh, gh = (x[0] for x in ref.operands(name, d, dv))
    q, k, v, g = (dbits(x) for x in (qh, kh, vh, gh))
    mask = dmask(name, kind)
    for out_bf16 in (False, True):
        out, lse = forward(name, q, k, v, mask, out_bf16)
        for grads_bf16 in (False, True):
            got = backward(name, q, k, v, out, lse, g, mask, grads_bf16=grads_bf16)
            tag = capi_attn_bwd.last_kernel()
            assert tag == ref.tag_of(bsr.block_row_size, d, dv, mask is not None), tag
            for what, x, rows in zip(("dq", "dk", "dv"), got, (bsr.num_rows, bsr.num_cols, bsr.num_cols)):
                assert x.dtype == (torch.int16 if grads_bf16 else torch.float32) and x.shape == (rows, dv if what == "dv" else d)
            # the check of tests/_attn_checks.py: the function tests/test_attn_mutants_cpu.py runs the faulty restatements through
            case = Case(name, d, dv, kind, src="bwd", out_bf16=out_bf16, grads_bf16=grads_bf16)
            ok, worst = checks.bwd_composed(dict(dq=host(got[0]), dk=host(got[1]), dv=host(got[2])), case)
            for what, w in zip(("dq", "dk", "dv"), worst):
                print(f"fused backward {name} D={d} Dv={dv} {kind} out_bf16={out_bf16} grads_bf16={grads_bf16} {what}: max |err| / tolerance = {w:.3g}")
            assert ok, f"{name} D={d} Dv={dv} {kind} out_bf16={out_bf16} grads_bf16={grads_bf16}: a gradient outside the derived tolerance {worst}"


@pytest.mark.parametrize("grads_bf16", [False, True])
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_empty_block_rows_and_columns_and_masked_columns_give_plus_zero_bits(name, grads_bf16):
    bsr, tbsr, perm = ref.bwd_pattern(name)
    bs = bsr.block_row_size
    q, k, v, g = (dbits(x[0]) for x in ref.operands(name, 40, 72))
    out, lse = forward(name, q, k, v, None, False)
    dq, dk, dv = backward(name, q, k, v, out, lse, g, None, grads_bf16=grads_bf16)
    empty_rows, empty_cols = empty_block_rows(bsr), empty_block_rows(tbsr)
    assert empty_rows.any() or name.startswith("edgesT")
    assert no_bits(dq, empty_rows) and bool((dq.view(torch.int16 if grads_bf16 else torch.int32)[torch.from_numpy(~empty_rows).cuda()] != 0).any(dim=1).all())
    if name.startswith("edgesT"):
        assert empty_cols[0] and empty_cols[-1]
    assert no_bits(dk, empty_cols) and no_bits(dv, empty_cols)
    assert checks.backward_zero_rows(dict(dq=host(dq), dk=host(dk), dv=host(dv)), Case(name, 40, 72, "none", src="bwd", grads_bf16=grads_bf16))[0]
    # -Inf over every block of some block columns (every second non-empty one; every matrix row keeps a finite key or was empty)
    m, blank = checks.blank_columns_mask(bsr, tbsr)
    md = dev(m)
    out, lse = forward(name, q, k, v, md, False)
    assert bool(torch.isfinite(lse[torch.from_numpy(~empty_rows).cuda()]).all())
    dq, dk, dv = backward(name, q, k, v, out, lse, g, md, grads_bf16=grads_bf16)
    masked = np.repeat(blank, bs)
    assert no_bits(dk, masked | empty_cols) and no_bits(dv, masked | empty_cols)
    for t in (dq, dk, dv):
        assert not np.isnan(host(t)).any()
    assert checks.backward_zero_rows(dict(dq=host(dq), dk=host(dk), dv=host(dv)), Case(name, 40, 72, "blankcols", src="bwd", grads_bf16=grads_bf16))[0]


@pytest.mark.parametrize("name", ["ragged16", "edgesT32"])
def test_heads_with_strides_equal_single_head_calls_and_sentinels_survive(name):
    """H = 3 from [rows, H, width] tensors permuted against three 2-D calls, bit for bit; the gradients as strided slices of wider
    buffers with sentinels in the gaps and either side; delta between sentinels."""
    bsr = ref.bwd_pattern(name)[0]
    d, dv, heads = 40, 72, 3
    qh, kh, vh, gh = ref.operands(name, d, dv, heads)
    mask = dmask(name, "causal")
    q, k, v, g = (dbits(np.ascontiguousarray(x.transpose(1, 0, 2))).permute(1, 0, 2) for x in (qh, kh, vh, gh))
    assert q.stride() == (d, heads * d, 1) and not q.is_contiguous()
    for out_bf16, grads_bf16 in ((False, False), (True, True)):
        out, lse = forward(name, q, k, v, mask, out_bf16)
        out = out.permute(1, 0, 2).contiguous().permute(1, 0, 2)              # out strided as [M, H, Dv] too
        singles = []
        for h in range(heads):
            o1, l1 = forward(name, dbits(qh[h]), dbits(kh[h]), dbits(vh[h]), mask, out_bf16)
            same_bits(o1, out[h].contiguous(), "the forward of one head")
            singles.append(backward(name, dbits(qh[h]), dbits(kh[h]), dbits(vh[h]), o1, l1, dbits(gh[h]), mask, grads_bf16=grads_bf16))
        got = backward(name, q, k, v, out, lse, g, mask, grads_bf16=grads_bf16)
        for what, x, rows, width in zip(("dq", "dk", "dv"), got, (bsr.num_rows, bsr.num_cols, bsr.num_cols), (d, d, dv)):
            assert x.shape == (heads, rows, width)
            for h in range(heads):
                same_bits(x[h], singles[h][("dq", "dk", "dv").index(what)], f"{name} {what} head {h} of 3 against a call of its own")
        # the gradients as [M, H, 80] buffers of which [:, h, :width] is written, inside longer buffers
        mark = 0x1234 if grads_bf16 else -7.0
        dtype = torch.int16 if grads_bf16 else torch.float32
        wide = 80
        bufs, views = [], []
        for rows, width in ((bsr.num_rows, d), (bsr.num_cols, d), (bsr.num_cols, dv)):
            buf = torch.full((SENTINELS + rows * heads * wide + SENTINELS,), mark, dtype=dtype, device="cuda")
            bufs.append(buf)
            views.append(buf[SENTINELS:SENTINELS + rows * heads * wide].view(rows, heads, wide).permute(1, 0, 2))
        dbuf = torch.full((SENTINELS + heads * bsr.num_rows + SENTINELS,), -7.0, device="cuda")
        delta = dbuf[SENTINELS:SENTINELS + heads * bsr.num_rows].view(heads, bsr.num_rows)
        again = backward(name, q, k, v, out, lse, g, mask, grads_bf16=grads_bf16, dq=views[0][:, :, :d], dk=views[1][:, :, :d], dv=views[2][:, :, :dv],
                         delta=delta)
        for what, x, view, buf, width in zip(("dq", "dk", "dv"), got, views, bufs, (d, d, dv)):
            assert again[("dq", "dk", "dv").index(what)].data_ptr() == view.data_ptr()
            same_bits(view[:, :, :width].contiguous(), x, f"{name} {what} inside a strided buffer")
            assert bool((view[:, :, width:] == mark).all()), f"a padding column of the strided {what} was written"
            assert bool((buf[:SENTINELS] == mark).all()) and bool((buf[-SENTINELS:] == mark).all()), f"a sentinel of {what} was written"
        assert bool((dbuf[:SENTINELS] == -7.0).all()) and bool((dbuf[-SENTINELS:] == -7.0).all()), "a sentinel of delta was written"
        want_delta = (host(g.contiguous()).astype(np.float64) * host(out.contiguous()).astype(np.float64)).sum(axis=2)
        assert np.allclose(delta.cpu().numpy(), want_delta, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("name,kind", [("edges16", "causal"), ("edgesT32", "none")])
def test_every_subset_of_need_has_the_bits_of_the_call_for_all_three(name, kind):
    q, k, v, g = (dbits(x[0]) for x in ref.operands(name, 64, 64))
    mask = dmask(name, kind)
    bs = ref.bwd_pattern(name)[0].block_row_size
    out, lse = forward(name, q, k, v, mask, True)
    full = backward(name, q, k, v, out, lse, g, mask)
    subsets = {}
    for need in itertools.product((False, True), repeat=3):
        got = backward(name, q, k, v, out, lse, g, mask, need=need)
        if any(need):
            assert capi_attn_bwd.last_kernel() == ref.tag_of(bs, 64, 64, mask is not None, need)
        for what, wanted, x, w in zip(("dq", "dk", "dv"), need, got, full):
            if wanted:
                same_bits(x, w, f"{name} {what} with need={need}")
            else:
                assert x is None
        subsets[need] = tuple(None if x is None else host(x) for x in got)
    assert checks.subsets_equal(dict(dq=host(full[0]), dk=host(full[1]), dv=host(full[2]), subsets=subsets), Case(name, 64, 64, kind, src="bwd", out_bf16=True, grads_bf16=True))[0]
    # dv alone needs neither delta nor out's row pass: perm is not needed without a mask either
    if mask is None:
        a, at, _ = device(name)
        alone = ops.attention_bsr_bwd_bf16(a, at, None, q, k, v, out, lse, g, need=(False, False, True))
        same_bits(alone[2], full[2], "dv alone, perm=None")


def test_deterministic_and_replays_from_a_graph():
    name = "edgesT16"
    q, k, v, g = (dbits(x) for x in ref.operands(name, 64, 64, 2))
    mask = dmask(name, "causal")
    out, lse = forward(name, q, k, v, mask, True)
    first = [x.clone() for x in backward(name, q, k, v, out, lse, g, mask)]
    again = backward(name, q, k, v, out, lse, g, mask)
    for what, x, w in zip(("dq", "dk", "dv"), again, first):
        same_bits(x, w, f"second run, {what}")
    held = [torch.empty_like(x) for x in first]
    delta = torch.empty_like(lse)
    kw = dict(dq=held[0], dk=held[1], dv=held[2], delta=delta)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture
        backward(name, q, k, v, out, lse, g, mask, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # two launches on one stream: no parallel branches
        backward(name, q, k, v, out, lse, g, mask, **kw)
    for _ in range(2):
        for x in held:
            x.zero_()
        delta.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for what, x, w in zip(("dq", "dk", "dv"), held, first):
            same_bits(x, w, f"graph replay, {what}")


def test_every_tag_of_the_table_is_reached_by_its_shape():
    seen = set()
    for bs, d, dv, with_mask in sorted(set(ref.TAGS.values())):
        name = f"ragged{bs}"
        q, k, v, g = (dbits(x[0]) for x in ref.operands(name, d, dv))
        mask = dmask(name, "causal") if with_mask else None
        out, lse = forward(name, q, k, v, mask, False)
        for need, tag in (((True, False, False), ref.rows_tag(bs, d, dv, with_mask)), ((False, False, True), ref.cols_tag(bs, d, dv, with_mask))):
            got = backward(name, q, k, v, out, lse, g, mask, need=need)
            assert capi_attn_bwd.last_kernel() == tag and ref.TAGS[tag] == (bs, d, dv, with_mask), (capi_attn_bwd.last_kernel(), tag)
            seen.add(tag)
            assert not any(np.isnan(host(x)).any() for x in got if x is not None)
    assert seen == set(ref.TAGS)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["ragged16", "edges32"])
def test_autograd_single_head_is_the_ops_call_and_close_to_the_unfused_path(name, out_dtype):
    d, dv = 64, 64
    a = trainable(name)
    qh, kh, vh, gh = (x[0] for x in ref.operands(name, d, dv))
    mask, mh = dmask(name, "causal"), ref.mask_of(name, "causal")
    out_bf16 = out_dtype == torch.bfloat16
    grads = {}
    for fused_backward in (False, True):
        q, k, v = (bf(x).requires_grad_(True) for x in (qh, kh, vh))
        out = autograd.block_sparse_attention(a, q, k, v, mask=mask, out_dtype=out_dtype, fused=True, fused_backward=fused_backward)
        assert out.dtype == out_dtype
        with torch.autograd.set_multithreading_enabled(False):    # the tag is per thread: keep the backward on this one
            out.backward(dev(gh).to(out_dtype))                   # bf16 numbers: exact in either type
        if fused_backward:
            assert capi_attn_bwd.last_kernel() == ref.tag_of(a.fwd.block_row_size, d, dv, True)
        grads[fused_backward] = (out.detach(), q.grad, k.grad, v.grad)
    for x, y in zip(grads[True][0:1], grads[False][0:1]):
        same_bits(bits(x) if out_bf16 else x, bits(y) if out_bf16 else y, "the forward with and without lse")
    o, lse = forward(name, dbits(qh), dbits(kh), dbits(vh), mask, out_bf16)
    direct = backward(name, dbits(qh), dbits(kh), dbits(vh), o, lse, dbits(gh), mask)
    fused_tol = ref.bwd_tolerances(name, qh, kh, vh, gh, d ** -0.5, mh, out_bf16, True)
    chain_tol = _attention_tolerances(name, qh, kh, vh, gh, d ** -0.5, mh, out_bf16)[1:]
    for what, x, y, w, t1, t2 in zip(("dq", "dk", "dv"), grads[True][1:], grads[False][1:], direct, fused_tol, chain_tol):
        assert x.dtype == torch.bfloat16
        same_bits(bits(x), w, f"autograd {what} against the direct ops call")
        diff = np.abs(x.float().cpu().numpy().astype(np.float64) - y.float().cpu().numpy().astype(np.float64))
        print(f"autograd {name} {out_dtype} {what}: max |fused - unfused| / (sum of the tolerances) = {float(np.max(diff / (t1 + t2))):.3g}")
        assert np.all(diff <= t1 + t2), f"{what}: the two backward paths are further apart than both tolerances"


@pytest.mark.parametrize("name", ["edges16", "edgesT32"])
def test_a_float32_grad_out_is_rounded_to_bf16_and_stays_inside_the_tolerance_with_its_rounding_term(name):
    """grad_out with all 24 significant bits: the backward rounds it to bf16 (ops.f32_to_bf16), the float64 reference keeps it as
    it is, and bwd_tolerances carries E_g = 2^-8 |grad_out| (g_rounded=True)."""
    d, dv = 40, 72
    a = trainable(name)
    bsr = ref.bwd_pattern(name)[0]
    qh, kh, vh, _ = (x[0] for x in ref.operands(name, d, dv))
    rng = np.random.default_rng(91)
    g32 = (np.where(rng.random((bsr.num_rows, dv)) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, (bsr.num_rows, dv))).astype(np.float32)
    assert (g32.view(np.uint32) & 0xFFFF).any()
    mask, mh = dmask(name, "causal"), ref.mask_of(name, "causal")
    q, k, v = (bf(x).requires_grad_(True) for x in (qh, kh, vh))
    out = autograd.block_sparse_attention(a, q, k, v, mask=mask, fused=True, fused_backward=True)
    out.backward(dev(g32))
    want = _dense_attention(bsr, qh, kh, vh, g32, d ** -0.5, mh)[1:]
    tols = ref.bwd_tolerances(name, qh, kh, vh, g32, d ** -0.5, mh, False, True, g_rounded=True)
    o, lse = forward(name, dbits(qh), dbits(kh), dbits(vh), mask, False)
    direct = backward(name, dbits(qh), dbits(kh), dbits(vh), o, lse, ops.f32_to_bf16(dev(g32)), mask)
    for what, x, w, tol, y in zip(("dq", "dk", "dv"), (q.grad, k.grad, v.grad), want, tols, direct):
        same_bits(bits(x), y, f"{what}: autograd against the ops call on the rounded grad_out")
        err = np.abs(x.float().cpu().numpy().astype(np.float64) - w)
        print(f"float32 grad_out {name} {what}: max |err| / tolerance = {float(np.max(err / tol)):.3g}")
        assert np.all(err <= tol), f"{what} outside the tolerance with the rounding of grad_out"


def test_autograd_with_heads_and_frozen_inputs():
    name, d, dv, heads = "ragged32", 40, 72, 2
    a = trainable(name)
    qh, kh, vh, gh = ref.operands(name, d, dv, heads)
    q, k, v = (bf(x).requires_grad_(True) for x in (qh, kh, vh))
    out = autograd.block_sparse_attention(a, q, k, v, fused=True, fused_backward=True)
    assert out.shape == (heads, a.fwd.num_rows, dv)
    out.backward(dev(gh))                                         # float32 holding bf16 numbers: the rounding is exact
    o, lse = forward(name, dbits(qh), dbits(kh), dbits(vh), None, False)
    direct = backward(name, dbits(qh), dbits(kh), dbits(vh), o, lse, dbits(gh), None)
    for what, x, w in zip(("dq", "dk", "dv"), (q.grad, k.grad, v.grad), direct):
        same_bits(bits(x), w, f"H = 2 autograd {what} against the direct ops call")
    for h in range(heads):                                       # every head against the unfused path's 2-D call
        q1, k1, v1 = (bf(x[h]).requires_grad_(True) for x in (qh, kh, vh))
        autograd.block_sparse_attention(a, q1, k1, v1).backward(dev(gh[h]))
        t1 = ref.bwd_tolerances(name, qh[h], kh[h], vh[h], gh[h], d ** -0.5, None, False, True)
        t2 = _attention_tolerances(name, qh[h], kh[h], vh[h], gh[h], d ** -0.5, None, False)[1:]
        for what, x, y, ta, tb in zip(("dq", "dk", "dv"), (q.grad[h], k.grad[h], v.grad[h]), (q1.grad, k1.grad, v1.grad), t1, t2):
            diff = np.abs(x.float().cpu().numpy().astype(np.float64) - y.float().cpu().numpy().astype(np.float64))
            assert np.all(diff <= ta + tb), f"head {h} {what}"
    # frozen inputs get None and their output pointers are passed null: the call made is the call for their `need`
    calls = []
    real = ops.attention_bsr_bwd_bf16
    with torch.autograd.set_multithreading_enabled(False):
        try:
            ops.attention_bsr_bwd_bf16 = lambda *args, **kw: (calls.append(kw["need"]), real(*args, **kw))[1]
            for need in ((False, False, True), (True, False, False), (False, True, True)):
                ins = [bf(x).requires_grad_(n) for x, n in zip((qh, kh, vh), need)]
                autograd.block_sparse_attention(a, *ins, fused=True, fused_backward=True).backward(dev(gh))
                assert calls[-1] == need and capi_attn_bwd.last_kernel() == ref.tag_of(32, d, dv, False, need)
                for t, n, w in zip(ins, need, direct):
                    if n:
                        same_bits(bits(t.grad), w, f"need={need}")
                    else:
                        assert t.grad is None
        finally:
            ops.attention_bsr_bwd_bf16 = real
    out = autograd.block_sparse_attention(a, bf(qh), bf(kh), bf(vh), fused=True, fused_backward=True)
    assert out.grad_fn is None and not out.requires_grad
    with pytest.raises(ValueError, match="needs fused=True"):
        autograd.block_sparse_attention(a, bf(qh[0]), bf(kh[0]), bf(vh[0]), fused_backward=True)


def test_activsg10k_two_heads_against_the_parents_backward():
    """16 x 16, 33100 blocks.  bf16 out: every gradient element within the sum of the two paths' tolerances, bwd_tolerances and
    the three-launch chain's composed ones, both evaluated block by block.  No dense reference exists at this size."""
    name, d, heads = "ACTIVSg10K", 64, 2
    a = trainable(name)
    qh, kh, vh, gh = ref.operands(name, d, d, heads)
    grads = {}
    for fused_backward in (False, True):
        q, k, v = (bf(x).requires_grad_(True) for x in (qh, kh, vh))
        out = autograd.block_sparse_attention(a, q, k, v, out_dtype=torch.bfloat16, fused=True, fused_backward=fused_backward)
        with torch.autograd.set_multithreading_enabled(False):    # the tag is per thread: keep the backward on this one
            out.backward(dev(gh).to(torch.bfloat16))
        grads[fused_backward] = (q.grad, k.grad, v.grad)
    assert capi_attn_bwd.last_kernel() == ref.tag_of(16, d, d, False), capi_attn_bwd.last_kernel()
    worst = {}
    for h in range(heads):
        t1 = ref.bwd_tolerances(name, qh[h], kh[h], vh[h], gh[h], d ** -0.5, None, True, True)
        t2 = ref.chain_grad_tolerances(name, qh[h], kh[h], vh[h], gh[h], d ** -0.5, None)
        for what, x, y, ta, tb in zip(("dq", "dk", "dv"), grads[True], grads[False], t1, t2):
            diff = np.abs(x[h].float().cpu().numpy().astype(np.float64) - y[h].float().cpu().numpy().astype(np.float64))
            worst[what] = max(worst.get(what, 0.0), float(np.max(diff / (ta + tb))))
            assert np.all(diff <= ta + tb), f"head {h} {what}: fused and parent backward further apart than both tolerances"
    print("ACTIVSg10K fused backward against the parent's: max |difference| / (sum of the tolerances) = "
          + ", ".join(f"{w} {r:.3g}" for w, r in worst.items()))
