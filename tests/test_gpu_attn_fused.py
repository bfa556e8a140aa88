"""The fused block-sparse attention forward (mispmm_attn_bsr_bf16, ops.attention_bsr_bf16, block_sparse_attention(fused=True))
on the GPU.  References and tolerances: tests/_attn_fused_ref.py -- out against float64 dense masked attention inside the `out`
component of the three-launch chain's composed tolerance (no term added), lse against float64 logsumexp inside
1.01 (E_z + (L + 8 T + 16) u + 2 u (|lse| + ln L + 1)).  The numerical checks are the functions of tests/_attn_checks.py, which
tests/test_attn_mutants_cpu.py runs deliberately faulty restatements through; the tighter, derived check: tests/test_gpu_attn_tight.py.

Worst |err| / tolerance printed on an MI355X (`-s` prints every one): out fp32 0.428, bf16 0.483;
lse 0.040; a constant V 0.045 of (L + 16) 2^-24; ACTIVSg10K against the three-launch chain 0.425 of the two tolerances' sum."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, capi_attn, ops  # noqa: E402

import _attn_checks as checks  # noqa: E402
import _attn_fused_ref as ref  # noqa: E402
from _attn_checks import Case  # noqa: E402
from _sddmm_bsr_ref import from_bits, full_mantissa, to_bits  # noqa: E402
from _softmax_bsr_ref import pattern  # noqa: E402
from test_gpu_softmax_bsr import bf, bits, dev, device_bsr, same_bits, trainable  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINELS = 64


def dbits(v):
    """float32 host array of bf16 numbers -> int16 device tensor of their bits."""
    return dev(to_bits(v))


def host(out):
    a = out.cpu().numpy()
    return from_bits(a) if a.dtype == np.int16 else a


def reference(name, d, dv, kind):
    """(float64 out, {out_bf16: tolerance}, exact lse, its tolerance) of head 0 of ref.operands(name, d, dv); read-only."""
    return checks.forward_reference(Case(name, d, dv, kind))


def empty_rows(name):
    p = pattern(name)
    return np.repeat(np.diff(p.block_row_ptrs.astype(np.int64)) == 0, p.block_row_size)


@pytest.mark.parametrize("kind", ref.MASKS)
@pytest.mark.parametrize("d,dv", ref.WIDTHS)
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_out_and_lse_against_float64_dense_masked_attention(name, d, dv, kind):
    a = device_bsr(name)
    q, k, v = (dbits(x[0]) for x in ref.operands(name, d, dv))
    mask = ref.mask_of(name, kind)
    md = None if mask is None else dev(mask)
    empty = empty_rows(name)
    for out_bf16 in (False, True):
        out, lse = ops.attention_bsr_bf16(a, q, k, v, mask=md, out_bf16=out_bf16, return_lse=True)
        tag = capi_attn.last_kernel()
        assert tag == ref.tag_of(a.block_row_size, d, dv, mask is not None, out_bf16), tag
        assert out.shape == (a.num_rows, dv) and out.dtype == (torch.int16 if out_bf16 else torch.float32) and lse.shape == (a.num_rows,)
        # the checks of tests/_attn_checks.py: the functions tests/test_attn_mutants_cpu.py runs the faulty restatements through
        case, got = Case(name, d, dv, kind, out_bf16=out_bf16), dict(out=host(out), lse=lse.cpu().numpy())
        ok, worst = checks.out_composed(got, case)
        print(f"fused attention {name} D={d} Dv={dv} {kind} {tag} out: max |err| / tolerance = {worst:.3g}")
        assert ok, f"{name} D={d} Dv={dv} {kind} bf16={out_bf16}: out outside the composed tolerance"
        # an empty block row: +0 rows and lse = -Inf
        assert empty.any() and not out.cpu().numpy().view(np.uint16 if out_bf16 else np.uint32)[empty].any() and checks.forward_zero_rows(got, case)[0]
        assert np.array_equal(np.isneginf(got["lse"]), empty)
        ok, worst = checks.lse_bound(got, case)
        print(f"fused attention {name} D={d} Dv={dv} {kind} {tag} lse: max |err| / tolerance = {worst:.3g}")
        assert ok, f"{name} D={d} Dv={dv} {kind}: lse outside its bound"


@pytest.mark.parametrize("name", ["edges16", "edges32"])
def test_a_constant_v_comes_back_to_fp32_accuracy(name):
    """l is summed from the bf16 weights the product multiplies by: out = value to within (L + 16) 2^-24 relative."""
    a, p = device_bsr(name), pattern(name)
    q, k, _ = (dbits(x[0]) for x in ref.operands(name, 64, 64))
    length = np.repeat(np.diff(p.block_row_ptrs.astype(np.int64)) * p.block_row_size, p.block_row_size).astype(np.float64)
    rows = length > 0
    for dv in (64, 128):
        for value in (1.0, -0.34765625):
            v = dbits(np.full((p.num_cols, dv), value, np.float32))
            out = ops.attention_bsr_bf16(a, q, k, v, mask=dev(ref.mask_of(name, "causal"))).cpu().numpy()
            ok, worst = checks.constant_v(dict(out=out), Case(name, 64, dv, "causal", const_v=value))
            print(f"constant V {name} Dv={dv} value={value}: max rel / ((L + 16) u) = {worst:.3g}")
            assert ok and rows.any()


@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_special_values_stay_in_their_matrix_row(name, out_bf16):
    """A NaN, a +Inf, both, and an all -Inf row, each injected through the mask into ONE matrix row of the first, the longest
    and the last non-empty block row: exactly that row of out is NaN, lse is what torch.logsumexp gives, and every other row
    -- the other rows of the same blocks included -- keeps the bits of the clean run."""
    p, a = pattern(name), device_bsr(name)
    bs = p.block_row_size
    ptrs = p.block_row_ptrs.astype(np.int64)
    counts = np.diff(ptrs)
    filled = np.argwhere(counts > 0).ravel()
    targets = sorted({int(filled[0]), int(np.argmax(counts)), int(filled[-1])})
    q, k, v = (dbits(x[0]) for x in ref.operands(name, 40, 72))
    base = ref.mask_of(name, "causal")
    clean, clean_lse = (x.cpu().numpy() for x in ops.attention_bsr_bf16(a, q, k, v, scale=0.3, mask=dev(base), out_bf16=out_bf16, return_lse=True))
    nan_of = lambda x: np.isnan(from_bits(x) if out_bf16 else x)   # noqa: E731
    assert not nan_of(clean).any()
    for t, r in enumerate(targets):
        i = (11 * t + 3) % bs                                   # 3, 14, 25 (9 at 16 x 16): both halves of a 32 x 32 block
        for what, want_lse in (("nan", np.nan), ("+inf", np.inf), ("nan and +inf", np.nan), ("all -inf", -np.inf)):
            m = base.copy()
            if "nan" in what:
                m[ptrs[r] + counts[r] // 2, i, bs - 1] = np.nan
            if "+inf" in what:
                m[ptrs[r + 1] - 1, i, 0] = np.inf
            if what == "all -inf":
                m[ptrs[r]:ptrs[r + 1], i, :] = -np.inf
            got, lse = (x.cpu().numpy() for x in ops.attention_bsr_bf16(a, q, k, v, scale=0.3, mask=dev(m), out_bf16=out_bf16, return_lse=True))
            hit = np.zeros(p.num_rows, bool)
            hit[r * bs + i] = True
            assert np.array_equal(nan_of(got), np.broadcast_to(hit[:, None], got.shape)), f"{what} in row {i} of block row {r}: NaN positions differ"
            assert np.array_equal(got[~hit], clean[~hit]) and np.array_equal(lse[~hit], clean_lse[~hit]), f"{what} in row {i} of block row {r}: another row changed"
            assert np.array_equal(lse[hit], np.array([want_lse], np.float32), equal_nan=True), f"{what}: lse {lse[hit]}"


@pytest.mark.parametrize("name", ["ragged16", "edges32"])
def test_heads_with_strides_equal_single_head_calls_and_sentinels_survive(name):
    """H = 3 from [rows, H, width] tensors permuted (head stride = width, row stride = 3 width) against three 2-D calls, bit
    for bit; out as a strided slice of a wider buffer with sentinels in the gaps and either side, lse between sentinels."""
    a, p = device_bsr(name), pattern(name)
    d, dv, heads = 40, 72, 3
    qh, kh, vh = ref.operands(name, d, dv, heads)
    mask = dev(ref.mask_of(name, "causal"))
    q, k, v = (dbits(np.ascontiguousarray(x.transpose(1, 0, 2))).permute(1, 0, 2) for x in (qh, kh, vh))
    assert q.stride() == (d, heads * d, 1) and not q.is_contiguous()
    for out_bf16 in (False, True):
        singles = [ops.attention_bsr_bf16(a, dbits(qh[h]), dbits(kh[h]), dbits(vh[h]), mask=mask, out_bf16=out_bf16, return_lse=True) for h in range(heads)]
        out, lse = ops.attention_bsr_bf16(a, q, k, v, mask=mask, out_bf16=out_bf16, return_lse=True)
        assert out.shape == (heads, p.num_rows, dv) and lse.shape == (heads, p.num_rows)
        for h in range(heads):
            same_bits(out[h], singles[h][0], f"{name} head {h} of 3 against a call of its own")
            same_bits(lse[h], singles[h][1], f"{name} lse of head {h}")
        # out: [H, M, 80] rows of which columns 0 .. 71 are written, inside a longer buffer
        mark = 0x1234 if out_bf16 else -7.0
        dtype = torch.int16 if out_bf16 else torch.float32
        wide = 80
        buf = torch.full((SENTINELS + heads * p.num_rows * wide + SENTINELS,), mark, dtype=dtype, device="cuda")
        view = buf[SENTINELS:SENTINELS + heads * p.num_rows * wide].view(heads, p.num_rows, wide)
        lbuf = torch.full((SENTINELS + heads * p.num_rows + SENTINELS,), -7.0, device="cuda")
        linner = lbuf[SENTINELS:SENTINELS + heads * p.num_rows].view(heads, p.num_rows)
        got = ops.attention_bsr_bf16(a, q, k, v, mask=mask, out_bf16=out_bf16, out=view[:, :, :dv], lse=linner)
        assert got.data_ptr() == view.data_ptr()
        same_bits(view[:, :, :dv].contiguous(), out, f"{name} out inside a strided buffer")
        same_bits(linner, lse, f"{name} lse between sentinels")
        assert bool((view[:, :, dv:] == mark).all()), "a gap of the strided out was written"
        assert bool((buf[:SENTINELS] == mark).all()) and bool((buf[-SENTINELS:] == mark).all()), "a sentinel of out was written"
        assert bool((lbuf[:SENTINELS] == -7.0).all()) and bool((lbuf[-SENTINELS:] == -7.0).all()), "a sentinel of lse was written"


def test_deterministic_and_replays_from_a_graph():
    name = "edges16"
    a = device_bsr(name)
    q, k, v = (dbits(x) for x in ref.operands(name, 64, 64, 2))
    mask = dev(ref.mask_of(name, "causal"))
    out, lse = (x.clone() for x in ops.attention_bsr_bf16(a, q, k, v, mask=mask, out_bf16=True, return_lse=True))
    again = ops.attention_bsr_bf16(a, q, k, v, mask=mask, out_bf16=True, return_lse=True)
    same_bits(again[0], out, "second run")
    same_bits(again[1], lse, "second run, lse")
    out2, lse2 = torch.empty_like(out), torch.empty_like(lse)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture
        ops.attention_bsr_bf16(a, q, k, v, mask=mask, out_bf16=True, out=out2, lse=lse2)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                   # one launch: no parallel branches
        ops.attention_bsr_bf16(a, q, k, v, mask=mask, out_bf16=True, out=out2, lse=lse2)
    for _ in range(2):
        out2.zero_()
        lse2.zero_()
        g.replay()
        torch.cuda.synchronize()
        same_bits(out2, out, "graph replay")
        same_bits(lse2, lse, "graph replay, lse")


def test_every_tag_of_the_table_is_reached_by_its_shape():
    for tag, (bs, d, dv, with_mask, out_bf16) in ref.TAGS.items():
        name = f"ragged{bs}"
        a = device_bsr(name)
        q, k, v = (dbits(x[0]) for x in ref.operands(name, d, dv))
        out = ops.attention_bsr_bf16(a, q, k, v, mask=dev(ref.mask_of(name, "causal")) if with_mask else None, out_bf16=out_bf16)
        assert capi_attn.last_kernel() == tag, (capi_attn.last_kernel(), tag)
        assert capi.last_kernel() == tag                        # one libmispmm.so behind both bindings here
        assert not torch.isnan(out.view(torch.bfloat16).float() if out_bf16 else out).any()


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_fused_autograd_has_the_unfused_gradients_bit_for_bit(out_dtype):
    name, d, dv = "ragged16", 64, 64
    a = trainable(name)
    qh, kh, vh = (x[0] for x in ref.operands(name, d, dv))
    gh = full_mantissa(np.random.default_rng(77), (pattern(name).num_rows, dv))
    mask = dev(ref.mask_of(name, "causal"))
    grads = {}
    for fused in (False, True):
        q, k, v = (bf(x).requires_grad_(True) for x in (qh, kh, vh))
        out = autograd.block_sparse_attention(a, q, k, v, mask=mask, out_dtype=out_dtype, fused=fused)
        assert out.dtype == out_dtype and out.shape == (a.fwd.num_rows, dv)
        if fused:
            assert capi_attn.last_kernel().startswith("attn_bsr<"), capi_attn.last_kernel()
        out.backward(dev(gh).to(out_dtype))
        grads[fused] = (out.detach(), q.grad, k.grad, v.grad)
    for what, x, y in zip(("dq", "dk", "dv"), grads[True][1:], grads[False][1:]):
        assert x.dtype == torch.bfloat16
        same_bits(bits(x), bits(y), f"fused {what} against the three-launch path")
    want, tols, _, _ = reference(name, d, dv, "causal")
    err = np.abs(grads[True][0].float().cpu().numpy().astype(np.float64) - want)
    assert np.all(err <= tols[out_dtype == torch.bfloat16])


def test_fused_autograd_with_heads_and_frozen_inputs():
    name, d, dv, heads = "ragged32", 40, 72, 2
    a = trainable(name)
    qh, kh, vh = ref.operands(name, d, dv, heads)
    q, k, v = (bf(x).requires_grad_(True) for x in (qh, kh, vh))
    out = autograd.block_sparse_attention(a, q, k, v, fused=True)
    assert out.shape == (heads, a.fwd.num_rows, dv)
    g = torch.ones_like(out)
    out.backward(g)
    for h in range(heads):                                       # every head: the gradients of a 2-D unfused call
        q1, k1, v1 = (bf(x[h]).requires_grad_(True) for x in (qh, kh, vh))
        autograd.block_sparse_attention(a, q1, k1, v1).backward(g[h])
        for what, x, y in zip(("dq", "dk", "dv"), (q.grad[h], k.grad[h], v.grad[h]), (q1.grad, k1.grad, v1.grad)):
            same_bits(bits(x.contiguous()), bits(y), f"head {h} {what}")
    # all inputs frozen: no graph, no backward kernel; only v trainable: no SDDMM for dP, no softmax backward
    out = autograd.block_sparse_attention(a, bf(qh), bf(kh), bf(vh), fused=True)
    assert out.grad_fn is None and not out.requires_grad
    seen = []
    real = ops.softmax_bsr_bwd
    with torch.autograd.set_multithreading_enabled(False):
        try:
            ops.softmax_bsr_bwd = lambda *args, **kw: (seen.append("softmax_bwd"), real(*args, **kw))[1]
            v = bf(vh).requires_grad_(True)
            autograd.block_sparse_attention(a, bf(qh), bf(kh), v, fused=True).sum().backward()
            assert seen == [] and v.grad is not None and capi.last_kernel().startswith("bsr_mfma_bf16"), (seen, capi.last_kernel())
        finally:
            ops.softmax_bsr_bwd = real
    with pytest.raises(ValueError, match="multiples of 8 up to 128"):
        autograd.block_sparse_attention(a, bf(qh[0][:, :36]), bf(kh[0][:, :36]), bf(vh[0]), fused=True)


def test_activsg10k_two_heads_against_the_three_launch_chain():
    """16 x 16, 33100 blocks, block rows of up to 54 blocks.  bf16 out of both paths: every element within the sum of the two
    paths' tolerances (each the composed `out` tolerance, evaluated block by block)."""
    name, d, heads = "ACTIVSg10K", 64, 2
    a = device_bsr(name)
    qh, kh, vh = ref.operands(name, d, d, heads)
    q, k, v = (dbits(x) for x in (qh, kh, vh))
    out = ops.attention_bsr_bf16(a, q, k, v, out_bf16=True)
    assert capi_attn.last_kernel() == "attn_bsr<b16,bf16,nomask,D2,T4>", capi_attn.last_kernel()
    worst = 0.0
    for h in range(heads):
        s = ops.sddmm_bsr_bf16(a, q[h], k[h])
        p = ops.softmax_bsr(a, s, scale=d ** -0.5, out_bf16=True)
        chain = ops.spmm_bsr_bf16(a, p, v[h], out_bf16=True)
        tol = ref.out_tolerance(name, qh[h], kh[h], vh[h], d ** -0.5, None, True)
        err = np.abs(host(out[h]).astype(np.float64) - host(chain).astype(np.float64))
        worst = max(worst, float(np.max(err / (2 * tol))))
        assert np.all(err <= 2 * tol), f"head {h}: fused and three-launch out further apart than both tolerances"
    print(f"ACTIVSg10K fused against the chain: max |difference| / (2 tolerance) = {worst:.3g}")
