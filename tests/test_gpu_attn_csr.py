"""Fused attention on a CSR pattern (mispmm_attn_csr_f32 through ops.attention_csr and autograd.sparse_attention(fused=True)) on
the GPU: against float64 inside the composed tolerance of the four-launch chain and the header's lse bound, inside the derived
tight check of tests/_attn_csr_tight.py on every element, bit for bit on the tie rows, special values, the census of kernel
tags, refusals, out= / lse= buffers, determinism and graph replay, autograd, and against the chain itself.  The checks are the
functions tests/test_attn_csr_mutants_cpu.py runs the faulty restatements through."""
import dataclasses
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, capi_attn_csr, formats, ops  # noqa: E402

import _attn_csr_mutants as mut  # noqa: E402
import _attn_csr_ref as ref  # noqa: E402
import _attn_csr_tight as tight  # noqa: E402
from _bits import assert_same_bits  # noqa: E402
from _sddmm_ref import dense_of  # noqa: E402
from _softmax_ref import full_mantissa, matrix  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the shared operands are read-only


@functools.lru_cache(maxsize=None)
def device_csr(name):
    return ops.DeviceCSR.from_host(matrix(name), plan=False)


def device_operands(op):
    """The operands as the suite lays them out: q a view of [M, H, D] storage, k and v one head expanded over all (head stride
    0), a bias shared ([nnz]) or per head ([H, nnz]); one head: plain 2-D tensors."""
    heads = op["q"].shape[0]
    bias = None if op["bias"] is None else dev(op["bias"])
    if heads == 1:
        return dev(op["q"][0]), dev(op["k"][0]), dev(op["v"][0]), bias
    q = dev(np.ascontiguousarray(op["q"].transpose(1, 0, 2))).permute(1, 0, 2)
    k, v = (dev(op[n][0]).unsqueeze(0).expand(heads, -1, -1) for n in ("k", "v"))
    assert q.stride(0) == op["q"].shape[2] and k.stride(0) == 0 and v.stride(0) == 0
    return q, k, v, bias


def run(a, op):
    q, k, v, bias = device_operands(op)
    out, lse = ops.attention_csr(a, q, k, v, scale=op["scale"], bias=bias, return_lse=True)
    if op["q"].shape[0] == 1:
        out, lse = out.unsqueeze(0), lse.unsqueeze(0)
    return dict(out=out.cpu().numpy(), lse=lse.cpu().numpy())


@pytest.mark.parametrize("heads", ref.HEADS)
@pytest.mark.parametrize("bias", ref.BIASES)
@pytest.mark.parametrize("d,dv", ref.WIDTHS)
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_against_float64_inside_both_tolerances_and_the_tight_check(name, d, dv, bias, heads):
    case = ref.Case(name, d, dv, bias, heads)
    got = run(device_csr(name), ref.operands(case))
    assert capi_attn_csr.last_kernel() == ref.tag_of(d, dv, True)
    results = {what: check(got, case) for what, check in mut.CHECKS.items()}
    print(f"attn_csr {case.id}: worst |err| / tolerance: " + ", ".join(f"{what} {worst:.3g}" for what, (_, worst) in results.items()))
    for what, (ok, worst) in results.items():
        assert ok, f"{case.id}: {what} fails, worst {worst:.3g} x"
    empty = np.diff(matrix(name).row_ptrs.astype(np.int64)) == 0
    assert not got["out"][:, empty].view(np.uint32).any(), "an empty row must be +0"


@pytest.mark.parametrize("through_bias", [False, True])
@pytest.mark.parametrize("t", tight.TIES)
def test_tie_rows_bit_for_bit(t, through_bias):
    seen = tight.tie_coverage(t)
    assert seen["slots"] == set(range(8)) and seen["first_batch"] and seen["last_batch"] and seen["partial_last"], seen
    csr = tight.tie_pattern(t)[0]
    got = run(ops.DeviceCSR.from_host(csr, plan=False), tight.tie_operands(t, through_bias))
    ok, wrong = tight.tie_check(got, t, through_bias)
    assert ok, f"t={t} through_bias={through_bias}: {wrong} elements differ from the exact answers"


def _shifted_edges():
    """`edges` with every column moved up by one on K + 2 columns: no entry names column 0 or the last one."""
    csr = matrix("edges")
    return formats.CSR(csr.num_rows, csr.num_cols + 2, csr.row_ptrs, (csr.col_idxs + 1).astype(np.uint32), csr.data)


def test_special_values_are_torchs_and_stay_in_their_rows():
    csr = matrix("edges")
    a = device_csr("edges")
    case = ref.Case("edges", 8, 8, "finite", 1)
    op = dict(ref.operands(case))
    ptrs = csr.row_ptrs.astype(np.int64)
    lens = np.diff(ptrs)
    clean = run(a, op)
    rows = {"nan": int(np.argwhere(lens == 33)[0, 0]), "+inf": int(np.argwhere(lens == 17)[0, 0]), "all -inf": int(np.argwhere(lens == 9)[0, 0]),
            "both": int(np.argwhere(lens == 300)[0, 0])}
    bias = op["bias"].copy()
    bias[ptrs[rows["nan"]] + 20] = np.nan
    bias[ptrs[rows["+inf"]] + 3] = np.inf
    bias[ptrs[rows["all -inf"]]:ptrs[rows["all -inf"] + 1]] = -np.inf
    bias[ptrs[rows["both"]] + 5], bias[ptrs[rows["both"]] + 250] = np.inf, np.nan
    op["bias"] = bias
    got = run(a, op)
    hit = np.zeros(csr.num_rows, bool)
    hit[list(rows.values())] = True
    assert np.array_equal(np.isnan(got["out"][0]), np.broadcast_to(hit[:, None], got["out"][0].shape))
    assert_same_bits(got["out"][0][~hit], clean["out"][0][~hit], "rows without a special value")
    assert_same_bits(got["lse"][0][~hit], clean["lse"][0][~hit], "lse of rows without a special value")
    want = torch.logsumexp(torch.tensor([[np.nan, 0.0], [np.inf, 0.0], [-np.inf, -np.inf], [np.inf, np.nan]]), dim=1).numpy()
    for (what, r), w in zip(rows.items(), want):
        assert np.array_equal(got["lse"][0][r:r + 1], w[None], equal_nan=True), (what, got["lse"][0][r], w)
    # an empty row: +0 and -Inf; a row of one finite entry: that row of V (w = 1, l = 1)
    assert np.array_equal(np.isneginf(clean["lse"][0]), lens == 0)
    for r in np.argwhere(lens == 1).ravel():
        assert_same_bits(clean["out"][0][r], op["v"][0][csr.col_idxs[ptrs[r]]] + np.float32(0), f"row {r} of one entry")
    # a -Inf bias beside finite scores contributes exactly +0: the masked entries taken out of the pattern give the same rows
    masked = dict(ref.operands(ref.Case("edges", 8, 8, "masked", 1)))
    keep = np.isfinite(masked["bias"])
    kept_rows = np.repeat(np.arange(csr.num_rows), lens)[keep]
    sub = formats.CSR(csr.num_rows, csr.num_cols, np.concatenate([[0], np.cumsum(np.bincount(kept_rows, minlength=csr.num_rows))]).astype(np.uint32),
                      csr.col_idxs[keep], csr.data[keep])
    sub_op = dict(masked, bias=masked["bias"][keep])
    want_out, want_lse = ref.attention_f64(sub, sub_op["q"], sub_op["k"], sub_op["v"], sub_op["scale"], sub_op["bias"])
    got_masked = run(a, masked)
    tol = ref.out_tolerance(sub, sub_op["q"], sub_op["k"], sub_op["v"], sub_op["scale"], sub_op["bias"])
    assert np.all(np.abs(got_masked["out"] - want_out) <= tol)
    # a (row, column) pair stored twice counts twice; columns unsorted
    twice = matrix("unsorted")
    assert any(np.unique(twice.col_idxs[lo:hi]).size < hi - lo for lo, hi in zip(twice.row_ptrs[:-1].astype(int), twice.row_ptrs[1:].astype(int)))
    rng = np.random.default_rng(77)
    t_op = dict(q=full_mantissa(rng, (1, twice.num_rows, 12), np.float32), k=full_mantissa(rng, (1, twice.num_cols, 12), np.float32),
                v=full_mantissa(rng, (1, twice.num_cols, 20), np.float32), bias=None, scale=12 ** -0.5)
    got_twice = run(ops.DeviceCSR.from_host(twice, plan=False), t_op)
    want_out, _ = ref.attention_f64(twice, t_op["q"], t_op["k"], t_op["v"], t_op["scale"])
    err = np.abs(got_twice["out"] - want_out) / ref.out_tolerance(twice, t_op["q"], t_op["k"], t_op["v"], t_op["scale"])
    print(f"attn_csr unsorted (pairs stored twice): worst |err| / tolerance {float(err.max()):.3g}")
    assert np.all(err <= 1.0)


@pytest.mark.parametrize("d,dv", [(8, 8), (3, 5), (40, 72), (1, 129)])
def test_a_nan_in_rows_of_k_and_v_that_no_entry_names_reaches_no_output(d, dv):
    csr = _shifted_edges()
    a = ops.DeviceCSR.from_host(csr, plan=False)
    rng = np.random.default_rng(78)
    op = dict(q=full_mantissa(rng, (1, csr.num_rows, d), np.float32), k=full_mantissa(rng, (1, csr.num_cols, d), np.float32),
              v=full_mantissa(rng, (1, csr.num_cols, dv), np.float32), bias=None, scale=d ** -0.5)
    clean = run(a, op)
    assert not np.isnan(clean["out"]).any()
    k, v = op["k"].copy(), op["v"].copy()
    for x in (k, v):
        x[0, 0], x[0, -1] = np.nan, np.nan           # row 0 (where a wrapped offset would land) and a row nobody names
    got = run(a, dict(op, k=k, v=v))
    assert_same_bits(got["out"], clean["out"], "out with NaN rows planted")
    assert_same_bits(got["lse"], clean["lse"], "lse with NaN rows planted")


def test_every_tag_of_the_census_table_is_reached():
    a = device_csr("edges")
    csr = matrix("edges")
    rng = np.random.default_rng(79)
    seen = set()
    for tag, (d, dv, aligned) in ref.TAGS.items():
        pad = 0 if aligned else 1                    # an odd leading dimension: element lanes whatever the widths
        q, k, v = (dev(full_mantissa(rng, (n, w + pad), np.float32))[:, :w] for n, w in ((csr.num_rows, d), (csr.num_cols, d), (csr.num_cols, dv)))
        out = ops.attention_csr(a, q, k, v)
        assert capi_attn_csr.last_kernel() == tag == ref.tag_of(d, dv, aligned), (capi_attn_csr.last_kernel(), tag)
        assert capi.last_kernel() == tag             # the tag is left in the library every binding shares
        want = ref.attention_f64(csr, q.cpu().numpy()[None], k.cpu().numpy()[None], v.cpu().numpy()[None], d ** -0.5)[0]
        tol = ref.out_tolerance(csr, q.cpu().numpy()[None], k.cpu().numpy()[None], v.cpu().numpy()[None], d ** -0.5)
        assert np.all(np.abs(out.cpu().numpy()[None] - want) <= tol), tag
        seen.add(tag)
    # multiples of 4 on unaligned storage take the element lanes too
    q, k, v = (dev(full_mantissa(rng, (n, 9), np.float32))[:, 1:9] for n in (csr.num_rows, csr.num_cols, csr.num_cols))
    ops.attention_csr(a, q, k, v)
    assert capi_attn_csr.last_kernel() == "attn_csr<f32,G8,V1,C1>"
    assert seen == set(ref.TAGS)


def test_refusals_return_their_codes_and_launch_nothing():
    a = device_csr("edges")
    csr = matrix("edges")
    q, k, v = (torch.zeros((n, w), device="cuda") for n, w in ((csr.num_rows, 8), (csr.num_cols, 8), (csr.num_cols, 8)))
    sentinel = torch.full((csr.num_rows, 8), 7.0, device="cuda")
    ops.spmm_csr(a, torch.zeros((csr.num_cols, 8), device="cuda"))
    before = capi.last_kernel()
    lib = capi_attn_csr.lib()

    def call(**kw):
        args = dict(stream=None, H=1, M=csr.num_rows, K=csr.num_cols, nnz=csr.nnz, ptrs=a.row_ptrs.data_ptr(), cols=a.col_idxs.data_ptr(),
                    q=q.data_ptr(), qh=0, ldq=8, k=k.data_ptr(), kh=0, ldk=8, D=8, v=v.data_ptr(), vh=0, ldv=8, Dv=8, scale=1.0, bias=None, bh=0,
                    out=sentinel.data_ptr(), oh=0, ldo=8, lse=None)
        assert set(kw) <= set(args)
        args.update(kw)
        return lib.mispmm_attn_csr_f32(*args.values())

    for kw, code in ((dict(D=257, ldq=257, ldk=257), capi.ERR_UNSUPPORTED), (dict(Dv=300, ldv=300, ldo=300), capi.ERR_UNSUPPORTED),
                     (dict(D=0), capi.ERR_UNSUPPORTED), (dict(scale=float("nan")), capi.ERR_INVALID_ARG), (dict(q=None), capi.ERR_INVALID_ARG),
                     (dict(out=None), capi.ERR_INVALID_ARG), (dict(cols=None), capi.ERR_INVALID_ARG), (dict(ldk=7), capi.ERR_INVALID_ARG),
                     (dict(ldo=4), capi.ERR_INVALID_ARG), (dict(K=1 << 28, ldk=8), capi.ERR_UNSUPPORTED)):
        assert call(**kw) == code, kw
        assert "attn_csr_f32" in capi_attn_csr.last_error()
    assert call(H=0, q=None, out=None) == capi.OK and call(M=0, ptrs=None) == capi.OK
    torch.cuda.synchronize()
    assert capi.last_kernel() == before and bool((sentinel == 7.0).all()), "a refused call must launch nothing"
    with pytest.raises(ValueError, match="1 to 256"):
        ops.attention_csr(a, torch.zeros((csr.num_rows, 260), device="cuda"), torch.zeros((csr.num_cols, 260), device="cuda"), v)
    with pytest.raises(ValueError, match="float32"):
        ops.attention_csr(a, q.double(), k.double(), v.double())
    with pytest.raises(ValueError, match="bias"):
        ops.attention_csr(a, q, k, v, bias=torch.zeros(csr.nnz + 1, device="cuda"))


def test_out_and_lse_buffers_with_a_padded_row_stride_keep_their_sentinels():
    case = ref.Case("edges", 40, 72, "finite", 3)
    op = ref.operands(case)
    a = device_csr("edges")
    q, k, v, bias = device_operands(op)
    want, want_lse = ops.attention_csr(a, q, k, v, scale=op["scale"], bias=bias, return_lse=True)
    m = matrix("edges").num_rows
    store = torch.full((3, m, 80), -5.0, device="cuda")
    lse = torch.full((3, m), -5.0, device="cuda")
    got = ops.attention_csr(a, q, k, v, scale=op["scale"], bias=bias, out=store[:, :, :72], lse=lse)
    assert got.data_ptr() == store.data_ptr()
    assert_same_bits(store[:, :, :72].cpu().numpy(), want.cpu().numpy(), "out= with ldo = 80")
    assert bool((store[:, :, 72:] == -5.0).all()), "the bytes between rows must keep their sentinel"
    assert_same_bits(lse.cpu().numpy(), want_lse.cpu().numpy(), "lse=")
    # an odd row stride: element lanes, the same contract
    store = torch.full((3, m, 75), -5.0, device="cuda")
    ops.attention_csr(a, q, k, v, scale=op["scale"], bias=bias, out=store[:, :, :72])
    assert capi_attn_csr.last_kernel() == ref.tag_of(40, 72, False)
    assert bool((store[:, :, 72:] == -5.0).all())
    assert mut.out_composed(dict(out=store[:, :, :72].cpu().numpy()), case)[0]


def test_deterministic_and_replays_from_a_graph():
    case = ref.Case("edges", 40, 72, "masked", 3)
    op = ref.operands(case)
    a = device_csr("edges")
    q, k, v, bias = device_operands(op)
    out, lse = (x.clone() for x in ops.attention_csr(a, q, k, v, scale=op["scale"], bias=bias, return_lse=True))
    again = ops.attention_csr(a, q, k, v, scale=op["scale"], bias=bias, return_lse=True)
    assert_same_bits(again[0].cpu().numpy(), out.cpu().numpy(), "second run")
    assert_same_bits(again[1].cpu().numpy(), lse.cpu().numpy(), "second run, lse")
    out2, lse2 = torch.empty_like(out), torch.empty_like(lse)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up outside the capture
        ops.attention_csr(a, q, k, v, scale=op["scale"], bias=bias, out=out2, lse=lse2)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.attention_csr(a, q, k, v, scale=op["scale"], bias=bias, out=out2, lse=lse2)
    out2.zero_()
    lse2.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert_same_bits(out2.cpu().numpy(), out.cpu().numpy(), "graph replay")
    assert_same_bits(lse2.cpu().numpy(), lse.cpu().numpy(), "graph replay, lse")


# ---- autograd
def _dense_attention(csr, q, k, v, g, scale, bias):
    """float64 dense masked attention of one head with torch autograd: (out, dq, dk, dv)."""
    pat = formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, np.ones(csr.nnz))
    mask = torch.from_numpy(dense_of(pat) > 0)
    add = torch.zeros((csr.num_rows, csr.num_cols), dtype=torch.float64)
    if bias is not None:
        add = torch.from_numpy(dense_of(dataclasses.replace(pat, data=bias.astype(np.float64))))
    qt, kt, vt = (torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in (q, k, v))
    sc = ((qt * scale) @ kt.t() + add).masked_fill(~mask, float("-inf"))
    p = torch.softmax(sc, dim=1).masked_fill(~mask.any(dim=1, keepdim=True), 0.0)
    out = p @ vt
    out.backward(torch.from_numpy(g.astype(np.float64)))
    return out.detach().numpy(), qt.grad.numpy(), kt.grad.numpy(), vt.grad.numpy()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("heads", [1, 2])
def test_fused_sparse_attention_forward_and_gradients(heads, with_bias):
    from test_gpu_softmax import _attention_tolerances
    name, d = "long", 8
    csr = matrix(name)
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(46 + heads)
    q, k, v, g = (full_mantissa(rng, (heads, n, d), np.float32) for n in (csr.num_rows, csr.num_cols, csr.num_cols, csr.num_rows))
    bias = rng.uniform(-2, 2, (heads, csr.nnz)).astype(np.float32) if with_bias else None
    scale = d ** -0.5
    squeeze = (lambda x: x[0]) if heads == 1 else (lambda x: x)
    qd, kd, vd = (dev(squeeze(x)).requires_grad_(True) for x in (q, k, v))
    bd = None if bias is None else dev(squeeze(bias))
    with torch.autograd.set_multithreading_enabled(False):
        out = autograd.sparse_attention(a, qd, kd, vd, bias=bd, fused=True)
        assert capi.last_kernel().startswith("attn_csr<")
        out.backward(dev(squeeze(g)))
    got = [x.detach().cpu().numpy().reshape(heads, *x.shape[-2:]) for x in (out, qd.grad, kd.grad, vd.grad)]
    for h in range(heads):
        bh = None if bias is None else bias[h]
        # against float64 dense attention: out inside this file's tolerance, the gradients inside the chain's composed ones
        want = _dense_attention(csr, q[h], k[h], v[h], g[h], scale, bh)
        tol_out = ref.out_tolerance(csr, q[h:h + 1], k[h:h + 1], v[h:h + 1], scale, None if bh is None else bh[None])[0]
        err = np.abs(got[0][h] - want[0])
        print(f"fused sparse_attention H={heads} bias={with_bias} head {h} out: max |err| / tolerance = {float(np.max(err / tol_out)):.3g}")
        assert np.all(err <= tol_out)
        if bh is None:
            tols = _attention_tolerances(csr, q[h], k[h], v[h], g[h], scale, "fast")
            for what, gv, wv, tol in zip(("dq", "dk", "dv"), got[1:], want[1:], tols[1:]):
                assert np.all(np.abs(gv[h] - wv) <= tol), f"head {h}: {what} outside the composed tolerance"
        # the gradients are the unfused acc="fast" call's, bit for bit
        q1, k1, v1 = (dev(x[h]).requires_grad_(True) for x in (q, k, v))
        autograd.sparse_attention(a, q1, k1, v1, acc="fast", bias=None if bh is None else dev(bh)).backward(dev(g[h]))
        for what, gv, x in zip(("dq", "dk", "dv"), got[1:], (q1, k1, v1)):
            assert_same_bits(gv[h], x.grad.cpu().numpy(), f"head {h} {what} against the unfused fast path")
        if bh is not None:
            for gv, wv in zip(got[1:], want[1:]):
                assert np.allclose(gv[h], wv, rtol=1e-3, atol=1e-4)


def test_frozen_inputs_skip_their_kernels_and_old_calls_keep_their_bits():
    csr = matrix("long")
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(47)
    q, k, v = (full_mantissa(rng, (n, 8), np.float32) for n in (csr.num_rows, csr.num_cols, csr.num_cols))
    with torch.autograd.set_multithreading_enabled(False):
        # only v trainable: the backward ends with the transposed product, and no softmax backward ran
        qd, kd, vd = dev(q), dev(k), dev(v).requires_grad_(True)
        out = autograd.sparse_attention(a, qd, kd, vd, fused=True)
        seen = []
        real = ops.softmax_csr_bwd
        ops.softmax_csr_bwd = lambda *args, **kw: seen.append(1) or real(*args, **kw)
        try:
            out.sum().backward()
            assert not seen and vd.grad is not None and qd.grad is None and kd.grad is None
            qd, kd, vd = dev(q).requires_grad_(True), dev(k), dev(v)
            autograd.sparse_attention(a, qd, kd, vd, fused=True).sum().backward()
            assert seen == [1] and qd.grad is not None and kd.grad is None and vd.grad is None
        finally:
            ops.softmax_csr_bwd = real
        out = autograd.sparse_attention(a, dev(q), dev(k), dev(v), fused=True)
        assert out.grad_fn is None and not out.requires_grad
    # a call without the new keywords is the three kernels it always was: the bits of the chain spelled out by hand
    for acc in ("reference", "fast"):
        got = autograd.sparse_attention(a, dev(q), dev(k), dev(v), acc=acc)
        s = ops.sddmm_csr(a.fwd, dev(q) * 8 ** -0.5, dev(k), acc=acc)
        want = ops.spmm_csr(dataclasses.replace(a.fwd, data=ops.softmax_csr(a.fwd, s, acc=acc)), dev(v), acc=acc)
        assert_same_bits(got.cpu().numpy(), want.cpu().numpy(), f"sparse_attention without the new keywords, {acc}")
    with pytest.raises(ValueError, match="constant"):
        autograd.sparse_attention(a, dev(q), dev(k), dev(v), bias=torch.zeros(csr.nnz, device="cuda", requires_grad=True))
    with pytest.raises(ValueError, match="float32"):
        a64 = autograd.TrainableCSR.from_host(csr, dtype=torch.float64)
        autograd.sparse_attention(a64, dev(q).double(), dev(k).double(), dev(v).double(), fused=True)


def test_against_the_four_launch_chain_on_n4c6_b13():
    name, d, heads = "n4c6-b13", 64, 2
    csr = matrix(name)
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(48)
    q, k, v = (full_mantissa(rng, (heads, n, d), np.float32) for n in (csr.num_rows, csr.num_cols, csr.num_cols))
    scale = d ** -0.5
    fused = ops.attention_csr(a.fwd, dev(q), dev(k), dev(v)).cpu().numpy()
    tol = ref.out_tolerance(csr, q, k, v, scale)
    for h in range(heads):
        chain = autograd.sparse_attention(a, dev(q[h]), dev(k[h]), dev(v[h]), acc="fast").cpu().numpy()
        err = np.abs(fused[h].astype(np.float64) - chain.astype(np.float64))
        print(f"fused against the chain, {name} D=Dv=64 head {h}: max |diff| / (2 x tolerance) = {float(np.max(err / (2 * tol[h]))):.3g}")
        assert np.all(err <= 2 * tol[h]), "every element within the sum of both tolerances"
