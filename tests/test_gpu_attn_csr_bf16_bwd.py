"""The fused bf16 backward of attention on a CSR pattern (mispmm_attn_csr_bf16_bwd through attn_csr_bf16.attention_csr_bf16_bwd
and autograd.sparse_attention_bf16(fused_backward=True)) on the GPU.  bf16 widens to fp32 exactly, so every reference is one
the project owns, on the widened operands: float64 inside the derived tolerances, the derived tight check around the kernel's
own out and lse, the fp32 backward BIT FOR BIT on element lanes and, with a one-hot grad_out, on 16-byte lanes too, the fp32
gradients rounded once for the bf16 ones; the eight `need` subsets, special values, NaN rows nobody names, strides and every
kernel tag, determinism and graph replay, and autograd.  The checks are the functions tests/test_attn_csr_bf16_bwd_cpu.py runs
the faulty restatements through."""
import dataclasses
import functools
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, capi_attn_csr_bf16_bwd, capi_attn_csr_bwd, formats, ops, synth  # noqa: E402
from mispmm import attn_csr_bf16 as mod  # noqa: E402
from mispmm.attn_csr_bf16 import attention_csr_bf16, attention_csr_bf16_bwd  # noqa: E402

import _attn_csr_bf16_bwd_ref as bb  # noqa: E402
import _attn_csr_bf16_ref as fref  # noqa: E402
import _attn_csr_bwd_ref as bref  # noqa: E402
import _attn_csr_tight as tight  # noqa: E402
from _bits import SENTINEL_BITS, assert_same_bits  # noqa: E402
from _softmax_ref import full_mantissa, matrix  # noqa: E402

pytestmark = pytest.mark.gpu
PAD, GRADS = bb.PAD, bb.GRADS


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the shared operands are read-only


def bf16_values(rng, shape):
    return synth.bf16_round(full_mantissa(rng, shape, np.float32).reshape(-1)).reshape(shape).astype(np.float32)


@dataclasses.dataclass
class Pattern:
    csr: object
    fwd: object
    at: object
    perm: object


def upload(csr):
    t_csr, perm = bref.transpose(csr)
    return Pattern(csr, ops.DeviceCSR.from_host(csr, plan=False), ops.DeviceCSR.from_host(t_csr, plan=False), dev(perm.astype(np.int32)))


@functools.lru_cache(maxsize=None)
def pattern(name):
    return upload(bb.matrix(name))


def layout(op, pad=PAD):
    """(q, k, v, g, bias) on the device as the suite lays them out: int16 bf16 bits, every operand the [:, :width] corner of a
    buffer `pad` columns wider whose pad holds NaN bits; q and g views of [M, H, . + pad] storage; k and v one head expanded
    over all (head stride 0); one head: plain 2-D tensors."""
    heads = op["q"].shape[0]
    bias = None if op["bias"] is None else dev(op["bias"])
    corner = lambda x: dev(fref.padded_bits(x, pad))[..., :x.shape[-1]]                                    # noqa: E731
    if heads == 1:
        return corner(op["q"][0]), corner(op["k"][0]), corner(op["v"][0]), corner(op["g"][0]), bias
    q, g = (dev(np.ascontiguousarray(fref.padded_bits(op[n], pad).transpose(1, 0, 2))).permute(1, 0, 2)[:, :, :op[n].shape[2]] for n in ("q", "g"))
    k, v = (corner(op[n][0]).unsqueeze(0).expand(heads, -1, -1) for n in ("k", "v"))
    assert q.stride(0) == op["q"].shape[2] + pad and g.stride(0) == op["g"].shape[2] + pad and k.stride(0) == 0 and v.stride(0) == 0
    return q, k, v, g, bias


def padded(shape, bf16, pad=PAD):
    """A result buffer `pad` columns wider than `shape` [H, rows, width], filled with a sentinel."""
    if bf16:
        return torch.full(shape[:2] + (shape[2] + pad,), bb.GRAD_SENTINEL_BF16, dtype=torch.int16, device="cuda")
    buf = torch.empty(shape[:2] + (shape[2] + pad,), dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(SENTINEL_BITS)
    return buf


def corner_of(store, width, heads):
    return store[:, :, :width] if heads > 1 else store[0, :, :width]


def forward(pat, op, lay, pad=PAD):
    """The bf16 forward's fp32 out (the corner of a padded buffer) and lse, on the device."""
    q, k, v, _, bias = lay
    heads, dv = op["q"].shape[0], op["v"].shape[2]
    store = padded((heads, pat.csr.num_rows, dv), False, pad)
    return attention_csr_bf16(pat.fwd, q, k, v, scale=op["scale"], bias=bias, out=corner_of(store, dv, heads), return_lse=True)


def backward(pat, op, lay, out, lse, need=(True, True, True), grads_bf16=False, pad=PAD, delta=None):
    """dict(dq, dk, dv [H, ...] numpy: float32, or uint16 bits; None where not asked for; delta; tags).  Every gradient is the
    corner of a buffer `pad` columns wider whose pad holds a sentinel that must survive."""
    q, k, v, g, bias = lay
    heads, d, dv = op["q"].shape[0], op["q"].shape[2], op["v"].shape[2]
    m, kk = pat.csr.num_rows, pat.csr.num_cols
    stores = {n: padded((heads, rows, w), grads_bf16, pad) if wanted else None
              for n, rows, w, wanted in (("dq", m, d, need[0]), ("dk", kk, d, need[1]), ("dv", kk, dv, need[2]))}
    widths = dict(dq=d, dk=d, dv=dv)
    views = {n: None if s is None else corner_of(s, widths[n], heads) for n, s in stores.items()}
    if delta is None and (need[0] or need[1]):
        delta = torch.full(tuple(lse.shape), -5.0, device="cuda")
    got = attention_csr_bf16_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, scale=op["scale"], bias=bias, need=need, grads_bf16=grads_bf16,
                                 delta=delta, **views)
    res = dict(tag=capi_attn_csr_bf16_bwd.last_kernel(), delta=None if delta is None else delta.cpu().numpy().reshape(heads, m))
    sentinel = bb.GRAD_SENTINEL_BF16 if grads_bf16 else SENTINEL_BITS
    for n, x in zip(GRADS, got):
        if stores[n] is None:
            assert x is None
            res[n] = None
            continue
        assert x.data_ptr() == stores[n].data_ptr()
        raw = stores[n].cpu().numpy()
        bits = raw.view(np.uint16 if grads_bf16 else np.uint32)
        assert np.all(bits[:, :, widths[n]:] == sentinel), f"the pad columns of {n} must keep their sentinel"
        res[n] = np.ascontiguousarray(bits[:, :, :widths[n]] if grads_bf16 else raw[:, :, :widths[n]])
    return res


def same_bytes(got, want):
    """Bit for bit, NaN payloads included."""
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def run(pat, op, pad=PAD, **kw):
    """Forward, then backward with fp32 and with bf16 gradients: dict(out, lse, delta, dq, dk, dv, dq_bf16, ..., tag)."""
    lay = layout(op, pad)
    heads = op["q"].shape[0]
    out, lse = forward(pat, op, lay, pad)
    f32 = backward(pat, op, lay, out, lse, grads_bf16=False, pad=pad, **kw)
    b16 = backward(pat, op, lay, out, lse, grads_bf16=True, pad=pad, **kw)
    assert f32["tag"] == b16["tag"]
    res = dict(out=out.cpu().numpy().reshape(heads, pat.csr.num_rows, -1), lse=lse.cpu().numpy().reshape(heads, -1), delta=f32["delta"], tag=f32["tag"],
               lay=lay, dev_out=out, dev_lse=lse)
    for n in GRADS:
        res[n], res[n + "_bf16"] = f32[n], b16[n]
    return res


def run_f32(pat, op, out, lse, aligned, need=(True, True, True)):
    """ops.attention_csr_bwd on the widened operands (the float32 arrays of the case ARE the widened values) with the SAME out
    and lse; aligned False: an odd row stride, so the fp32 kernel runs on element lanes too."""
    heads = op["q"].shape[0]
    pad = 0 if aligned else 1
    corner = lambda x: dev(np.pad(x, [(0, 0)] * (x.ndim - 1) + [(0, pad)]))[..., :x.shape[-1]]       # noqa: E731
    bias = None if op["bias"] is None else dev(op["bias"])
    if heads == 1:
        q, k, v, g = (corner(op[n][0]) for n in ("q", "k", "v", "g"))
    else:
        q, g = corner(op["q"]), corner(op["g"])
        k, v = (corner(op[n][0]).unsqueeze(0).expand(heads, -1, -1) for n in ("k", "v"))
    o = corner(out.cpu().numpy())
    delta = torch.full(tuple(lse.shape), -5.0, device="cuda")
    stores = [None if not w else corner(np.zeros((heads, rows, width) if heads > 1 else (rows, width), np.float32))
              for w, rows, width in zip(need, (pat.csr.num_rows, pat.csr.num_cols, pat.csr.num_cols), (q.shape[-1], q.shape[-1], v.shape[-1]))]
    got = ops.attention_csr_bwd(pat.fwd, pat.at, pat.perm, q, k, v, o, lse, g, scale=op["scale"], bias=bias, need=need, delta=delta,
                                dq=stores[0], dk=stores[1], dv=stores[2])
    res = dict(tag=capi_attn_csr_bwd.last_kernel(), delta=delta.cpu().numpy().reshape(heads, -1))
    for n, x in zip(GRADS, got):
        res[n] = None if x is None else x.cpu().numpy().reshape(heads, *x.shape[-2:])
    return res


@functools.lru_cache(maxsize=None)
def results(case):
    got = run(pattern(case.name), bb.operands(case))
    return {n: x for n, x in got.items() if n not in ("lay", "dev_out", "dev_lse")}


CASE_PARAMS = [pytest.param(c, id=c.id) for c in bb.CASES]


def test_the_device_widening_is_the_hosts():
    op = bb.operands(bb.Case("ragged", 40, 72, "none", 3))
    for n in ("q", "k", "v", "g"):
        assert_same_bits(ops.bf16_to_f32(dev(fref.to_bits(op[n]))).cpu().numpy(), op[n], n)


@pytest.mark.parametrize("case", CASE_PARAMS)
def test_against_float64_inside_the_tolerances_the_tight_check_and_rounded_once(case):
    got = results(case)
    assert got["tag"] == bb.tags_of(case.d, case.dv, True)[-1], got["tag"]
    assert bb.coverage(case, got["out"], got["lse"]) == 1.0
    res = {what: check(got, case) for what, check in bb.CHECKS.items()}
    print(f"attn_csr_bf16_bwd {case.id} {got['tag']}: worst |err| / tolerance (dq, dk, dv): "
          + "; ".join(f"{what} " + ", ".join(f"{w:.3g}" for w in worst) for what, (_, worst) in res.items() if what != "rounded_once"))
    for what, (ok, worst) in res.items():
        assert ok, f"{case.id}: {what} fails, worst (dq, dk, dv) {worst}"
    csr = bb.matrix(case.name)
    empty_rows = np.diff(csr.row_ptrs.astype(np.int64)) == 0
    empty_cols = np.bincount(csr.col_idxs.astype(np.int64), minlength=csr.num_cols) == 0
    assert empty_rows.any() and empty_cols.any()
    for suffix, kind in (("", np.uint32), ("_bf16", np.uint16)):
        assert not got["dq" + suffix][:, empty_rows].view(kind).any(), "an empty row must give a +0 row of dq"
        assert not got["dk" + suffix][:, empty_cols].view(kind).any() and not got["dv" + suffix][:, empty_cols].view(kind).any(), "an empty column: +0"


V1_PARAMS = [p for p in CASE_PARAMS if bb.vec_of(p.values[0]) == 1]
V8_PARAMS = [p for p in CASE_PARAMS if bb.vec_of(p.values[0]) == 8]


@pytest.mark.parametrize("case", V1_PARAMS)
def test_on_element_lanes_every_output_has_the_fp32_kernels_bits(case):
    pat, op = pattern(case.name), bb.operands(case)
    lay = layout(op)
    out, lse = forward(pat, op, lay)
    got = backward(pat, op, lay, out, lse)
    f32 = run_f32(pat, op, out, lse, aligned=False)
    assert bb.fp32_tag(got["tag"]) == f32["tag"], (got["tag"], f32["tag"])        # the same G, V1 and C
    for n in GRADS + ("delta",):
        assert_same_bits(got[n], f32[n], f"{case.id} {n} against ops.attention_csr_bwd on the widened operands")


@pytest.mark.parametrize("case", V8_PARAMS)
def test_on_16_byte_lanes_a_one_hot_grad_out_gives_the_fp32_kernels_bits(case):
    pat, op = pattern(case.name), dict(bb.operands(case))
    op["g"] = bb.one_hot_g(case)
    lay = layout(op)
    out, lse = forward(pat, op, lay)
    got = backward(pat, op, lay, out, lse)
    f32 = run_f32(pat, op, out, lse, aligned=True)
    assert ",V8," in got["tag"] and ",V4," in f32["tag"]
    for n in GRADS + ("delta",):
        assert_same_bits(got[n], f32[n], f"{case.id} {n}: every sum is exact or in one order")


def test_the_eight_need_subsets_keep_their_bits_and_launch_what_they_say():
    case = bb.Case("edgesT", 40, 72, "masked", 3)
    op, pat = bb.operands(case), pattern("edgesT")
    full = results(case)
    lay = layout(op)
    out, lse = forward(pat, op, lay)
    m = pat.csr.num_rows
    ops.spmm_csr(pat.fwd, torch.zeros((pat.csr.num_cols, 8), device="cuda"))
    idle = capi.last_kernel()
    for bf16, need in itertools.product((False, True), itertools.product((False, True), repeat=3)):
        ops.spmm_csr(pat.fwd, torch.zeros((pat.csr.num_cols, 8), device="cuda"))
        delta = torch.full((3, m), -5.0, device="cuda")
        got = backward(pat, op, lay, out, lse, need=need, grads_bf16=bf16, delta=delta)
        for n, wanted in zip(GRADS, need):
            if wanted:
                assert same_bytes(got[n], full[n + ("_bf16" if bf16 else "")]), f"{n} with need={need}, bf16 gradients: {bf16}"
            else:
                assert got[n] is None
        tags = bb.tags_of(40, 72, True, need)
        assert capi.last_kernel() == (tags[-1] if tags else idle), (need, capi.last_kernel())
        row_ran = bool((delta != -5.0).any())
        assert row_ran == (need[0] or need[1]) and len(tags) == int(row_ran) + int(need[1] or need[2])


def test_special_values_a_masked_column_and_a_row_whose_lse_is_not_finite():
    case = bb.Case("edges", 8, 8, "finite", 3)
    op, csr, pat = dict(bb.operands(case)), bb.matrix("edges"), pattern("edges")
    ptrs, cols = csr.row_ptrs.astype(np.int64), csr.col_idxs.astype(np.int64)
    lens = np.diff(ptrs)
    rows = np.repeat(np.arange(csr.num_rows), lens)
    counts = np.bincount(cols, minlength=csr.num_cols)
    ok = [c for c in np.argsort(-counts)[:200] if counts[c] >= 2 and all(lens[r] > (cols[ptrs[r]:ptrs[r + 1]] == c).sum() for r in rows[cols == c])][:3]
    assert len(ok) == 3
    bias = op["bias"].copy()
    bias[:, np.isin(cols, ok)] = -np.inf
    op["bias"] = bias
    got = run(pat, op)
    assert np.isfinite(got["lse"][:, lens > 0]).all()
    for suffix, kind in (("", np.uint32), ("_bf16", np.uint16)):
        assert not got["dk" + suffix][:, ok].view(kind).any() and not got["dv" + suffix][:, ok].view(kind).any(), "a masked column must be +0 bit for bit"
    args = (csr, op["q"], op["k"], op["v"], op["g"], op["scale"], bias)
    for n, w, t in zip(GRADS, bref.backward_f64(*args), bref.bwd_tolerances(*args)):
        assert np.all(np.abs(got[n] - w) <= t), n
    # a row whose lse is not finite: NaN in its dQ row and in the dK and dV rows of its keys, and nowhere else
    for bad in (np.inf, np.nan, -np.inf):
        row = int(np.flatnonzero(lens == 9)[0])
        lse = got["dev_lse"].clone()
        lse[1, row] = bad
        hurt = backward(pat, op, got["lay"], got["dev_out"], lse)
        keys = np.zeros(csr.num_cols, bool)
        keys[cols[ptrs[row]:ptrs[row + 1]]] = True
        assert np.isnan(hurt["dq"][1, row]).all() and np.isnan(hurt["dk"][1, keys]).all() and np.isnan(hurt["dv"][1, keys]).all(), bad
        for n, mask in (("dq", np.arange(csr.num_rows) == row), ("dk", keys), ("dv", keys)):
            clean = hurt[n].copy()
            clean[1, mask] = got[n][1, mask]
            assert_same_bits(clean, got[n], f"{n}: the other rows with lse = {bad} in one row")


def _shifted_edges():
    """`edges` with every column moved up by one on K + 2 columns: no entry names column 0 or the last one; its first and last
    rows are empty, so no entry lies in row 0 or in the last row either."""
    csr = matrix("edges")
    assert csr.row_ptrs[1] == 0 and csr.row_ptrs[-1] == csr.row_ptrs[-2]
    return formats.CSR(csr.num_rows, csr.num_cols + 2, csr.row_ptrs, (csr.col_idxs + 1).astype(np.uint32), csr.data)


@pytest.mark.parametrize("d,dv", [(8, 8), (3, 5), (40, 72), (1, 129)])
def test_nan_bits_in_rows_that_no_entry_names_reach_no_output(d, dv):
    csr = _shifted_edges()
    pat = upload(csr)
    rng = np.random.default_rng(278)
    op = dict(q=bf16_values(rng, (1, csr.num_rows, d)), k=bf16_values(rng, (1, csr.num_cols, d)), v=bf16_values(rng, (1, csr.num_cols, dv)),
              g=bf16_values(rng, (1, csr.num_rows, dv)), bias=None, scale=d ** -0.5)
    clean = run(pat, op)
    assert not any(np.isnan(clean[n]).any() for n in GRADS)
    q, k, v, g, _ = (x.clone() if x is not None else None for x in clean["lay"])
    for x in (q, k, v, g):
        x[0], x[-1] = fref.NAN_BITS, fref.NAN_BITS          # row 0 (where a wrapped offset would land) and a row nobody names
    for bf16 in (False, True):
        got = backward(pat, op, (q, k, v, g, None), clean["dev_out"], clean["dev_lse"], grads_bf16=bf16)
        for n in GRADS:
            assert same_bytes(got[n], clean[n + ("_bf16" if bf16 else "")]), f"{n} with NaN rows planted in q, k, v and grad_out"


def test_odd_strides_and_offsets_run_on_element_lanes_with_the_same_values():
    case = bb.Case("edgesT", 40, 72, "finite", 3)
    op, pat = bb.operands(case), pattern("edgesT")
    for pad in (3, 1):
        got = run(pat, op, pad=pad)
        assert got["tag"] == bb.tags_of(40, 72, False)[-1], got["tag"]
        for what, check in bb.CHECKS.items():
            assert check(got, case)[0], (what, pad)
    # a base 2 bytes off a 16-byte boundary with every stride a multiple of 8: element lanes again
    lay = layout(op)
    out, lse = forward(pat, op, lay)
    q = lay[0]
    shifted = torch.full((q.shape[1], 3 * (40 + PAD) + 8), fref.NAN_BITS, dtype=torch.int16, device="cuda")[:, 1:1 + 3 * (40 + PAD)]
    shifted = shifted.view(q.shape[1], 3, 40 + PAD).permute(1, 0, 2)[:, :, :40]
    shifted.copy_(q)
    assert shifted.data_ptr() % 16 == 2 and shifted.stride() == (48, 3 * 48 + 8, 1)
    got = backward(pat, op, (shifted,) + tuple(lay[1:]), out, lse)
    assert got["tag"] == bb.tags_of(40, 72, False)[-1]
    v8 = results(case)
    assert v8["tag"] == bb.tags_of(40, 72, True)[-1]
    want, tols = bb.expected(case)
    for n, w, t in zip(GRADS, want, tols):
        assert np.all(np.abs(got[n] - w) <= t) and np.all(np.abs(got[n].astype(np.float64) - v8[n]) <= 2 * t), n


def test_every_tag_of_the_census_table_is_reached():
    pat = pattern("edges")
    csr = pat.csr
    rng = np.random.default_rng(279)
    seen = set()
    for tag, (d, dv, aligned) in fref.TAGS.items():
        op = dict(q=bf16_values(rng, (1, csr.num_rows, d)), k=bf16_values(rng, (1, csr.num_cols, d)), v=bf16_values(rng, (1, csr.num_cols, dv)),
                  g=bf16_values(rng, (1, csr.num_rows, dv)), bias=None, scale=d ** -0.5)
        pad = PAD if aligned else 1                    # an odd leading dimension: element lanes whatever the widths
        lay = layout(op, pad)
        out, lse = forward(pat, op, lay, pad)
        only_q = backward(pat, op, lay, out, lse, need=(True, False, False), pad=pad)
        row_tag = only_q["tag"]
        got = backward(pat, op, lay, out, lse, pad=pad)
        assert [row_tag, got["tag"]] == bb.tags_of(d, dv, aligned) and capi.last_kernel() == got["tag"], (row_tag, got["tag"], tag)
        assert_same_bits(only_q["dq"], got["dq"], f"{row_tag}: dq alone")
        args = (csr, op["q"], op["k"], op["v"], op["g"], op["scale"])
        for n, w, t in zip(GRADS, bref.backward_f64(*args), bref.bwd_tolerances(*args)):
            assert np.all(np.abs(got[n] - w) <= t), (got["tag"], n)
        seen |= {row_tag, got["tag"]}
    assert seen == set(bb.TAGS) and len(seen) == 18


def test_deterministic_replays_from_a_graph_and_a_head_does_not_depend_on_h():
    case = bb.Case("edgesT", 40, 72, "masked", 3)
    op, pat = bb.operands(case), pattern("edgesT")
    base = results(case)
    lay = layout(op)
    q, k, v, g, bias = lay
    out, lse = forward(pat, op, lay)
    for bf16 in (False, True):
        suffix, dtype = ("_bf16", torch.int16) if bf16 else ("", torch.float32)
        again = backward(pat, op, lay, out, lse, grads_bf16=bf16)
        for n in GRADS:
            assert same_bytes(again[n], base[n + suffix]), f"second run, {n}"
        m, kk = pat.csr.num_rows, pat.csr.num_cols
        bufs = dict(dq=torch.empty((3, m, 40), dtype=dtype, device="cuda"), dk=torch.empty((3, kk, 40), dtype=dtype, device="cuda"),
                    dv=torch.empty((3, kk, 72), dtype=dtype, device="cuda"), delta=torch.empty_like(lse))
        call = lambda: attention_csr_bf16_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, scale=op["scale"], bias=bias, grads_bf16=bf16, **bufs)  # noqa: E731
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                   # warm-up outside the capture
            call()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        for x in bufs.values():
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for n in GRADS:
            assert same_bytes(bufs[n].cpu().numpy().view(base[n + suffix].dtype), base[n + suffix]), f"graph replay, {n}"
        assert_same_bits(bufs["delta"].cpu().numpy(), base["delta"], "graph replay, delta")
    # the result of a head does not depend on H: head 1 alone, head 1 among 2 (per-head bias rows of the finite case)
    fin = bb.Case("edgesT", 40, 72, "finite", 3)
    fop, fbase = bb.operands(fin), results(fin)
    for pick in ([1], [1, 2], [2, 0]):
        sub = dict(fop, q=fop["q"][pick], g=fop["g"][pick], bias=fop["bias"][pick] if len(pick) > 1 else fop["bias"][pick[0]])
        got = run(pat, sub)
        for n in GRADS:
            assert_same_bits(got[n], fbase[n][pick], f"heads {pick} of 3, {n}")
            assert np.array_equal(got[n + "_bf16"], fbase[n + "_bf16"][pick])


def test_refusals_launch_nothing():
    pat = pattern("edges")
    m, kk = pat.csr.num_rows, pat.csr.num_cols
    bits = lambda *shape: torch.zeros(shape, dtype=torch.int16, device="cuda")                  # noqa: E731
    q, k, v, g = bits(m, 8), bits(kk, 8), bits(kk, 8), bits(m, 8)
    out, lse = torch.zeros((m, 8), device="cuda"), torch.zeros(m, device="cuda")
    sent = torch.full((m, 8), 7, dtype=torch.int16, device="cuda")
    ops.spmm_csr(pat.fwd, torch.zeros((kk, 8), device="cuda"))
    before = capi.last_kernel()
    with pytest.raises(capi.MispmmError, match="scale must be finite"):
        attention_csr_bf16_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, scale=float("inf"), dq=sent)
    with pytest.raises(capi.MispmmError, match="overlaps an input"):
        attention_csr_bf16_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, dq=q)
    with pytest.raises(ValueError, match="grad_out must be an int16"):
        attention_csr_bf16_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g.float(), dq=sent)
    with pytest.raises(ValueError, match="dq must be a float32"):
        attention_csr_bf16_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, dq=sent, grads_bf16=False)
    torch.cuda.synchronize()
    assert capi.last_kernel() == before and bool((sent == 7).all()), "a refused call must launch nothing"


# ---- autograd
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("heads", [1, 2])
def test_fused_backward_through_autograd(heads, with_bias):
    name, d = "long", 8
    csr = matrix(name)
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(346 + heads)
    q, k, v, g = (bf16_values(rng, (heads, n, d)) for n in (csr.num_rows, csr.num_cols, csr.num_cols, csr.num_rows))
    bias = rng.uniform(-2, 2, (heads, csr.nnz)).astype(np.float32) if with_bias else None
    scale = d ** -0.5
    squeeze = (lambda x: x[0]) if heads == 1 else (lambda x: x)
    bd = None if bias is None else dev(squeeze(bias))
    bits = lambda t: t.detach().view(torch.int16)                                  # noqa: E731

    def grads(**kw):
        qd, kd, vd = (dev(squeeze(x)).to(torch.bfloat16).requires_grad_(True) for x in (q, k, v))
        with torch.autograd.set_multithreading_enabled(False):
            out = autograd.sparse_attention_bf16(a, qd, kd, vd, bias=bd, **kw)
            assert out.dtype == torch.bfloat16
            out.backward(dev(squeeze(g)).to(torch.bfloat16))
            tag = capi.last_kernel()
        return (qd, kd, vd), tag, out

    (qd, kd, vd), tag, out = grads(fused_backward=True)
    assert tag == "attn_csr_bf16_bwd_col<G8,V8,C1>", tag
    # the forward is what it is without the keyword; the gradients are one call made by hand, bit for bit
    out32, lse = attention_csr_bf16(a.fwd, bits(qd), bits(kd), bits(vd), scale=scale, bias=bd, return_lse=True)
    assert np.array_equal(bits(out).cpu().numpy().view(np.uint16), fref.bf16_bits(out32.cpu().numpy()))
    hand = attention_csr_bf16_bwd(a.fwd, a.tpattern, a.perm32(), bits(qd), bits(kd), bits(vd), out32, lse, dev(fref.to_bits(squeeze(g))), scale=scale, bias=bd)
    want = bref.backward_f64(csr, q, k, v, g, scale, bias)
    tols = bref.bwd_tolerances(csr, q, k, v, g, scale, bias)
    for n, t, h, w, tol in zip(GRADS, (qd, kd, vd), hand, want, tols):
        assert t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape and h.dtype == torch.int16
        assert np.array_equal(bits(t.grad).cpu().numpy(), h.cpu().numpy()), f"{n} against attention_csr_bf16_bwd called by hand"
        ok, worst = tight._worst(fref.widen(bits(t.grad).cpu().numpy().view(np.uint16)).reshape(heads, *t.shape[-2:]), w, fref.with_one_bf16_rounding(w, tol))
        print(f"sparse_attention_bf16(fused_backward=True) H={heads} bias={with_bias} {n}: max |err| / tolerance = {worst:.3g}")
        assert ok, n
    # without the keyword the backward still is its old composition, and the new library is not called
    ops.spmm_csr(a.fwd, torch.zeros((csr.num_cols, 8), device="cuda"))
    (q0, k0, v0), old_tag, _ = grads()
    assert capi_attn_csr_bwd.last_kernel().startswith("attn_csr_bwd_col<") and not old_tag.startswith("attn_csr_bf16_bwd"), old_tag
    qf, kf, vf = (ops.bf16_to_f32(bits(t)) for t in (q0, k0, v0))
    comp = ops.attention_csr_bwd(a.fwd, a.tpattern, a.perm32(), qf, kf, vf, out32, lse, ops.bf16_to_f32(dev(fref.to_bits(squeeze(g)))), scale=scale, bias=bd)
    for n, t, h in zip(GRADS, (q0, k0, v0), comp):
        assert np.array_equal(bits(t.grad).cpu().numpy(), ops.f32_to_bf16(h).cpu().numpy()), f"{n}: the default backward against its composition"


def test_frozen_inputs_get_none_and_their_pass_is_skipped():
    csr = matrix("long")
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(347)
    q, k, v = (bf16_values(rng, (n, 8)) for n in (csr.num_rows, csr.num_cols, csr.num_cols))
    seen, old = [], []
    real, real_old = mod.attention_csr_bf16_bwd, ops.attention_csr_bwd
    mod.attention_csr_bf16_bwd = lambda *args, **kw: seen.append((tuple(kw["need"]), kw["grads_bf16"])) or real(*args, **kw)
    ops.attention_csr_bwd = lambda *args, **kw: old.append(1) or real_old(*args, **kw)
    try:
        with torch.autograd.set_multithreading_enabled(False):
            for trainable in ((False, False, True), (True, False, False), (False, True, False), (True, True, True)):
                qd, kd, vd = (dev(x).to(torch.bfloat16).requires_grad_(t) for x, t in zip((q, k, v), trainable))
                autograd.sparse_attention_bf16(a, qd, kd, vd, fused_backward=True).sum().backward()                  # an expanded grad_out
                assert seen[-1] == (trainable, True) and [x.grad is not None for x in (qd, kd, vd)] == list(trainable)
                # dq alone ends with the row pass: the column pass on A^T's pattern was not launched
                assert capi.last_kernel().startswith("attn_csr_bf16_bwd_row<" if trainable == (True, False, False) else "attn_csr_bf16_bwd_col<")
            count = len(seen)
            out = autograd.sparse_attention_bf16(a, *(dev(x).to(torch.bfloat16) for x in (q, k, v)), fused_backward=True)
            assert out.grad_fn is None and not out.requires_grad and out.dtype == torch.bfloat16 and len(seen) == count and not old
    finally:
        mod.attention_csr_bf16_bwd, ops.attention_csr_bwd = real, real_old
    qb, kb, vb = (dev(x).to(torch.bfloat16) for x in (q, k, v))
    with pytest.raises(ValueError, match="grad_out would be float32"):
        autograd.sparse_attention_bf16(a, qb, kb, vb, fused_backward=True, out_dtype=torch.float32)
