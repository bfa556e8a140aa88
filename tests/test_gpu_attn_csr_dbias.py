"""The bias gradient of the fused CSR attention (mispmm_attn_csr_dbias_f32 / _bf16 through mispmm.attn_csr_dbias and the
bias_grad keyword of autograd.sparse_attention / sparse_attention_bf16) on the GPU: dBias against float64 inside the derived
tolerance with out and lse from the matching fused forward; dq rebuilt from dBias against the dq of the backward that already
exists, bit for bit; nothing written but the H * nnz entries; special values; strides; independence of H and of the run; and
autograd on its five paths.  The checks are the functions tests/test_attn_csr_dbias_cpu.py runs the faulty restatements through."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import attn_csr_bf16, attn_csr_dbias, autograd, capi, capi_attn_csr_bf16_bwd, capi_attn_csr_bwd, capi_attn_csr_dbias, formats, ops  # noqa: E402

import _attn_csr_bf16_ref as fref  # noqa: E402
import _attn_csr_bwd_ref as bref  # noqa: E402
import _attn_csr_dbias_ref as db  # noqa: E402
from _bits import assert_same_bits  # noqa: E402
from _softmax_ref import full_mantissa, matrix  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64                                   # guard words before and after dBias


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the shared operands are read-only


class Pattern:
    def __init__(self, csr):
        t_csr, perm = bref.transpose(csr)
        self.csr, self.fwd, self.at = csr, ops.DeviceCSR.from_host(csr, plan=False), ops.DeviceCSR.from_host(t_csr, plan=False)
        self.perm = dev(perm.astype(np.int32))


@functools.lru_cache(maxsize=None)
def pattern(name):
    return Pattern(db.matrix(name))


def _put(x, elem):
    return dev(x if elem == "f32" else fref.to_bits(x))


def device_operands(op, elem, layout="suite"):
    """(q, k, v, g, bias) on the device.  layout "suite": q and g views of [M, H, .] storage, k and v one head expanded over all
    (head stride 0), one head: plain 2-D tensors; "contiguous": [H, ., .] contiguous with k and v materialised per head;
    "padded": rows 8 columns apart from the next."""
    heads = op["q"].shape[0]
    bias = None if op["bias"] is None else dev(op["bias"])
    if heads == 1 and layout == "suite":
        return (*(_put(op[n][0], elem) for n in ("q", "k", "v", "g")), bias)
    full = {n: np.broadcast_to(op[n], (heads,) + op[n].shape[1:]) for n in ("q", "k", "v", "g")}
    if layout == "contiguous":
        return (*(_put(full[n], elem) for n in ("q", "k", "v", "g")), bias)
    if layout == "padded":
        wide = {n: np.concatenate([full[n], np.full(full[n].shape[:2] + (8,), 3.0, np.float32)], axis=2) for n in full}
        return (*(_put(wide[n], elem)[:, :, :full[n].shape[2]] for n in ("q", "k", "v", "g")), bias)
    q, g = (_put(np.ascontiguousarray(op[n].transpose(1, 0, 2)), elem).permute(1, 0, 2) for n in ("q", "g"))
    k, v = (_put(op[n][0], elem).unsqueeze(0).expand(heads, -1, -1) for n in ("k", "v"))
    assert q.stride(0) == op["q"].shape[2] and g.stride(0) == op["g"].shape[2] and k.stride(0) == 0 and v.stride(0) == 0
    return q, k, v, g, bias


def forward(pat, elem, q, k, v, scale, bias):
    """(out, lse) in fp32 from the matching fused forward."""
    if elem == "f32":
        return ops.attention_csr(pat.fwd, q, k, v, scale=scale, bias=bias, return_lse=True)
    return attn_csr_bf16.attention_csr_bf16(pat.fwd, q, k, v, scale=scale, bias=bias, return_lse=True)


def dbias_call(pat, elem, *args, **kw):
    fn = attn_csr_dbias.attention_csr_dbias if elem == "f32" else attn_csr_dbias.attention_csr_dbias_bf16
    return fn(pat.fwd, *args, **kw)


def guarded(heads, nnz, stride):
    """(store, view [H, nnz] at head stride `stride`): GUARD words, the heads, GUARD words, all holding the sentinel NaN."""
    store = dev(np.full(2 * GUARD + heads * stride, db.SENTINEL, np.uint32).view(np.float32))
    return store, store[GUARD:GUARD + heads * stride].view(heads, stride)[:, :nnz]


def run(case, elem, layout="suite", with_dq=False, stride=None, op=None, pat=None):
    """dict(dbias [H, stride] with its guard words checked, lse, out, tag[, dq, row_tag]) as numpy arrays."""
    pat, op = pat or pattern(case.name), op or db.operands(case, elem)
    heads, nnz = op["q"].shape[0], pat.csr.nnz
    q, k, v, g, bias = device_operands(op, elem, layout)
    out, lse = forward(pat, elem, q, k, v, op["scale"], bias)
    stride = nnz if stride is None else stride
    store, view = guarded(heads, nnz, stride)
    batched = q.dim() == 3
    got = dbias_call(pat, elem, q, k, v, out, lse, g, op["scale"], bias, dbias=view if batched else view[0])
    assert got.data_ptr() == view.data_ptr()
    res = dict(tag=capi_attn_csr_dbias.last_kernel())
    assert capi.last_kernel() == res["tag"]
    words = store.cpu().numpy().view(np.uint32)
    assert np.all(words[:GUARD] == db.SENTINEL) and np.all(words[GUARD + heads * stride:] == db.SENTINEL), "a guard word before or after dBias has changed"
    res["dbias"] = words[GUARD:GUARD + heads * stride].view(np.float32).reshape(heads, stride)
    res["lse"], res["out"] = lse.cpu().numpy().reshape(heads, -1), out.cpu().numpy().reshape(heads, -1, op["v"].shape[2])
    if with_dq:
        if elem == "f32":
            dq = ops.attention_csr_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, scale=op["scale"], bias=bias, need=(True, False, False))[0]
            res["row_tag"] = capi_attn_csr_bwd.last_kernel()
        else:
            dq = attn_csr_bf16.attention_csr_bf16_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, scale=op["scale"], bias=bias,
                                                      need=(True, False, False), grads_bf16=False)[0]
            res["row_tag"] = capi_attn_csr_bf16_bwd.last_kernel()
        assert dq.is_contiguous() and dq.data_ptr() % 16 == 0
        res["dq"] = dq.cpu().numpy().reshape(heads, -1, op["q"].shape[2])
    return res


@pytest.mark.parametrize("elem", db.ELEMS)
@pytest.mark.parametrize("case", db.CASES, ids=lambda c: c.id)
def test_inside_the_tolerance_and_the_backwards_dq_is_rebuilt_bit_for_bit(case, elem):
    got = run(case, elem, with_dq=True)
    assert got["tag"] == db.tag_of(elem, case.d, case.dv, True)
    assert got["row_tag"].split("G")[1] == got["tag"].split("G")[1], "the same (G, V, C) as the backward's row pass"
    csr = db.matrix(case.name)
    lens = np.diff(csr.row_ptrs.astype(np.int64))
    assert np.isfinite(got["lse"][:, lens > 0]).all(), "no row is left out of either check"
    results = {what: check(got, case, elem) for what, check in db.CHECKS.items()}
    print(f"attn_csr_dbias {elem} {case.id} {got['tag']}: worst |err| / tolerance {results['inside_tolerance'][1]:.3g}; "
          f"entries not written {results['all_written'][1]}; dq elements that differ {results['rebuilds_dq'][1]}")
    for what, (ok, worst) in results.items():
        assert ok, f"{elem} {case.id}: {what} fails ({worst})"
    if case.bias == "masked":
        masked = np.isneginf(np.broadcast_to(db.operands(case, elem)["bias"], got["dbias"].shape))
        assert masked.any() and np.all(got["dbias"][masked] == 0), "a masked entry is a zero"


@pytest.mark.parametrize("elem", db.ELEMS)
@pytest.mark.parametrize("d,dv", [(40, 72), (3, 5)])
def test_nothing_is_written_but_the_entries_also_between_heads(d, dv, elem):
    case = db.Case("edges", d, dv, "finite", 3)
    nnz = db.matrix("edges").nnz
    plain = run(case, elem)
    for pad in (1, 37):
        got = run(case, elem, stride=nnz + pad)              # run() itself holds the guards before and after
        ok, count = db.all_written(got, case, elem)
        assert ok, f"{count} entries left unwritten or guard words between the heads changed (head stride nnz + {pad})"
        assert_same_bits(got["dbias"][:, :nnz], plain["dbias"], f"head stride nnz + {pad}")


def _shifted_edges():
    """`edges` with every column moved up by one on K + 2 columns: no entry names column 0 or the last one; its first and last
    rows are empty, so no entry lies in row 0 or in the last row either."""
    csr = matrix("edges")
    assert csr.row_ptrs[1] == 0 and csr.row_ptrs[-1] == csr.row_ptrs[-2]
    return formats.CSR(csr.num_rows, csr.num_cols + 2, csr.row_ptrs, (csr.col_idxs + 1).astype(np.uint32), csr.data)


@pytest.mark.parametrize("elem", db.ELEMS)
@pytest.mark.parametrize("d,dv", [(8, 8), (3, 5), (40, 72), (1, 129)])
def test_a_nan_in_rows_that_no_entry_names_reaches_nothing(d, dv, elem):
    csr = _shifted_edges()
    pat = Pattern(csr)
    rng = np.random.default_rng(181)
    op = dict(q=full_mantissa(rng, (1, csr.num_rows, d), np.float32), k=full_mantissa(rng, (1, csr.num_cols, d), np.float32),
              v=full_mantissa(rng, (1, csr.num_cols, dv), np.float32), g=full_mantissa(rng, (1, csr.num_rows, dv), np.float32), bias=None, scale=d ** -0.5)
    if elem == "bf16":
        op.update({n: db.synth.bf16_round(op[n].reshape(-1)).reshape(op[n].shape) for n in ("q", "k", "v", "g")})
    case = db.Case("edges", d, dv, "none", 1)
    clean = run(case, elem, op=op, pat=pat)
    assert not np.isnan(clean["dbias"]).any()
    planted = {n: op[n].copy() for n in ("q", "k", "v", "g")}
    for x in planted.values():
        x[0, 0], x[0, -1] = np.nan, np.nan           # row 0 (where a wrapped offset would land) and a row nobody names
    got = run(case, elem, op=dict(op, **planted), pat=pat)
    assert_same_bits(got["dbias"], clean["dbias"], "dBias with NaN rows planted in q, k, v and grad_out")


@pytest.mark.parametrize("elem", db.ELEMS)
def test_a_row_made_non_finite_is_nan_in_exactly_its_own_entries(elem):
    case = db.Case("edges", 8, 64, "finite", 3)
    op, csr = dict(db.operands(case, elem)), db.matrix("edges")
    ptrs = csr.row_ptrs.astype(np.int64)
    row = int(np.flatnonzero(np.diff(ptrs) == 17)[0])
    bias = op["bias"].copy()
    bias[1, ptrs[row] + 9] = np.inf                  # head 1 alone, an entry of the row's second batch
    op["bias"] = bias
    clean, got = run(case, elem), run(case, elem, op=op)
    finite = np.repeat((np.diff(ptrs) > 0)[None, :], 3, axis=0)
    finite[1, row] = False
    assert np.isposinf(got["lse"][1, row]) and np.array_equal(np.isfinite(got["lse"]), finite), "the row's lse is +Inf in head 1 and nowhere else"
    hit = np.zeros(got["dbias"].shape, dtype=bool)
    hit[1, ptrs[row]:ptrs[row + 1]] = True
    assert np.isnan(got["dbias"][hit]).all() and not np.isnan(got["dbias"][~hit]).any()
    assert np.array_equal(got["dbias"].view(np.uint32)[~hit], clean["dbias"].view(np.uint32)[~hit]), "every other entry keeps its bits"


@pytest.mark.parametrize("elem", db.ELEMS)
@pytest.mark.parametrize("d,dv,bias", [(40, 72, "finite"), (64, 8, "masked"), (3, 5, "finite")])
def test_strided_operands_give_the_contiguous_calls_bits(d, dv, bias, elem):
    case = db.Case("edges", d, dv, bias, 3)
    op = db.operands(case, elem)
    plain = run(case, elem, layout="contiguous")
    for layout in ("suite", "padded"):               # permuted q and grad_out with k, v at head stride 0; a row stride above the width
        got = run(case, elem, layout=layout)
        assert got["tag"] == plain["tag"], layout
        assert_same_bits(got["dbias"], plain["dbias"], f"{layout} layout")
    if op["bias"].ndim == 1:                         # a shared bias against the same bias written out per head
        per_head = dict(op, bias=np.ascontiguousarray(np.broadcast_to(op["bias"], (3, op["bias"].shape[0]))))
        assert_same_bits(run(case, elem, op=per_head)["dbias"], plain["dbias"], "a shared bias")
    # an odd row stride: element lanes; the result stays inside the tolerance
    q, k, v, g, bd = device_operands(op, elem, "contiguous")
    odd = lambda t: torch.cat([t, torch.zeros_like(t[:, :, :1])], dim=2)[:, :, :t.shape[2]]          # noqa: E731
    pat = pattern("edges")
    out, lse = forward(pat, elem, q, k, v, op["scale"], bd)
    got = dbias_call(pat, elem, odd(q), odd(k), odd(v), out, lse, odd(g), op["scale"], bd)
    assert capi_attn_csr_dbias.last_kernel() == db.tag_of(elem, d, dv, False)
    assert db.inside_tolerance(dict(dbias=got.cpu().numpy(), lse=lse.cpu().numpy()), case, elem)[0]


@pytest.mark.parametrize("elem", db.ELEMS)
def test_a_head_does_not_depend_on_h_and_two_runs_give_equal_bits(elem):
    case = db.Case("ragged", 40, 72, "finite", 3)
    op = db.operands(case, elem)
    all_heads = run(case, elem)
    assert_same_bits(run(case, elem)["dbias"], all_heads["dbias"], "second run")
    for h in range(3):
        one = dict(op, q=op["q"][h:h + 1], g=op["g"][h:h + 1], bias=op["bias"][h])
        got = run(case, elem, op=one)
        assert got["tag"] == all_heads["tag"]
        assert_same_bits(got["dbias"][0], all_heads["dbias"][h], f"head {h} alone")
    # no bias: the gradient with respect to the scores, the same bits as with a bias of zeros
    assert_same_bits(run(case, elem, op=dict(op, bias=None))["dbias"], run(case, elem, op=dict(op, bias=np.zeros_like(op["bias"])))["dbias"], "bias=None")


def test_replays_from_a_graph():
    case = db.Case("edges", 40, 72, "masked", 3)
    op, pat = db.operands(case), pattern("edges")
    q, k, v, g, bias = device_operands(op, "f32")
    out, lse = forward(pat, "f32", q, k, v, op["scale"], bias)
    first = dbias_call(pat, "f32", q, k, v, out, lse, g, op["scale"], bias).clone()
    buf = torch.empty_like(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up outside the capture
        dbias_call(pat, "f32", q, k, v, out, lse, g, op["scale"], bias, dbias=buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dbias_call(pat, "f32", q, k, v, out, lse, g, op["scale"], bias, dbias=buf)
    buf.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(buf.cpu().numpy(), first.cpu().numpy(), "graph replay")


def test_every_tag_of_the_census_table_is_reached():
    pat = pattern("edges")
    csr = pat.csr
    rng = np.random.default_rng(182)
    seen = set()
    for tag, (elem, (d, dv, aligned)) in db.TAGS.items():
        pad = 0 if aligned else 1                    # an odd leading dimension: element lanes whatever the widths
        host = [full_mantissa(rng, (n, w), np.float32) for n, w in ((csr.num_rows, d), (csr.num_cols, d), (csr.num_cols, dv), (csr.num_rows, dv))]
        if elem == "bf16":
            host = [db.synth.bf16_round(x.reshape(-1)).reshape(x.shape) for x in host]
        q, k, v, g = (_put(np.concatenate([x, np.zeros((x.shape[0], pad), np.float32)], axis=1), elem)[:, :x.shape[1]] for x in host)
        out, lse = forward(pat, elem, q, k, v, d ** -0.5, None)
        got = dbias_call(pat, elem, q, k, v, out, lse, g, d ** -0.5, None)
        assert capi_attn_csr_dbias.last_kernel() == tag
        args = (csr, *(x[None] for x in host), d ** -0.5)
        assert np.all(np.abs(got.cpu().numpy()[None] - db.dbias_f64(*args)) <= db.dbias_tolerance(*args)), tag
        seen.add(tag)
    assert seen == set(db.TAGS) and len(seen) == 19


def test_refusals_launch_nothing():
    pat = pattern("edges")
    csr = pat.csr
    m, kk = csr.num_rows, csr.num_cols
    q, k, v, g, out = (torch.zeros((n, 8), device="cuda") for n in (m, kk, kk, m, m))
    lse = torch.zeros(m, device="cuda")
    sent = torch.full((csr.nnz,), 7.0, device="cuda")
    ops.spmm_csr(pat.fwd, torch.zeros((kk, 8), device="cuda"))
    before = capi.last_kernel()
    for bad in (dict(q=q.view(-1).as_strided((m, 8), (4, 1))),dict(dbias=lse), dict(scale=float("inf"))):
        args = dict(q=q, k=k, v=v, out=out, lse=lse, grad_out=g, scale=1.0, bias=None, dbias=sent)
        args.update(bad)
        with pytest.raises((ValueError, RuntimeError)):
            attn_csr_dbias.attention_csr_dbias(pat.fwd, *args.values())
    torch.cuda.synchronize()
    assert capi.last_kernel() == before and bool((sent == 7.0).all()), "a refused call must launch nothing"
    with pytest.raises(RuntimeError, match="overlaps an input"):
        attn_csr_dbias.attention_csr_dbias(pat.fwd, q, k, v, out, lse, g, 1.0, sent, dbias=sent)


# ---- autograd
def _autograd_operands(heads, shared, bf16):
    csr = matrix("long")
    rng = np.random.default_rng(183 + heads + 10 * shared)
    d = 8
    q, k, v, g = (full_mantissa(rng, (heads, n, d), np.float32) for n in (csr.num_rows, csr.num_cols, csr.num_cols, csr.num_rows))
    if bf16:
        q, k, v, g = (db.synth.bf16_round(x.reshape(-1)).reshape(x.shape) for x in (q, k, v, g))
    bias = rng.uniform(-2, 2, (csr.nnz,) if shared else (heads, csr.nnz)).astype(np.float32)
    return csr, q, k, v, g, bias, d ** -0.5


PATHS = {"unfused": (False, dict()), "fused": (False, dict(fused=True)), "fused_backward": (False, dict(fused=True, fused_backward=True)),
         "bf16": (True, dict()), "bf16_fused_backward": (True, dict(fused_backward=True))}


# the unfused composition takes 2-D operands: one head
@pytest.mark.parametrize("path,heads,shared", [(p, h, s) for p in sorted(PATHS) for h, s in ((1, False), (2, False), (2, True)) if p != "unfused" or h == 1])
def test_bias_grad_through_autograd(path, heads, shared):
    bf16, kw = PATHS[path]
    csr, q, k, v, g, bias, scale = _autograd_operands(heads, shared, bf16)
    a = autograd.TrainableCSR.from_host(csr)
    squeeze = (lambda x: x[0]) if heads == 1 else (lambda x: x)
    put = (lambda x: dev(squeeze(x)).to(torch.bfloat16)) if bf16 else (lambda x: dev(squeeze(x)))
    fn = autograd.sparse_attention_bf16 if bf16 else autograd.sparse_attention
    bias_h = bias if shared else squeeze(bias)

    def grads(train_bias, train_qkv=True):
        qd, kd, vd = (put(x).requires_grad_(train_qkv) for x in (q, k, v))
        bd = dev(bias_h).requires_grad_(train_bias)
        with torch.autograd.set_multithreading_enabled(False):
            out = fn(a, qd, kd, vd, scale=scale, bias=bd, bias_grad=train_bias, **kw)
            out.backward(put(g).to(out.dtype))
            tag = capi.last_kernel()
        return [None if x.grad is None else x.grad for x in (qd, kd, vd, bd)], tag

    with pytest.raises(ValueError, match="bias is a constant"):
        fn(a, put(q), put(k), put(v), scale=scale, bias=dev(bias_h).requires_grad_(True), **kw)
    got, _ = grads(True)
    const, _ = grads(False)
    assert const[3] is None and got[3].dtype == torch.float32 and tuple(got[3].shape) == bias_h.shape
    for n, x, y in zip(("q.grad", "k.grad", "v.grad"), got, const):
        assert_same_bits(x.float().cpu().numpy(), y.float().cpu().numpy(), f"{path}: {n} with a trained bias against a constant one")
    args = (csr, q, k, v, g, scale, bias)
    want, tol = db.dbias_f64(*args), db.dbias_tolerance(*args)
    if shared:
        want, tol = want.sum(axis=0), tol.sum(axis=0) + bref.gamma_u(heads) * np.abs(want).sum(axis=0)
    else:
        want, tol = squeeze(want), squeeze(tol)
    err = np.abs(got[3].cpu().numpy().astype(np.float64) - want)
    print(f"bias.grad {path} H={heads} shared={shared}: max |err| / tolerance = {float(np.max(err / tol)):.3g}")
    assert np.all(err <= tol)
    # the bias alone: the new launch is the last one and the backward proper is not called
    if "fused_backward" in path or path == "bf16":
        seen = []
        real_f32, real_bf16 = ops.attention_csr_bwd, attn_csr_bf16.attention_csr_bf16_bwd
        ops.attention_csr_bwd = lambda *args, **kw: seen.append("f32") or real_f32(*args, **kw)
        attn_csr_bf16.attention_csr_bf16_bwd = lambda *args, **kw: seen.append("bf16") or real_bf16(*args, **kw)
        try:
            alone, tag = grads(True, train_qkv=False)
            assert not seen, seen
            grads(True)
            assert seen == ["bf16" if path == "bf16_fused_backward" else "f32"]
        finally:
            ops.attention_csr_bwd, attn_csr_bf16.attention_csr_bf16_bwd = real_f32, real_bf16
        assert tag.startswith("attn_csr_dbias<bf16," if path == "bf16_fused_backward" else "attn_csr_dbias<f32,"), tag
        assert alone[:3] == [None, None, None]
        assert_same_bits(alone[3].cpu().numpy(), got[3].cpu().numpy(), "bias.grad alone against bias.grad beside the others")
