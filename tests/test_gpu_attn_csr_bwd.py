"""The fused backward of attention on a CSR pattern (mispmm_attn_csr_bwd_f32 through ops.attention_csr_bwd and
autograd.sparse_attention(fused=True, fused_backward=True)) on the GPU: dq, dk, dv against float64 inside the derived
tolerances and inside the derived tight check around the kernel's own out and lse on every element; +0 bits where the header
promises them, the eight `need` subsets, NaN rows nobody names, padded outputs, determinism and graph replay, the census of
kernel tags, refusals, and autograd.  The checks are the functions tests/test_attn_csr_bwd_mutants_cpu.py runs the faulty
restatements through."""
import dataclasses
import functools
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, capi_attn_csr_bwd, formats, ops  # noqa: E402

import _attn_csr_bwd_mutants as mut  # noqa: E402
import _attn_csr_bwd_ref as bref  # noqa: E402
import _attn_csr_ref as ref  # noqa: E402
from _bits import assert_same_bits  # noqa: E402
from _softmax_ref import full_mantissa, matrix  # noqa: E402

pytestmark = pytest.mark.gpu
GRADS = ("dq", "dk", "dv")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the shared operands are read-only


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
    return upload(bref.matrix(name))


def device_operands(op):
    """The operands as the suite lays them out: q and g views of [M, H, .] storage, k and v one head expanded over all (head
    stride 0), a bias shared ([nnz]) or per head ([H, nnz]); one head: plain 2-D tensors."""
    heads = op["q"].shape[0]
    bias = None if op["bias"] is None else dev(op["bias"])
    if heads == 1:
        return dev(op["q"][0]), dev(op["k"][0]), dev(op["v"][0]), dev(op["g"][0]), bias
    q, g = (dev(np.ascontiguousarray(op[n].transpose(1, 0, 2))).permute(1, 0, 2) for n in ("q", "g"))
    k, v = (dev(op[n][0]).unsqueeze(0).expand(heads, -1, -1) for n in ("k", "v"))
    assert q.stride(0) == op["q"].shape[2] and g.stride(0) == op["g"].shape[2] and k.stride(0) == 0 and v.stride(0) == 0
    return q, k, v, g, bias


def run(pat, op, need=(True, True, True), **kw):
    """Forward, then backward: dict(out, lse, dq, dk, dv) as [H, ...] numpy arrays (None where not asked for)."""
    q, k, v, g, bias = device_operands(op)
    out, lse = ops.attention_csr(pat.fwd, q, k, v, scale=op["scale"], bias=bias, return_lse=True)
    grads = ops.attention_csr_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, scale=op["scale"], bias=bias, need=need, **kw)
    lift = lambda x: None if x is None else (x.unsqueeze(0) if op["q"].shape[0] == 1 else x).cpu().numpy()     # noqa: E731
    return dict(out=lift(out), lse=lift(lse), **{n: lift(x) for n, x in zip(GRADS, grads)})


@pytest.mark.parametrize("heads", bref.HEADS)
@pytest.mark.parametrize("bias", bref.BIASES)
@pytest.mark.parametrize("d,dv", bref.WIDTHS)
@pytest.mark.parametrize("name", bref.PATTERNS)
def test_against_float64_inside_the_tolerances_and_the_tight_check(name, d, dv, bias, heads):
    case = bref.Case(name, d, dv, bias, heads)
    got = run(pattern(name), bref.operands(case))
    assert capi_attn_csr_bwd.last_kernel() == bref.tags_of(d, dv, True)[-1]
    results = {what: check(got, case) for what, check in mut.CHECKS.items()}
    print(f"attn_csr_bwd {case.id}: worst |err| / tolerance (dq, dk, dv): "
          + "; ".join(f"{what} " + ", ".join(f"{w:.3g}" for w in worst) for what, (_, worst) in results.items()))
    for what, (ok, worst) in results.items():
        assert ok, f"{case.id}: {what} fails, worst (dq, dk, dv) {worst} x"
    csr = bref.matrix(name)
    empty_rows = np.diff(csr.row_ptrs.astype(np.int64)) == 0
    empty_cols = np.bincount(csr.col_idxs.astype(np.int64), minlength=csr.num_cols) == 0
    assert not got["dq"][:, empty_rows].view(np.uint32).any(), "an empty row must give a +0 row of dq"
    assert not got["dk"][:, empty_cols].view(np.uint32).any() and not got["dv"][:, empty_cols].view(np.uint32).any(), "an empty column: +0"


def test_a_column_masked_in_every_entry_gives_plus_zero_bits():
    case = bref.Case("edges", 8, 8, "finite", 3)
    op, csr = dict(bref.operands(case)), bref.matrix("edges")
    ptrs, cols = csr.row_ptrs.astype(np.int64), csr.col_idxs.astype(np.int64)
    lens = np.diff(ptrs)
    rows = np.repeat(np.arange(csr.num_rows), lens)
    # columns all of whose rows hold other entries too (their lse stays finite), several entries among them
    counts = np.bincount(cols, minlength=csr.num_cols)
    ok = [c for c in np.argsort(-counts)[:200] if counts[c] >= 2 and all(lens[r] > (cols[ptrs[r]:ptrs[r + 1]] == c).sum() for r in rows[cols == c])][:3]
    assert len(ok) == 3
    bias = op["bias"].copy()
    bias[:, np.isin(cols, ok)] = -np.inf
    op["bias"] = bias
    got = run(pattern("edges"), op)
    assert np.isfinite(got["lse"][:, lens > 0]).all()
    assert not got["dk"][:, ok].view(np.uint32).any() and not got["dv"][:, ok].view(np.uint32).any(), "a masked column must be +0 bit for bit"
    want, tols = bref.backward_f64(csr, op["q"], op["k"], op["v"], op["g"], op["scale"], bias), \
        bref.bwd_tolerances(csr, op["q"], op["k"], op["v"], op["g"], op["scale"], bias)
    for n, w, t in zip(GRADS, want, tols):
        assert np.all(np.abs(got[n] - w) <= t), n


def test_the_eight_need_subsets_keep_their_bits_and_launch_what_they_say():
    case = bref.Case("edgesT", 40, 72, "masked", 3)
    op, pat = bref.operands(case), pattern("edgesT")
    full = run(pat, op)
    m = pat.csr.num_rows
    for need in itertools.product((False, True), repeat=3):
        delta = torch.full((3, m), -5.0, device="cuda")
        got = run(pat, op, need=need, delta=delta if need[0] or need[1] else None)
        for n, wanted in zip(GRADS, need):
            if wanted:
                assert_same_bits(got[n], full[n], f"{n} with need={need}")
            else:
                assert got[n] is None
        tags = bref.tags_of(40, 72, True, need)
        # launches: the last tag (the forward's where nothing is asked for), and whether the row pass ran (it alone writes delta)
        assert capi_attn_csr_bwd.last_kernel() == (tags[-1] if tags else ref.tag_of(40, 72, True)), (need, capi_attn_csr_bwd.last_kernel())
        row_ran = bool((delta != -5.0).any())
        assert row_ran == (need[0] or need[1]) and len(tags) == int(row_ran) + int(need[1] or need[2])


def _shifted_edges():
    """`edges` with every column moved up by one on K + 2 columns: no entry names column 0 or the last one; its first and last
    rows are empty, so no entry lies in row 0 or in the last row either."""
    csr = matrix("edges")
    assert csr.row_ptrs[1] == 0 and csr.row_ptrs[-1] == csr.row_ptrs[-2]
    return formats.CSR(csr.num_rows, csr.num_cols + 2, csr.row_ptrs, (csr.col_idxs + 1).astype(np.uint32), csr.data)


@pytest.mark.parametrize("d,dv", [(8, 8), (3, 5), (40, 72), (1, 129)])
def test_a_nan_in_rows_that_no_entry_names_reaches_no_output(d, dv):
    csr = _shifted_edges()
    pat = upload(csr)
    rng = np.random.default_rng(178)
    op = dict(q=full_mantissa(rng, (1, csr.num_rows, d), np.float32), k=full_mantissa(rng, (1, csr.num_cols, d), np.float32),
              v=full_mantissa(rng, (1, csr.num_cols, dv), np.float32), g=full_mantissa(rng, (1, csr.num_rows, dv), np.float32), bias=None, scale=d ** -0.5)
    clean = run(pat, op)
    assert not any(np.isnan(clean[n]).any() for n in GRADS)
    planted = {n: op[n].copy() for n in ("q", "k", "v", "g")}
    for x in planted.values():
        x[0, 0], x[0, -1] = np.nan, np.nan           # row 0 (where a wrapped offset would land) and a row nobody names
    got = run(pat, dict(op, **planted))
    for n in GRADS:
        assert_same_bits(got[n], clean[n], f"{n} with NaN rows planted in q, k, v and grad_out")


def test_padded_outputs_keep_their_sentinels():
    case = bref.Case("edgesT", 40, 72, "finite", 3)
    op, pat = bref.operands(case), pattern("edgesT")
    want = run(pat, op)
    m, kk = pat.csr.num_rows, pat.csr.num_cols
    for pad in (8, 3):                                # 16-byte lanes, then an odd row stride: element lanes, the same contract
        stores = dict(dq=torch.full((3, m, 40 + pad), -5.0, device="cuda"), dk=torch.full((3, kk, 40 + pad), -5.0, device="cuda"),
                      dv=torch.full((3, kk, 72 + pad), -5.0, device="cuda"))
        views = dict(dq=stores["dq"][:, :, :40], dk=stores["dk"][:, :, :40], dv=stores["dv"][:, :, :72])
        got = run(pat, op, **views)
        assert capi_attn_csr_bwd.last_kernel() == bref.tags_of(40, 72, pad == 8)[-1]
        for n, w in (("dq", 40), ("dk", 40), ("dv", 72)):
            assert bool((stores[n][:, :, w:] == -5.0).all()), f"{n}: the bytes between rows must keep their sentinel"
            assert np.array_equal(got[n], stores[n][:, :, :w].cpu().numpy())
            if pad == 8:
                assert_same_bits(got[n], want[n], f"{n}= with a padded row stride")
        assert mut.bwd_composed(got, case)[0]


def test_deterministic_and_replays_from_a_graph():
    case = bref.Case("edgesT", 40, 72, "masked", 3)
    op, pat = bref.operands(case), pattern("edgesT")
    q, k, v, g, bias = device_operands(op)
    out, lse = ops.attention_csr(pat.fwd, q, k, v, scale=op["scale"], bias=bias, return_lse=True)
    call = lambda **kw: ops.attention_csr_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, scale=op["scale"], bias=bias, **kw)   # noqa: E731
    first = [x.clone() for x in call()]
    for x, y, n in zip(call(), first, GRADS):
        assert_same_bits(x.cpu().numpy(), y.cpu().numpy(), f"second run, {n}")
    bufs = dict(dq=torch.empty_like(first[0]), dk=torch.empty_like(first[1]), dv=torch.empty_like(first[2]), delta=torch.empty_like(lse))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up outside the capture
        call(**bufs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(**bufs)
    for x in bufs.values():
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for n, y in zip(GRADS, first):
        assert_same_bits(bufs[n].cpu().numpy(), y.cpu().numpy(), f"graph replay, {n}")


def test_every_tag_of_the_census_table_is_reached():
    pat = pattern("edges")
    csr = pat.csr
    rng = np.random.default_rng(179)
    seen = set()
    for tag, (d, dv, aligned) in ref.TAGS.items():
        pad = 0 if aligned else 1                    # an odd leading dimension: element lanes whatever the widths
        q, k, v, g = (dev(full_mantissa(rng, (n, w + pad), np.float32))[:, :w]
                      for n, w in ((csr.num_rows, d), (csr.num_cols, d), (csr.num_cols, dv), (csr.num_rows, dv)))
        out, lse = ops.attention_csr(pat.fwd, q, k, v, return_lse=True)
        only_q = ops.attention_csr_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, need=(True, False, False))[0]
        row_tag = capi_attn_csr_bwd.last_kernel()
        got = ops.attention_csr_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g)
        col_tag = capi_attn_csr_bwd.last_kernel()
        assert [row_tag, col_tag] == bref.tags_of(d, dv, aligned) and capi.last_kernel() == col_tag, (row_tag, col_tag, tag)
        assert_same_bits(only_q.cpu().numpy(), got[0].cpu().numpy(), f"{row_tag}: dq alone")
        args = (csr, *(x.cpu().numpy()[None] for x in (q, k, v, g)), d ** -0.5)
        for n, x, w, t in zip(GRADS, got, bref.backward_f64(*args), bref.bwd_tolerances(*args)):
            assert np.all(np.abs(x.cpu().numpy()[None] - w) <= t), (col_tag, n)
        seen |= {row_tag, col_tag}
    assert seen == set(bref.TAGS) and len(seen) == 20


def test_refusals_return_their_codes_and_launch_nothing():
    pat = pattern("edges")
    csr = pat.csr
    m, kk = csr.num_rows, csr.num_cols
    q, k, v, g, out = (torch.zeros((n, 8), device="cuda") for n in (m, kk, kk, m, m))
    lse, delta = torch.zeros(m, device="cuda"), torch.full((m,), 7.0, device="cuda")
    sent = dict(dq=torch.full((m, 8), 7.0, device="cuda"), dk=torch.full((kk, 8), 7.0, device="cuda"), dv=torch.full((kk, 8), 7.0, device="cuda"))
    bias = torch.zeros(csr.nnz, device="cuda")
    ops.spmm_csr(pat.fwd, torch.zeros((kk, 8), device="cuda"))
    before = capi.last_kernel()
    lib = capi_attn_csr_bwd.lib()
    p = lambda t: None if t is None else t.data_ptr()                # noqa: E731

    def call(**kw):
        args = dict(stream=None, H=1, M=m, K=kk, nnz=csr.nnz, ptrs=p(pat.fwd.row_ptrs), cols=p(pat.fwd.col_idxs), tptrs=p(pat.at.row_ptrs),
                    tcols=p(pat.at.col_idxs), perm=p(pat.perm), q=p(q), qh=0, ldq=8, k=p(k), kh=0, ldk=8, D=8, v=p(v), vh=0, ldv=8, Dv=8, scale=1.0,
                    bias=None, bh=0, out=p(out), oh=0, ldo=8, lse=p(lse), g=p(g), gh=0, ldg=8, delta=p(delta), dq=p(sent["dq"]), dqh=0, lddq=8,
                    dk=p(sent["dk"]), dkh=0, lddk=8, dv=p(sent["dv"]), dvh=0, lddv=8)
        assert set(kw) <= set(args)
        args.update(kw)
        return lib.mispmm_attn_csr_bwd_f32(*args.values())

    for kw, code in ((dict(D=257, ldq=257, ldk=257), capi.ERR_UNSUPPORTED), (dict(Dv=0), capi.ERR_UNSUPPORTED), (dict(scale=float("nan")), capi.ERR_INVALID_ARG),
                     (dict(q=None), capi.ERR_INVALID_ARG), (dict(out=None), capi.ERR_INVALID_ARG), (dict(lse=None), capi.ERR_INVALID_ARG),
                     (dict(g=None), capi.ERR_INVALID_ARG), (dict(delta=None), capi.ERR_INVALID_ARG), (dict(tptrs=None), capi.ERR_INVALID_ARG),
                     (dict(tcols=None, dq=None), capi.ERR_INVALID_ARG), (dict(bias=p(bias), perm=None), capi.ERR_INVALID_ARG),
                     (dict(ldg=7), capi.ERR_INVALID_ARG), (dict(lddk=4), capi.ERR_INVALID_ARG), (dict(K=1 << 28, ldk=8), capi.ERR_UNSUPPORTED),
                     (dict(dq=p(q)), capi.ERR_INVALID_ARG), (dict(dv=p(g)), capi.ERR_INVALID_ARG), (dict(dk=p(sent["dq"])), capi.ERR_INVALID_ARG),
                     (dict(delta=p(lse)), capi.ERR_INVALID_ARG)):
        assert call(**kw) == code, kw
        assert "attn_csr_bwd_f32" in capi_attn_csr_bwd.last_error()
    assert call(H=0, q=None, out=None) == capi.OK and call(M=0, ptrs=None) == capi.OK and call(dq=None, dk=None, dv=None, lse=None) == capi.OK
    torch.cuda.synchronize()
    assert capi.last_kernel() == before and all(bool((x == 7.0).all()) for x in (*sent.values(), delta)), "a refused call must launch nothing"
    with pytest.raises(ValueError, match="1 to 256"):
        big = torch.zeros((m, 260), device="cuda")
        ops.attention_csr_bwd(pat.fwd, pat.at, pat.perm, big, torch.zeros((kk, 260), device="cuda"), v, out, lse, g)
    with pytest.raises(ValueError, match="grad_out"):
        ops.attention_csr_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g.double())
    with pytest.raises(ValueError, match="perm"):
        ops.attention_csr_bwd(pat.fwd, pat.at, None, q, k, v, out, lse, g, bias=bias)
    with pytest.raises(ValueError, match="A\\^T"):
        ops.attention_csr_bwd(pat.fwd, pat.fwd, pat.perm, q, k, v, out, lse, g)
    with pytest.raises(ValueError, match="three flags"):
        ops.attention_csr_bwd(pat.fwd, pat.at, pat.perm, q, k, v, out, lse, g, need=(True, True))


# ---- autograd
def _chain_tolerances(csr, q, k, v, g, scale):
    from test_gpu_softmax import _attention_tolerances
    return _attention_tolerances(csr, q, k, v, g, scale, "fast")[1:]


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("heads", [1, 2])
def test_fused_backward_through_autograd(heads, with_bias):
    name, d = "long", 8
    csr = matrix(name)
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(146 + heads)
    q, k, v, g = (full_mantissa(rng, (heads, n, d), np.float32) for n in (csr.num_rows, csr.num_cols, csr.num_cols, csr.num_rows))
    bias = rng.uniform(-2, 2, (heads, csr.nnz)).astype(np.float32) if with_bias else None
    scale = d ** -0.5
    squeeze = (lambda x: x[0]) if heads == 1 else (lambda x: x)
    bd = None if bias is None else dev(squeeze(bias))

    def grads(**kw):
        qd, kd, vd = (dev(squeeze(x)).requires_grad_(True) for x in (q, k, v))
        with torch.autograd.set_multithreading_enabled(False):
            out = autograd.sparse_attention(a, qd, kd, vd, bias=bd, fused=True, **kw)
            out.backward(dev(squeeze(g)))
            tag = capi.last_kernel()
        return [x.grad.cpu().numpy().reshape(heads, *x.shape[-2:]) for x in (qd, kd, vd)], tag

    got, tag = grads(fused_backward=True)
    assert tag.startswith("attn_csr_bwd_col<")
    old, old_tag = grads()
    assert not old_tag.startswith("attn_csr_bwd")
    want = bref.backward_f64(csr, q, k, v, g, scale, bias)
    tols = bref.bwd_tolerances(csr, q, k, v, g, scale, bias)
    for n, x, w, t in zip(GRADS, got, want, tols):
        ok, worst = mut.tight._worst(x, w, t)
        print(f"fused_backward H={heads} bias={with_bias} {n}: max |err| / tolerance = {worst:.3g}")
        assert ok, n
    if bias is None:                # against the code path without the keyword, inside the sum of both tolerances
        for h in range(heads):
            chain = _chain_tolerances(csr, q[h], k[h], v[h], g[h], scale)
            for n, x, y, t, c in zip(GRADS, got, old, tols, chain):
                assert np.all(np.abs(x[h].astype(np.float64) - y[h]) <= t[h] + c), f"head {h} {n} against fused=True without the keyword"


def test_frozen_inputs_skip_their_work_and_calls_without_the_keyword_keep_their_bits():
    csr = matrix("long")
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(147)
    q, k, v = (full_mantissa(rng, (n, 8), np.float32) for n in (csr.num_rows, csr.num_cols, csr.num_cols))
    seen = []
    real = ops.attention_csr_bwd
    ops.attention_csr_bwd = lambda *args, **kw: seen.append(tuple(kw["need"])) or real(*args, **kw)
    try:
        with torch.autograd.set_multithreading_enabled(False):
            for trainable in ((False, False, True), (True, False, False), (False, True, False), (True, True, True)):
                qd, kd, vd = (dev(x).requires_grad_(t) for x, t in zip((q, k, v), trainable))
                autograd.sparse_attention(a, qd, kd, vd, fused=True, fused_backward=True).sum().backward()      # an expanded grad_out
                assert seen[-1] == trainable and [x.grad is not None for x in (qd, kd, vd)] == list(trainable)
                assert capi.last_kernel().startswith("attn_csr_bwd_row<" if trainable == (True, False, False) else "attn_csr_bwd_col<")
            out = autograd.sparse_attention(a, dev(q), dev(k), dev(v), fused=True, fused_backward=True)
            assert out.grad_fn is None and not out.requires_grad
            count = len(seen)
            # without the keyword the backward is the chain it was, bit for bit, and the new entry point is not called
            grads = []
            for _ in range(2):
                qd, kd, vd = (dev(x).requires_grad_(True) for x in (q, k, v))
                autograd.sparse_attention(a, qd, kd, vd, fused=True).backward(dev(np.ones((csr.num_rows, 8), np.float32)))
                grads.append([x.grad.cpu().numpy() for x in (qd, kd, vd)])
            q1, k1, v1 = (dev(x).requires_grad_(True) for x in (q, k, v))
            autograd.sparse_attention(a, q1, k1, v1, acc="fast").backward(dev(np.ones((csr.num_rows, 8), np.float32)))
            for n, x, y, z in zip(GRADS, grads[0], grads[1], (q1, k1, v1)):
                assert_same_bits(x, y, n)
                assert_same_bits(x, z.grad.cpu().numpy(), f"{n}: fused=True without the keyword against the unfused fast path")
            assert len(seen) == count
    finally:
        ops.attention_csr_bwd = real
    with pytest.raises(ValueError, match="needs fused=True"):
        autograd.sparse_attention(a, dev(q), dev(k), dev(v), fused_backward=True)


def test_against_the_chain_on_n4c6_b13():
    name, d, heads = "n4c6-b13", 64, 2
    csr = matrix(name)
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(148)
    q, k, v, g = (full_mantissa(rng, (heads, n, d), np.float32) for n in (csr.num_rows, csr.num_cols, csr.num_cols, csr.num_rows))
    scale = d ** -0.5
    both = []
    for kw in (dict(fused_backward=True), dict()):
        qd, kd, vd = (dev(x).requires_grad_(True) for x in (q, k, v))
        with torch.autograd.set_multithreading_enabled(False):
            autograd.sparse_attention(a, qd, kd, vd, fused=True, **kw).backward(dev(g))
        both.append([x.grad.cpu().numpy().astype(np.float64) for x in (qd, kd, vd)])
    tols = bref.bwd_tolerances(csr, q, k, v, g, scale)
    for h in range(heads):
        chain = _chain_tolerances(csr, q[h], k[h], v[h], g[h], scale)
        for n, x, y, t, c in zip(GRADS, both[0], both[1], tols, chain):
            err = np.abs(x[h] - y[h])
            print(f"fused backward against the chain, {name} D=Dv=64 head {h} {n}: max |diff| / (sum of tolerances) = {float(np.max(err / (t[h] + c))):.3g}")
            assert np.all(err <= t[h] + c), "every element within the sum of both tolerances"
