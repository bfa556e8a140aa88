"""Row softmax on a CSR pattern (mispmm_softmax_csr_f32 / _f64 and their backward) and the autograd functions built on it
(sddmm, edge_softmax, sparse_attention), on the GPU, against the numpy restatements and bounds of tests/_softmax_ref.py.

Worst |err| / bound printed on an MI355X (forward, backward): f32 REFERENCE 1, 0.997 (the 2^-24 term is the rounding
to fp32 itself); f64 0.226, 0.145; f32 FAST 0.999 (the 2^-126 flush term; 0.16 on the narrow scores), 0.263.  Worst
|row sum - 1| / (L u) 0.688; sparse_attention against the composed tolerance 0.0274.
tests/test_gpu_softmax_tight.py holds the same kernels to a derived tolerance without this slack, to exact tie rows and to offset rows."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, formats, ops  # noqa: E402

from _bits import assert_same_bits  # noqa: E402
from _ref64 import assert_same_bits64  # noqa: E402
from _sddmm_ref import bound as sddmm_bound, dense_of, entry_rows  # noqa: E402
from _softmax_ref import (EDGE_MATRICES, LD, assert_inside, bwd_bound, full_mantissa, fwd_bound, matrix, row_lengths,  # noqa: E402
                          row_sums, scores, softmax_bwd_rows, softmax_rows, spread)

pytestmark = pytest.mark.gpu

MATRICES = EDGE_MATRICES + ["ragged", "long", "n4c6-b13"]
DTYPES = {"f32": (np.float32, torch.float32), "f64": (np.float64, torch.float64)}
MODES = ("reference", "fast")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def device_csr(name):
    return ops.DeviceCSR.from_host(matrix(name), plan=False)


@functools.lru_cache(maxsize=None)
def case(name, kind, dt):
    """(scores, exact softmax, L, T) on the host for (matrix, generator, dtype), shared by the tests; read-only."""
    csr = matrix(name)
    s = scores(kind, csr.nnz, DTYPES[dt][0])
    return s, softmax_rows(csr.row_ptrs, s), row_lengths(csr.row_ptrs), spread(csr.row_ptrs, s)


def same_bits(dt):
    return assert_same_bits if dt == "f32" else assert_same_bits64


def expect_tag(name, prefix):
    tag = capi.last_kernel()
    assert tag.startswith(prefix + "<"), tag
    if "-g" in name:                                   # a matrix padded so that the host picks this group size
        assert f",G{name.split('-g')[1]}," in tag, tag


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("name", MATRICES)
def test_forward_within_the_stated_bounds_and_rows_sum_to_one(name, kind, dt):
    csr, a = matrix(name), device_csr(name)
    s, exact, length, t = case(name, kind, dt)
    sd = dev(s)
    u = 2.0 ** -24 if dt == "f32" else 2.0 ** -53
    for acc in MODES:
        out = ops.softmax_csr(a, sd, acc=acc)
        expect_tag(name, "softmax_csr")
        assert out.shape == (a.nnz,) and out.dtype == DTYPES[dt][1]
        got = out.cpu().numpy()
        what = f"forward {name} {kind} {dt} {acc} {capi.last_kernel()}"
        assert_inside(got, exact, fwd_bound(DTYPES[dt][0], acc, length, t, exact), what)
        sums, lens = row_sums(csr.row_ptrs, got)
        off = np.abs(sums - 1).astype(np.float64)
        print(f"{what}: max |row sum - 1| / (L u) = {float(np.max(off / (lens * u))):.3g}")
        assert np.all(off <= lens * u), f"{what}: rows {np.argwhere(off > lens * u)[:4].ravel().tolist()} do not sum to 1 within L u"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", EDGE_MATRICES + ["ragged"])
def test_exactness_anchors(name, dt):
    csr, a = matrix(name), device_csr(name)
    length = row_lengths(csr.row_ptrs)
    assert (length == 1).any()
    s, _, _, _ = case(name, "wide", dt)
    eq = dev(scores("equal", csr.nnz, DTYPES[dt][0]))
    for acc in MODES:
        got = ops.softmax_csr(a, dev(s), acc=acc).cpu().numpy()
        assert np.all(got[length == 1] == 1.0), f"{acc}: a row of one entry is not exactly 1"
        if acc == "reference" or dt == "f64":
            got = ops.softmax_csr(a, eq, acc=acc).cpu().numpy()
            want = (LD(1.0) / length.astype(LD)).astype(DTYPES[dt][0])           # the correctly rounded 1 / L
            assert np.array_equal(got, want), f"{acc}: equal scores differ from 1 / L in rows of {sorted(set(length[got != want].tolist()))}"
        dp0 = torch.zeros(a.nnz, dtype=DTYPES[dt][1], device="cuda")
        ds = ops.softmax_csr_bwd(a, dev(got), dp0, acc=acc).cpu().numpy()
        assert not ds.any() and not np.signbit(ds).any(), f"{acc}: the backward of an all-zero dp is not all +0"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", EDGE_MATRICES)
def test_masks_and_special_values(name, dt):
    csr, a = matrix(name), device_csr(name)
    rp = csr.row_ptrs.astype(np.int64)
    lens = np.diff(rp)
    rng = np.random.default_rng(8)
    s = scores("narrow", csr.nnz, DTYPES[dt][0]).copy()
    s[rng.random(csr.nnz) < 0.25] = -np.inf
    r_inf, r_nan, r_pinf, r_keep = [int(np.argwhere(lens == n)[0, 0]) for n in (17, 65, 300, 1025)]
    s[rp[r_inf]:rp[r_inf + 1]] = -np.inf                       # one row all -Inf
    s[rp[r_nan] + 40] = np.nan                                 # one row with a NaN
    s[rp[r_pinf] + 7] = np.inf                                 # one row with +Inf
    s[rp[r_keep]] = 0.0                                        # the longest row keeps a finite score
    want = softmax_rows(csr.row_ptrs, s, np.float64)           # the contract: NaN positions and zeros
    exact = softmax_rows(csr.row_ptrs, s)
    rows = entry_rows(csr.row_ptrs)
    dead = np.isnan(want)
    assert set(rows[dead].tolist()) >= {r_inf, r_nan, r_pinf} and (~dead).sum() > csr.nnz // 2
    masked = np.isneginf(s) & ~dead
    assert masked.sum() > csr.nnz // 8
    length, t = row_lengths(csr.row_ptrs), spread(csr.row_ptrs, s)
    for acc in MODES:
        got = ops.softmax_csr(a, dev(s), acc=acc).cpu().numpy()
        assert np.array_equal(np.isnan(got), dead), f"{acc}: NaN positions differ at {np.argwhere(np.isnan(got) != dead)[:4].ravel().tolist()}"
        assert not got[masked].any() and not np.signbit(got[masked]).any(), f"{acc}: a masked entry is not +0"
        live = ~dead
        assert_inside(got[live], exact[live], fwd_bound(DTYPES[dt][0], acc, length[live], t[live], exact[live]),
                      f"specials {name} {dt} {acc}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", EDGE_MATRICES + ["ragged"])
def test_in_place_gives_the_same_bits_and_leaves_the_tail_alone(name, dt):
    a = device_csr(name)
    s, _, _, _ = case(name, "narrow", dt)
    tdt = DTYPES[dt][1]
    dp = dev(full_mantissa(np.random.default_rng(9), a.nnz, DTYPES[dt][0]))
    for acc in MODES:
        p = ops.softmax_csr(a, dev(s), acc=acc)
        buf = torch.full((a.nnz + 37,), -7.0, dtype=tdt, device="cuda")
        buf[:a.nnz] = dev(s)
        got = ops.softmax_csr(a, buf[:a.nnz], out=buf[:a.nnz], acc=acc)
        assert got.data_ptr() == buf.data_ptr()
        same_bits(dt)(got, p.cpu().numpy(), f"in place forward {acc}")
        assert bool((buf[a.nnz:] == -7.0).all()), "elements behind out[nnz - 1] were written"
        ds = ops.softmax_csr_bwd(a, p, dp, acc=acc)
        buf = torch.full((a.nnz + 37,), -7.0, dtype=tdt, device="cuda")
        buf[:a.nnz] = dp
        got = ops.softmax_csr_bwd(a, p, buf[:a.nnz], out=buf[:a.nnz], acc=acc)
        assert got.data_ptr() == buf.data_ptr()
        same_bits(dt)(got, ds.cpu().numpy(), f"in place backward {acc}")
        assert bool((buf[a.nnz:] == -7.0).all()), "elements behind ds[nnz - 1] were written"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("name", MATRICES)
def test_backward_within_the_stated_bounds(name, kind, dt):
    csr, a = matrix(name), device_csr(name)
    s, _, length, _ = case(name, kind, dt)
    dp = full_mantissa(np.random.default_rng(10), csr.nnz, DTYPES[dt][0])
    for acc in MODES:
        p = ops.softmax_csr(a, dev(s), acc=acc)                 # p from the library's forward
        ds = ops.softmax_csr_bwd(a, p, dev(dp), acc=acc)
        expect_tag(name, "softmax_csr_bwd")
        ph = p.cpu().numpy()
        exact, cap = softmax_bwd_rows(csr.row_ptrs, ph, dp)
        assert_inside(ds.cpu().numpy(), exact, bwd_bound(DTYPES[dt][0], acc, length, ph, dp, cap, exact),
                      f"backward {name} {kind} {dt} {acc} {capi.last_kernel()}")


def test_empty_patterns_are_no_ops():
    empty = ops.DeviceCSR.from_host(formats.CSR(5, 7, np.zeros(6, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32)), plan=False)
    none = ops.DeviceCSR.from_host(formats.CSR(0, 7, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32)), plan=False)
    z = torch.zeros(0, device="cuda")
    for a in (empty, none):
        assert ops.softmax_csr(a, z).shape == (0,) and ops.softmax_csr_bwd(a, z, z).shape == (0,)
    with pytest.raises(ValueError):
        ops.softmax_csr(empty, torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError):
        ops.softmax_csr_bwd(empty, z, z.double())


@pytest.mark.parametrize("dt", list(DTYPES))
def test_deterministic_and_replays_from_a_graph(dt):
    name = "edges"
    a = device_csr(name)
    sd = dev(case(name, "narrow", dt)[0])
    dp = dev(full_mantissa(np.random.default_rng(11), a.nnz, DTYPES[dt][0]))
    same = same_bits(dt)
    for acc in MODES:
        p = ops.softmax_csr(a, sd, acc=acc).clone()
        ds = ops.softmax_csr_bwd(a, p, dp, acc=acc).clone()
        same(ops.softmax_csr(a, sd, acc=acc), p.cpu().numpy(), f"second run {acc}")
        same(ops.softmax_csr_bwd(a, p, dp, acc=acc), ds.cpu().numpy(), f"second backward run {acc}")
        p2, ds2 = torch.empty_like(p), torch.empty_like(ds)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                               # warm-up outside the capture
            ops.softmax_csr(a, sd, out=p2, acc=acc)
            ops.softmax_csr_bwd(a, p2, dp, out=ds2, acc=acc)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.softmax_csr(a, sd, out=p2, acc=acc)
            ops.softmax_csr_bwd(a, p2, dp, out=ds2, acc=acc)
        p2.zero_()
        ds2.zero_()
        g.replay()
        torch.cuda.synchronize()
        same(p2, p.cpu().numpy(), f"graph replay {acc}")
        same(ds2, ds.cpu().numpy(), f"graph replay backward {acc}")


# ---- autograd
def _tiny():
    """7 x 9, 20 entries, row 2 empty, column 4 twice in row 5."""
    lens = [3, 4, 0, 2, 5, 4, 2]
    cols = [0, 3, 8, 1, 2, 5, 7, 4, 6, 0, 1, 3, 5, 8, 4, 2, 4, 7, 6, 8]
    rng = np.random.default_rng(41)
    return formats.CSR(7, 9, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), np.array(cols, np.uint32),
                       rng.uniform(-1, 1, 20).astype(np.float64))


def _flags(n):
    """Every non-empty choice of which of n inputs require a gradient: each alone, then all."""
    return [tuple(i == j for i in range(n)) for j in range(n)] + [(True,) * n]


@pytest.mark.parametrize("acc", MODES)
def test_gradcheck_in_float64(acc):
    csr = _tiny()
    a = autograd.TrainableCSR.from_host(csr, dtype=torch.float64)
    rng = np.random.default_rng(42)
    s0 = dev(rng.uniform(-2, 2, csr.nnz))
    assert torch.autograd.gradcheck(lambda s: autograd.edge_softmax(a, s, acc=acc), (s0.clone().requires_grad_(True),))
    x0, y0, v0 = dev(rng.uniform(-1, 1, (7, 5))), dev(rng.uniform(-1, 1, (9, 5))), dev(rng.uniform(-1, 1, (9, 3)))
    for wx, wy in _flags(2):
        x, y = x0.clone().requires_grad_(wx), y0.clone().requires_grad_(wy)
        assert torch.autograd.gradcheck(lambda p, q: autograd.sddmm(a, p, q, acc=acc), (x, y))
    for wq, wk, wv in _flags(3):
        q, k, v = x0.clone().requires_grad_(wq), y0.clone().requires_grad_(wk), v0.clone().requires_grad_(wv)
        assert torch.autograd.gradcheck(lambda p, r, t: autograd.sparse_attention(a, p, r, t, acc=acc), (q, k, v))
    assert torch.autograd.gradcheck(lambda p, r, t: autograd.sparse_attention(a, p, r, t, scale=0.3, acc=acc), (q, k, v))


def _dense_attention(csr, q, k, v, g, scale):
    """float64 dense masked attention on the pattern (a repeated (row, column) pair is not among these matrices):
    (out, dq, dk, dv) as numpy arrays."""
    mask = torch.from_numpy(dense_of(formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, np.ones(csr.nnz))) > 0)
    qt, kt, vt = (torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in (q, k, v))
    sc = ((qt * scale) @ kt.t()).masked_fill(~mask, float("-inf"))
    p = torch.softmax(sc, dim=1).masked_fill(~mask.any(dim=1, keepdim=True), 0.0)      # a row without entries: a zero row
    out = p @ vt
    out.backward(torch.from_numpy(g.astype(np.float64)))
    return out.detach().numpy(), qt.grad.numpy(), kt.grad.numpy(), vt.grad.numpy()


def _attention_tolerances(csr, q, k, v, g, scale, acc):
    """Tolerances on (out, dq, dk, dv) of the float32 chain, composed from the three stated bounds by first-order error
    propagation in float64: each kernel's own bound at the exact values, plus the bounds of the kernels before it carried
    through the step's derivative.  Second-order terms are covered by evaluating every propagated factor at (value + its
    own error) and by the factor 1.01 on the whole."""
    f64 = np.float64
    rows, cols = entry_rows(csr.row_ptrs), csr.col_idxs.astype(np.int64)
    d = q.shape[1]
    u = 2.0 ** -24
    pattern = lambda vals: dense_of(formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, vals))   # noqa: E731
    length = row_lengths(csr.row_ptrs)
    u2 = 2 * u                                                                  # q' = fl(q * fl(scale)): two roundings
    qs = q.astype(f64) * scale
    s = (qs[rows] * k.astype(f64)[cols]).sum(axis=1)
    s_abs = (np.abs(qs[rows]) * np.abs(k.astype(f64)[cols])).sum(axis=1)
    e_s = sddmm_bound(np.float32, acc, d, s, s_abs * (1 + u2)) + u2 * s_abs     # SDDMM's bound + the rounded q'
    p = softmax_rows(csr.row_ptrs, s).astype(f64)
    # a score error of at most e per entry of a row moves every quotient by a factor within exp(+-2 e)
    e_row = np.zeros(csr.num_rows)
    np.maximum.at(e_row, rows, e_s)
    shift = np.expm1(2 * e_row[rows])
    e_p = p * shift + fwd_bound(np.float32, acc, length, spread(csr.row_ptrs, s) + 2 * e_row[rows], p * (1 + shift))
    prod = lambda a_abs, b_abs, e_a: 1e-5 * ((a_abs + e_a) @ b_abs) + e_a @ b_abs          # noqa: E731  the product's bound + A's error
    tol_out = prod(pattern(p), np.abs(v).astype(f64), pattern(e_p))
    tol_dv = prod(pattern(p).T, np.abs(g).astype(f64), pattern(e_p).T)
    dp = (g.astype(f64)[rows] * v.astype(f64)[cols]).sum(axis=1)
    dp_abs = (np.abs(g.astype(f64)[rows]) * np.abs(v.astype(f64)[cols])).sum(axis=1)
    e_dp = sddmm_bound(np.float32, acc, v.shape[1], dp, dp_abs)
    ds, cap = (x.astype(f64) for x in softmax_bwd_rows(csr.row_ptrs, p, dp))
    # ds = p (dp - <p, dp>): the kernel's bound at the perturbed operands, then the operands' errors through the formula
    ph, dph = p + e_p, np.abs(dp) + e_dp
    cap_h = np.zeros(csr.num_rows)
    np.add.at(cap_h, rows, ph * dph)
    e_dot = np.zeros(csr.num_rows)
    np.add.at(e_dot, rows, e_p * dph + ph * e_dp)
    e_ds = (bwd_bound(np.float32, acc, length, ph, dph, cap_h[rows], ph * (dph + cap_h[rows]))
            + e_p * (dph + cap_h[rows]) + ph * (e_dp + e_dot[rows]))
    tol_dq = (prod(np.abs(pattern(ds)), np.abs(k).astype(f64), pattern(e_ds)) * (1 + u2)
              + u2 * (np.abs(pattern(ds)) @ np.abs(k).astype(f64))) * scale               # dq = fl(dq' * fl(scale))
    tol_dk = prod(np.abs(pattern(ds)).T, np.abs(qs) * (1 + u2), pattern(e_ds).T) + u2 * (np.abs(pattern(ds)).T @ np.abs(qs))
    return [1.01 * t + 1e-30 for t in (tol_out, tol_dq, tol_dk, tol_dv)]


@pytest.mark.parametrize("d", [8, 64])
@pytest.mark.parametrize("name", ["long", "ragged"])
def test_sparse_attention_float32_against_dense_masked_attention(name, d):
    csr = matrix(name)
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(46)
    q, k = full_mantissa(rng, (csr.num_rows, d), np.float32), full_mantissa(rng, (csr.num_cols, d), np.float32)
    v, g = full_mantissa(rng, (csr.num_cols, d), np.float32), full_mantissa(rng, (csr.num_rows, d), np.float32)
    scale = d ** -0.5
    want = _dense_attention(csr, q, k, v, g, scale)
    for acc in MODES:
        qd, kd, vd = (dev(x).requires_grad_(True) for x in (q, k, v))
        out = autograd.sparse_attention(a, qd, kd, vd, acc=acc)
        out.backward(dev(g))
        got = [x.detach().cpu().numpy() for x in (out, qd.grad, kd.grad, vd.grad)]
        tols = _attention_tolerances(csr, q, k, v, g, scale, acc)
        for what, gv, wv, tol in zip(("out", "dq", "dk", "dv"), got, want, tols):
            err = np.abs(gv.astype(np.float64) - wv)
            print(f"attention {name} d={d} {acc} {what}: max |err| / tolerance = {float(np.max(err / tol)):.3g}")
            assert np.all(err <= tol), f"{name} d={d} {acc}: {what} outside the composed tolerance"


def test_frozen_inputs_skip_their_kernels():
    csr = matrix("long")
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(47)
    x_h, y_h = full_mantissa(rng, (csr.num_rows, 8), np.float32), full_mantissa(rng, (csr.num_cols, 8), np.float32)
    t_rows = a.tpattern.num_rows
    # the tag of the last kernel is kept per thread: run the backward passes on this one
    with torch.autograd.set_multithreading_enabled(False):
        # sddmm: each gradient is one product; its tag ends the backward pass.  Tell the two apart by running the other first.
        x, y = dev(x_h).requires_grad_(True), dev(y_h)
        sc = autograd.sddmm(a, x, y)
        assert capi.last_kernel().startswith("sddmm_csr<")
        sc.sum().backward()
        assert not capi.last_kernel().startswith("sddmm_csr<"), capi.last_kernel()      # a product ran
        assert x.grad is not None and x.grad.shape == (csr.num_rows, 8) and y.grad is None
        x, y = dev(x_h), dev(y_h).requires_grad_(True)
        sc = autograd.sddmm(a, x, y)
        sc.sum().backward()
        assert not capi.last_kernel().startswith("sddmm_csr<"), capi.last_kernel()
        assert y.grad is not None and y.grad.shape == (t_rows, 8) and x.grad is None
        # with neither trainable nothing is recorded
        out = autograd.sddmm(a, dev(x_h), dev(y_h))
        assert out.grad_fn is None and not out.requires_grad
        # edge_softmax: the backward is the one softmax_csr_bwd launch
        s = dev(scores("narrow", csr.nnz, np.float32)).requires_grad_(True)
        p = autograd.edge_softmax(a, s)
        assert capi.last_kernel().startswith("softmax_csr<")
        (p * dev(full_mantissa(rng, csr.nnz, np.float32))).sum().backward()
        assert capi.last_kernel().startswith("softmax_csr_bwd<"), capi.last_kernel()
        assert s.grad is not None
        p = autograd.edge_softmax(a, s.detach())
        assert p.grad_fn is None
        # sparse_attention with only v trainable: the backward is the transposed product alone -- no SDDMM for dP, no
        # softmax backward, no score gradients
        q, k, v = dev(x_h), dev(y_h), dev(y_h).requires_grad_(True)
        out = autograd.sparse_attention(a, q, k, v)
        ops.softmax_csr_bwd(a.fwd, p, p)                                             # leave a tag behind ...
        assert capi.last_kernel().startswith("softmax_csr_bwd<")
        out.sum().backward()
        tag = capi.last_kernel()
        assert not tag.startswith("softmax_csr") and not tag.startswith("sddmm_csr<"), tag   # ... which the product replaces
        assert v.grad is not None
        # with only q trainable the chain runs back to the scores: SDDMM (dP), softmax backward, then the product for dq
        q, k, v = dev(x_h).requires_grad_(True), dev(y_h), dev(y_h)
        autograd.sparse_attention(a, q, k, v).sum().backward()
        assert q.grad is not None and not capi.last_kernel().startswith("softmax_csr"), capi.last_kernel()
    with pytest.raises(ValueError):
        autograd.sddmm(a, dev(x_h).double(), dev(y_h))
    with pytest.raises(ValueError):
        autograd.edge_softmax(a, dev(x_h))
