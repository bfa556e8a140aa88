"""Row softmax on a CSR pattern on a machine WITHOUT a GPU: the numpy restatement of the contract against closed forms, the
stated bounds against a plain float64 softmax (they must be satisfiable by a correct implementation), the entry points'
argument validation (which happens before any device work) and the Python layer's refusals."""
import ctypes

import numpy as np
import pytest

from mispmm import capi, ops

from _softmax_ref import (EDGE_LENGTHS, EDGE_MATRICES, GROUPS, LD, REGS, assert_inside, bwd_bound, full_mantissa, fwd_bound,
                          matrix, picked_group, row_lengths, row_sums, scores, softmax_bwd_rows, softmax_rows, spread)

GPU_MATRICES = EDGE_MATRICES + ["ragged", "long", "n4c6-b13"]


def test_restatement_agrees_with_closed_forms_on_tiny_rows():
    ptr = np.array([0, 0, 1, 3, 3, 6], np.uint32)                # rows of 0, 1, 2, 0 and 3 entries
    s = np.array([5.0, 0.0, np.log(3.0), 1.0, 1.0, 1.0])
    p = softmax_rows(ptr, s, np.float64)
    assert p[0] == 1.0
    assert np.allclose(p[1:3], [0.25, 0.75], rtol=1e-15, atol=0)
    assert np.array_equal(p[3:], np.full(3, 1.0 / 3.0))
    assert np.array_equal(spread(ptr, s), [0, np.log(3.0), np.log(3.0), 0, 0, 0])
    assert np.array_equal(row_lengths(ptr), [1, 2, 2, 3, 3, 3])
    # backward of the row of two: ds = p (dp - <p, dp>) = [0.25 (1 - 1.75), 0.75 (2 - 1.75)]
    dp = np.array([9.0, 1.0, 2.0, 0.0, 0.0, 0.0])
    ds, cap = softmax_bwd_rows(ptr, p, dp, np.float64)
    assert ds[0] == 0.0 and np.allclose(ds[1:3], [-0.1875, 0.1875], rtol=1e-15, atol=0)
    assert np.array_equal(ds[3:], np.zeros(3)) and not np.signbit(ds[3:]).any()
    assert np.allclose(cap, [9.0, 1.75, 1.75, 0, 0, 0], rtol=1e-15, atol=0)
    sums, lens = row_sums(ptr, p)
    assert np.array_equal(lens, [1, 2, 3]) and np.allclose(sums.astype(np.float64), 1.0, rtol=1e-15)


def test_restatement_of_the_special_values_is_torch_softmax():
    torch = pytest.importorskip("torch")
    inf, nan = np.inf, np.nan
    rows = [[1.0, -inf, 2.0], [-inf, -inf], [0.5, nan, 1.0], [inf, 1.0], [-inf, 3.0], [-inf]]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    got = softmax_rows(ptr, np.concatenate(rows), np.float64)
    want = np.concatenate([torch.softmax(torch.tensor(r, dtype=torch.float64), 0).numpy() for r in rows])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isnan(got), [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1])
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=1e-15, atol=0)
    assert got[1] == 0.0 and not np.signbit(got[1]) and got[10] == 0.0 and got[11] == 1.0


def test_the_edge_matrices_hold_the_lengths_they_claim_and_pick_every_group():
    lens = set(np.diff(matrix("edges").row_ptrs.astype(np.int64)).tolist())
    for g in GROUPS:
        assert {g - 1, g, g + 1} <= lens and {REGS * g, REGS * g + 1} <= lens
    assert {0, 1, 2, 3, 4, 300, 1025} <= lens
    assert EDGE_LENGTHS[0] == 0 and EDGE_LENGTHS[1] == 0 and EDGE_LENGTHS[-1] == 0
    for g in GROUPS:
        m = matrix(f"edges-g{g}")
        assert picked_group(m.num_rows, m.nnz) == g
    assert picked_group(matrix("edges").num_rows, matrix("edges").nnz) == 32


@pytest.mark.parametrize("kind", ["narrow", "wide", "equal"])
@pytest.mark.parametrize("name", GPU_MATRICES)
def test_a_plain_float64_softmax_lies_inside_the_f64_bound(name, kind):
    """The bounds are satisfiable: numpy's float64 arithmetic (exp, pairwise sum, division), taken alone, stays inside the
    tightest of them on every matrix and generator the GPU tests use -- forward and backward."""
    csr = matrix(name)
    s = scores(kind, csr.nnz, np.float64)
    exact = softmax_rows(csr.row_ptrs, s)
    lim = fwd_bound(np.float64, "reference", row_lengths(csr.row_ptrs), spread(csr.row_ptrs, s), exact)
    p = softmax_rows(csr.row_ptrs, s, np.float64)
    assert assert_inside(p, exact, lim, f"float64 numpy forward {name} {kind}") <= 1.0
    dp = full_mantissa(np.random.default_rng(5), csr.nnz, np.float64)
    ds_exact, cap = softmax_bwd_rows(csr.row_ptrs, p, dp)
    ds, _ = softmax_bwd_rows(csr.row_ptrs, p, dp, np.float64)
    assert_inside(ds, ds_exact, bwd_bound(np.float64, "reference", row_lengths(csr.row_ptrs), p, dp, cap, ds_exact),
                  f"float64 numpy backward {name} {kind}")


def test_the_backward_bounds_need_their_underflow_term():
    """Why the backward bounds end in a multiple of tiny: with scores 100 apart an fp32 p[e] is subnormal, ds[e] ~ p[e] lands
    on the subnormal grid, and even the CORRECTLY ROUNDED fp32 result is off by up to tiny / 2 -- 2^24 times the relative
    terms alone.  With the term, the correctly rounded result is inside."""
    csr = matrix("edges")
    length = row_lengths(csr.row_ptrs)
    p = softmax_rows(csr.row_ptrs, scores("wide", csr.nnz, np.float32)).astype(np.float32)
    assert ((p > 0) & (p < 2.0 ** -126)).any()
    dp = full_mantissa(np.random.default_rng(10), csr.nnz, np.float32)
    exact, cap = softmax_bwd_rows(csr.row_ptrs, p, dp)
    best = exact.astype(np.float32)                                # nothing in fp32 is closer
    lim = bwd_bound(np.float32, "reference", length, p, dp, cap, exact)
    assert_inside(best, exact, lim, "correctly rounded fp32 backward")
    err = np.abs(best.astype(LD) - exact)
    assert (err > lim - 2.0 ** -149).any(), "the relative terms alone would hold: the underflow term is not needed"


def test_equal_scores_in_fp64_then_fp32_is_the_correctly_rounded_quotient():
    """The f32 REFERENCE anchor rounds the fp64 quotient 1 / L to fp32; for every row length of the tests that IS the
    correctly rounded 1 / L (no double-rounding case among them)."""
    for n in sorted(set(EDGE_LENGTHS + list(range(1, 41)) + [77, 129]) - {0}):
        twice = np.float32(np.float64(1.0) / np.float64(n))
        once = np.float32(LD(1.0) / LD(n))
        assert twice == once, n


@pytest.mark.parametrize("fn", ["mispmm_softmax_csr_f32", "mispmm_softmax_csr_f64", "mispmm_softmax_csr_bwd_f32", "mispmm_softmax_csr_bwd_f64"])
def test_softmax_validates_before_any_device_work(fn):
    l = capi.lib()
    bwd = "_bwd_" in fn
    one = ctypes.c_void_p(16)   # never dereferenced: every call below must return from validation

    def call(m, nnz, row_ptrs, a, b, out, acc):
        args = (None, m, nnz, row_ptrs, a) + ((b,) if bwd else ()) + (out, acc)
        return getattr(l, fn)(*args)
    assert call(4, 3, None, one, one, one, 0) == capi.ERR_INVALID_ARG
    assert call(4, 3, one, None, one, one, 0) == capi.ERR_INVALID_ARG
    assert call(4, 3, one, one, one, None, 1) == capi.ERR_INVALID_ARG
    if bwd:
        assert call(4, 3, one, one, None, one, 1) == capi.ERR_INVALID_ARG
    assert b"null" in l.mispmm_last_error() and fn[len("mispmm_"):].encode() in l.mispmm_last_error()
    for acc in (2, 7, -1):
        assert call(4, 3, one, one, one, one, acc) == capi.ERR_INVALID_ARG
        assert b"accumulate mode" in l.mispmm_last_error()
    assert call(4, 0, one, None, None, None, 7) == capi.ERR_INVALID_ARG            # the mode is checked even for a no-op
    assert call(4, 0, one, None, None, None, 0) == capi.OK                         # nnz == 0: a no-op
    assert call(0, 0, None, None, None, None, 1) == capi.OK                        # M == 0
    assert call(0, 5, None, None, None, None, 0) == capi.OK
    # no 2 GiB refusal to test: the kernels address through 64-bit pointers and decline no array size (mispmm.h)


def test_python_layer_without_a_gpu():
    torch = pytest.importorskip("torch")
    from mispmm import autograd
    csr = matrix("long")
    a = ops.DeviceCSR.from_host(csr, device="cpu")
    s = torch.zeros(csr.nnz)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.softmax_csr(a, s)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.softmax_csr_bwd(a, s, s)
    for dtype in (torch.float32, torch.float64):
        t = autograd.TrainableCSR.from_host(csr, device="cpu", dtype=dtype)
        q, k = torch.zeros(csr.num_rows, 8, dtype=dtype), torch.zeros(csr.num_cols, 8, dtype=dtype)
        with pytest.raises(ValueError, match="no CPU path"):
            autograd.sddmm(t, q, k)
        with pytest.raises(ValueError, match="no CPU path"):
            autograd.edge_softmax(t, torch.zeros(csr.nnz, dtype=dtype))
        with pytest.raises(ValueError, match="no CPU path"):
            autograd.sparse_attention(t, q, k, k)


class _OnDevice:
    """A stand-in that says it lives on the device, so that the checks behind the CPU refusal can run here; every call
    below must raise before anything would be read."""
    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_wrong_dtypes_and_shapes_are_refused():
    torch = pytest.importorskip("torch")
    from mispmm import autograd
    csr = matrix("long")
    t = autograd.TrainableCSR.from_host(csr, device="cpu")
    t.fwd.row_ptrs = _OnDevice(t.fwd.row_ptrs)
    dev = lambda *shape, dtype=torch.float32: _OnDevice(torch.zeros(*shape, dtype=dtype))   # noqa: E731
    m, k, nnz = csr.num_rows, csr.num_cols, csr.nnz
    bad_ops = [lambda: ops.softmax_csr(t.fwd, dev(nnz, dtype=torch.float16)),
               lambda: ops.softmax_csr(t.fwd, dev(nnz + 1)),
               lambda: ops.softmax_csr(t.fwd, dev(nnz, 1)),
               lambda: ops.softmax_csr(t.fwd, _OnDevice(torch.zeros(2 * nnz)[::2])),
               lambda: ops.softmax_csr(t.fwd, dev(nnz), out=dev(nnz, dtype=torch.float64)),
               lambda: ops.softmax_csr(t.fwd, dev(nnz), out=dev(nnz - 1)),
               lambda: ops.softmax_csr_bwd(t.fwd, dev(nnz), dev(nnz, dtype=torch.float64)),
               lambda: ops.softmax_csr_bwd(t.fwd, dev(nnz), dev(nnz - 1)),
               lambda: ops.softmax_csr_bwd(t.fwd, dev(nnz, dtype=torch.int32), dev(nnz, dtype=torch.int32)),
               lambda: ops.softmax_csr_bwd(t.fwd, dev(nnz), dev(nnz), out=dev(nnz + 2)),
               lambda: autograd.edge_softmax(t, dev(nnz, dtype=torch.float64)),
               lambda: autograd.edge_softmax(t, dev(nnz - 1)),
               lambda: autograd.sddmm(t, dev(m, 8, dtype=torch.float64), dev(k, 8)),
               lambda: autograd.sddmm(t, dev(m, 8), dev(k, 8, dtype=torch.float64)),
               lambda: autograd.sddmm(t, dev(m + 1, 8), dev(k, 8)),
               lambda: autograd.sddmm(t, dev(m, 8), dev(k, 4)),
               lambda: autograd.sddmm(t, dev(m * 8), dev(k, 8)),
               lambda: autograd.sddmm(t, _OnDevice(torch.zeros(8, m).t()), dev(k, 8)),
               lambda: autograd.sparse_attention(t, dev(m, 8), dev(k, 8), dev(k + 1, 8)),
               lambda: autograd.sparse_attention(t, dev(m, 8), dev(k, 6), dev(k, 8)),
               lambda: autograd.sparse_attention(t, dev(m, 8), dev(k, 8), dev(k, 8, dtype=torch.float64)),
               lambda: autograd.sparse_attention(t, dev(m, 8, dtype=torch.float64), dev(k, 8), dev(k, 8))]
    for i, f in enumerate(bad_ops):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was not refused")
