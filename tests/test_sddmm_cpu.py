"""SDDMM and the transposed product on a machine WITHOUT a GPU: the host transpose (mispmm_csr_transpose_host) against its
argsort restatement, the oracle's CSR arithmetic on the transposed arrays, the SDDMM entry points' argument validation (which
happens before any device work) and the Python layer's refusal of CPU tensors."""
import ctypes

import numpy as np
import pytest

from mispmm import capi, formats, ops

from _sddmm_ref import dense_of, matrix, small_ints, transpose_ref


def _handmade(name):
    if name == "empty_rows":
        return formats.CSR(5, 7, np.zeros(6, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    if name == "no_rows":
        return formats.CSR(0, 7, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    assert name == "one_entry"
    return formats.CSR(3, 4, np.array([0, 0, 1, 1], np.uint32), np.array([2], np.uint32), np.array([1.5], np.float32))


CASES = ["n4c6-b13", "ragged", "tall", "flat", "unsorted", "no_rows", "empty_rows", "one_entry"]


def _case(name):
    return _handmade(name) if name in ("no_rows", "empty_rows", "one_entry") else matrix(name)


@pytest.mark.parametrize("name", CASES)
def test_transpose_is_the_stable_sort_by_column(name):
    csr = _case(name)
    t, perm = ops.csr_transpose(csr)
    want_ptrs, want_cols, want_perm = transpose_ref(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs)
    assert (t.num_rows, t.num_cols) == (csr.num_cols, csr.num_rows)
    assert perm.dtype == np.uint32 and np.array_equal(perm, want_perm)
    assert np.array_equal(t.row_ptrs, want_ptrs) and np.array_equal(t.col_idxs, want_cols)
    assert np.array_equal(t.data, np.asarray(csr.data)[want_perm.astype(np.int64)])


def test_transpose_cases_cover_what_they_claim():
    tall, flat, uns = matrix("tall"), matrix("flat"), matrix("unsorted")
    assert tall.num_rows > tall.num_cols and flat.num_cols > flat.num_rows
    rp, ci = uns.row_ptrs.astype(np.int64), uns.col_idxs.astype(np.int64)
    rows = [ci[rp[r]:rp[r + 1]] for r in range(uns.num_rows)]
    assert any(len(np.unique(c)) < len(c) for c in rows) and any(np.any(np.diff(c) < 0) for c in rows)
    lens = np.diff(matrix("ragged").row_ptrs.astype(np.int64))
    assert lens[0] == 0 and lens[-1] == 0 and int((lens == 0).sum()) == 280


def test_transpose_rejects_bad_input():
    l = capi.lib()
    rp, ci = np.array([0, 2, 3], np.uint32), np.array([0, 4, 1], np.uint32)
    trp, tci, perm = np.zeros(5, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    call = lambda k, rp_, ci_: l.mispmm_csr_transpose_host(2, k, 3, rp_.ctypes.data, ci_.ctypes.data, trp.ctypes.data,   # noqa: E731
                                                           tci.ctypes.data, perm.ctypes.data)
    assert call(5, rp, ci) == capi.OK
    assert call(4, rp, ci) == capi.ERR_INVALID_ARG                                   # column 4 >= K = 4
    assert b"out of range" in l.mispmm_last_error()
    assert call(5, np.array([0, 3, 2], np.uint32), ci) == capi.ERR_INVALID_ARG       # row pointers decrease
    assert b"decrease" in l.mispmm_last_error()
    assert call(5, np.array([0, 2, 2], np.uint32), ci) == capi.ERR_INVALID_ARG       # do not reach nnz
    assert l.mispmm_csr_transpose_host(2, 5, 3, None, ci.ctypes.data, trp.ctypes.data, tci.ctypes.data, perm.ctypes.data) == capi.ERR_INVALID_ARG
    assert l.mispmm_csr_transpose_host(2, 5, 3, rp.ctypes.data, ci.ctypes.data, None, tci.ctypes.data, perm.ctypes.data) == capi.ERR_INVALID_ARG
    with pytest.raises(capi.MispmmError):
        ops.csr_transpose(formats.CSR(2, 4, rp, ci, np.ones(3, np.float32)))


@pytest.mark.parametrize("name", ["ragged", "unsorted", "long"])
def test_oracle_on_the_transposed_arrays_is_the_transposed_product(name, oracle):
    """Small-integer data: every sum is exact, so the reference's CSR arithmetic on (tRowPtrs, tColIdxs, vals[perm]) must
    give A^T B to the bit -- repeated (row, column) pairs of A included."""
    rng = np.random.default_rng(21)
    csr = matrix(name)
    csr = formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, small_ints(rng, csr.nnz, np.float32))
    t, _ = ops.csr_transpose(csr)
    g = small_ints(rng, (csr.num_rows, 5), np.float32)
    got = oracle.spmm_csr(t.row_ptrs, t.col_idxs, t.data, g)
    want = (dense_of(csr).T @ g.astype(np.float64)).astype(np.float32)
    assert got.shape == (csr.num_cols, 5)
    assert np.array_equal(got.view(np.uint32), (want + np.float32(0)).view(np.uint32))


@pytest.mark.parametrize("fn", ["mispmm_sddmm_csr_f32", "mispmm_sddmm_csr_f64"])
def test_sddmm_validates_before_any_device_work(fn):
    l = capi.lib()
    call = getattr(l, fn)
    one = ctypes.c_void_p(16)   # never dereferenced: every call below must return from validation
    elem = 4 if fn.endswith("f32") else 8
    #           stream M  K  nnz rowPtrs colIdxs X   ldx  Y   ldy  N  out  acc
    assert call(None, 4, 4, 1, None, one, one, 8, one, 8, 8, one, 0) == capi.ERR_INVALID_ARG
    assert call(None, 4, 4, 1, one, None, one, 8, one, 8, 8, one, 0) == capi.ERR_INVALID_ARG
    assert call(None, 4, 4, 1, one, one, None, 8, one, 8, 8, one, 0) == capi.ERR_INVALID_ARG
    assert call(None, 4, 4, 1, one, one, one, 8, None, 8, 8, one, 0) == capi.ERR_INVALID_ARG
    assert call(None, 4, 4, 1, one, one, one, 8, one, 8, 8, None, 0) == capi.ERR_INVALID_ARG
    assert b"null" in l.mispmm_last_error()
    assert call(None, 4, 4, 1, one, one, one, 7, one, 8, 8, one, 0) == capi.ERR_INVALID_ARG        # ldx < N
    assert call(None, 4, 4, 1, one, one, one, 8, one, 7, 8, one, 1) == capi.ERR_INVALID_ARG        # ldy < N
    assert b"leading dimension" in l.mispmm_last_error()
    assert call(None, 4, 4, 1, one, one, one, 8, one, 8, 8, one, 7) == capi.ERR_INVALID_ARG        # accumulate mode
    big = (1 << 31) // (4 * elem)                                                                  # K * ldy * elem = 2 GiB
    assert call(None, 4, 4, 1, one, one, one, 8, one, big, 8, one, 0) == capi.ERR_UNSUPPORTED
    assert call(None, 4, 4, 1, one, one, one, big, one, 8, 8, one, 1) == capi.ERR_UNSUPPORTED
    assert b"2 GiB" in l.mispmm_last_error()
    assert call(None, 4, 4, 0, one, None, one, 8, one, 8, 8, None, 0) == capi.OK                    # nnz == 0: a no-op
    assert call(None, 0, 4, 0, None, None, None, 8, None, 8, 8, None, 1) == capi.OK                 # M == 0


def test_python_layer_without_a_gpu():
    torch = pytest.importorskip("torch")
    from mispmm import autograd                      # imports without a GPU
    csr = matrix("unsorted")
    a = ops.DeviceCSR.from_host(csr, device="cpu")
    x, y = torch.zeros(csr.num_rows, 8), torch.zeros(csr.num_cols, 8)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.sddmm_csr(a, x, y)
    for dtype in (torch.float32, torch.float64):
        t = autograd.TrainableCSR.from_host(csr, device="cpu", dtype=dtype)
        assert t.perm.dtype == torch.int64 and t.values.dtype == dtype and t.fwd.plan is None and t.tpattern.plan is None
        assert (t.tpattern.num_rows, t.tpattern.num_cols) == (csr.num_cols, csr.num_rows)
        with pytest.raises(ValueError, match="no CPU path"):
            autograd.spmm(t, t.values, torch.zeros(csr.num_cols, 8, dtype=dtype))
