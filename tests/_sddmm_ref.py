"""The SDDMM contract (include/mispmm.h, section "SDDMM on a CSR pattern") restated in numpy, the error bounds it states,
the transpose contract (mispmm_csr_transpose_host) restated with argsort, and the small matrices the tests share.

    out[e] = sum_j X[row(e)][j] * Y[col(e)][j]          for every stored entry e of A, A's values unread

`exact` below is that sum in the widest float numpy has (x87 extended where the platform has it: 64-bit mantissas, so its own
error, N 2^-64 S, is far below every bound; plain float64 elsewhere, which the bounds' factor 2 absorbs) and S = sum |x||y|."""
import functools

import numpy as np

from mispmm import datasets, formats


def entry_rows(row_ptrs):
    rp = np.asarray(row_ptrs, dtype=np.int64)
    return np.repeat(np.arange(rp.shape[0] - 1), np.diff(rp))


def sddmm_exact(row_ptrs, col_idxs, x, y):
    """(exact, S) per entry, float64 arrays of nnz elements."""
    rows, cols = entry_rows(row_ptrs), np.asarray(col_idxs, dtype=np.int64)
    xl, yl = np.asarray(x, dtype=np.longdouble), np.asarray(y, dtype=np.longdouble)
    exact, scale = np.zeros(rows.shape[0], np.longdouble), np.zeros(rows.shape[0], np.longdouble)
    step = max(1, (1 << 22) // max(1, xl.shape[1]))       # a few million products at a time
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, rows.shape[0], step):
            p = xl[rows[s:s + step]] * yl[cols[s:s + step]]
            exact[s:s + step] = p.sum(axis=1)
            scale[s:s + step] = np.abs(p).sum(axis=1)
        return exact.astype(np.float64), scale.astype(np.float64)


def sddmm_f64(row_ptrs, col_idxs, x, y):
    """The plain float64 restatement (what decides where a NaN or an Inf belongs)."""
    rows, cols = entry_rows(row_ptrs), np.asarray(col_idxs, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(x, np.float64)[rows] * np.asarray(y, np.float64)[cols]).sum(axis=1)


def bound(dtype, acc, n, exact, scale):
    """The header's bound on |out - exact| for (dtype, accumulate mode, N)."""
    if np.dtype(dtype) == np.float64:
        return 2.0 * n * 2.0 ** -53 * scale
    if acc == "reference":
        return 2.0 ** -24 * np.abs(exact) + n * 2.0 ** -52 * scale
    u = n * 2.0 ** -24
    return u / (1.0 - u) * scale


def assert_within(got, dtype, acc, n, exact, scale, what=""):
    got = np.asarray(got, dtype=np.float64)
    err, lim = np.abs(got - exact), bound(dtype, acc, n, exact, scale)
    worst = float(np.max(err / np.where(lim > 0, lim, 1.0), initial=0.0))
    print(f"{what}: max |out - exact| / bound = {worst:.3g}")
    bad = ~(err <= lim)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries outside the bound, worst {worst:.3g} x at {np.argwhere(bad)[:4].ravel().tolist()}"


def full_mantissa(rng, shape, dtype):
    """Random signs, magnitudes in [0.5, 2) with random low bits: every product rounds, nothing underflows."""
    v = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, shape)
    return v.astype(dtype)


def small_ints(rng, shape, dtype):
    return rng.integers(-8, 9, shape).astype(dtype)


# ---- the transpose contract
def transpose_ref(num_rows, num_cols, row_ptrs, col_idxs):
    cols = np.asarray(col_idxs, dtype=np.int64)
    perm = np.argsort(cols, kind="stable")
    t_cols = entry_rows(row_ptrs)[perm]
    t_ptrs = np.searchsorted(cols[perm], np.arange(num_cols + 1))
    return t_ptrs.astype(np.uint32), t_cols.astype(np.uint32), perm.astype(np.uint32)


def dense_of(csr, dtype=np.float64):
    """A as a dense array, repeated (row, column) pairs ADDED (formats.CSR.to_dense keeps the last)."""
    d = np.zeros((csr.num_rows, csr.num_cols), dtype=dtype)
    np.add.at(d, (entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)), np.asarray(csr.data, dtype=dtype))
    return d


# ---- matrices
def _csr(m, k, lens, rng, sort=True, replace=False):
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    pick = [rng.choice(k, size=int(n), replace=replace) for n in lens]
    cols = np.concatenate([np.sort(c) if sort else c for c in pick] or [np.zeros(0, np.int64)]).astype(np.uint32)
    return formats.CSR(m, k, ptr, cols, rng.uniform(-1, 1, int(ptr[-1])).astype(np.float32))


@functools.lru_cache(maxsize=None)
def matrix(name):
    """qh1484 | ragged (700 x 900, 40 % empty rows, first and last among them) | long (96 x 400, rows of 300, 129, 77 and 40
    entries among rows of 0-9) | unsorted (50 x 70, columns unsorted and repeated inside a row) | tall (300 x 40) | flat
    (40 x 300) | n4c6-b13.  Treat the result as read-only."""
    rng = np.random.default_rng({"ragged": 11, "long": 4, "unsorted": 12, "tall": 13, "flat": 14}.get(name, 0))
    if name == "ragged":
        lens = rng.integers(1, 30, 700)
        empty = rng.choice(np.arange(1, 699), size=278, replace=False)
        lens[empty] = 0
        lens[[0, 699]] = 0
        return _csr(700, 900, lens, rng)
    if name == "long":
        lens = rng.integers(0, 10, 96)
        lens[[3, 40, 41, 90]] = [300, 40, 129, 77]
        return _csr(96, 400, lens, rng)
    if name == "unsorted":
        return _csr(50, 70, rng.integers(0, 24, 50), rng, sort=False, replace=True)
    if name == "tall":
        return _csr(300, 40, rng.integers(0, 6, 300), rng)
    if name == "flat":
        return _csr(40, 300, rng.integers(0, 40, 40), rng)
    return datasets.load_csr(name)
