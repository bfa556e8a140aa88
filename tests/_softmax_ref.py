"""The row-softmax contract (include/mispmm.h, section "Row softmax on a CSR pattern") restated in numpy, the error bounds it
states, the score generators and the `edges` matrices the tests share.

    out[e] = exp(s[e] - m_r) / sum_{e' in row r} exp(s[e'] - m_r)            m_r the largest score of row r
    ds[e]  = p[e] * (dp[e] - sum_{e' in row r} p[e'] * dp[e'])

`exact` below is computed in the widest float numpy has (x87 extended where the platform has it: 64-bit mantissas, its own
error of a few 2^-64 per operation far below every bound; plain float64 elsewhere).  Every function is vectorised over the
entries: a row's reduction is a ufunc.reduceat over the starts of the non-empty rows."""
import functools

import numpy as np

from mispmm import formats

from _sddmm_ref import entry_rows, matrix as sddmm_matrix

LD = np.longdouble
REGS = 4                         # entries per lane the kernel keeps in registers: a row of up to REGS * G entries is one pass
GROUPS = (4, 8, 16, 32, 64)      # lanes per row the host can pick


def _segments(row_ptrs):
    """(rows, starts, slot): the row of every entry, the first entry of every non-empty row, and for every entry the index
    of its row among the non-empty ones."""
    rp = np.asarray(row_ptrs, dtype=np.int64)
    lens = np.diff(rp)
    rows = np.repeat(np.arange(lens.shape[0]), lens)
    slot = (np.cumsum(lens > 0) - 1)[rows]
    return rows, rp[:-1][lens > 0], slot


def row_lengths(row_ptrs):
    """L per entry."""
    rp = np.asarray(row_ptrs, dtype=np.int64)
    return np.diff(rp)[entry_rows(rp)]


def _reduce(ufunc, v, starts, slot):
    return ufunc.reduceat(v, starts)[slot] if v.shape[0] else v


def softmax_rows(row_ptrs, scores, dtype=LD):
    """The contract in `dtype` arithmetic, special values included: np.maximum hands a NaN on, Inf - Inf and -Inf - -Inf are
    NaN, and a NaN term makes its row's sum NaN."""
    _, starts, slot = _segments(row_ptrs)
    s = np.asarray(scores).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(s - _reduce(np.maximum, s, starts, slot))
        return e / _reduce(np.add, e, starts, slot)


def spread(row_ptrs, scores):
    """T per entry: the largest |s - m_r| over the finite scores of the entry's row."""
    _, starts, slot = _segments(row_ptrs)
    s = np.asarray(scores, dtype=np.float64)
    hi = _reduce(np.maximum, np.where(np.isfinite(s), s, -np.inf), starts, slot)
    lo = _reduce(np.minimum, np.where(np.isfinite(s), s, np.inf), starts, slot)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(hi) & np.isfinite(lo), hi - lo, 0.0)


def softmax_bwd_rows(row_ptrs, p, dp, dtype=LD):
    """(ds, S) per entry, S = sum over the row of |p||dp|."""
    _, starts, slot = _segments(row_ptrs)
    pl, dl = np.asarray(p).astype(dtype), np.asarray(dp).astype(dtype)
    dot = _reduce(np.add, pl * dl, starts, slot)
    return pl * (dl - dot), _reduce(np.add, np.abs(pl * dl), starts, slot)


def tiny(dtype):
    return 2.0 ** -149 if np.dtype(dtype) == np.float32 else 2.0 ** -1074


def fwd_bound(dtype, acc, length, t, exact):
    """The header's bound on |out - exact|."""
    exact = np.asarray(exact, dtype=np.float64)
    wide = (length + 2.0 * t + 8.0) * 2.0 ** -52 * exact + 2.0 * tiny(dtype)
    if np.dtype(dtype) == np.float64:
        return wide
    if acc == "reference":
        return 2.0 ** -24 * exact + wide
    return (length + 8.0 * t + 16.0) * 2.0 ** -24 * exact + 2.0 ** -126


def bwd_bound(dtype, acc, length, p, dp, s, exact):
    """The header's bound on |ds - exact|."""
    scale = np.abs(np.asarray(p, np.float64)) * (np.abs(np.asarray(dp, np.float64)) + np.asarray(s, np.float64))
    wide = (length + 4.0) * 2.0 ** -52 * scale
    if np.dtype(dtype) == np.float64:
        return wide + (length + 2.0) * tiny(dtype)
    if acc == "reference":
        return 2.0 ** -24 * np.abs(np.asarray(exact, np.float64)) + wide + tiny(dtype)
    u = (length + 4.0) * 2.0 ** -24
    return u / (1.0 - u) * scale + (length + 2.0) * 2.0 ** -126


def assert_inside(got, exact, lim, what=""):
    got, exact, lim = np.asarray(got).astype(LD), np.asarray(exact).astype(LD), np.asarray(lim).astype(LD)
    err = np.abs(got - exact)
    worst = float(np.max(err / np.where(lim > 0, lim, 1.0), initial=0.0))
    print(f"{what}: max |err| / bound = {worst:.3g}")
    bad = ~(err <= lim)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries outside the bound, worst {worst:.3g} x at {np.argwhere(bad)[:4].ravel().tolist()}"
    return worst


def row_sums(row_ptrs, out):
    """(sum of every non-empty row in the widest float, its length)."""
    rp = np.asarray(row_ptrs, dtype=np.int64)
    lens = np.diff(rp)
    starts = rp[:-1][lens > 0]
    v = np.asarray(out).astype(LD)
    return (np.add.reduceat(v, starts) if v.shape[0] else v), lens[lens > 0]


# ---- scores
def scores(kind, nnz, dtype, seed=0):
    """narrow: uniform in [-4, 4), full mantissa.  wide: uniform in [-60, 60), T up to ~120: in fp32 the small terms of a row go
    subnormal or to zero.  equal: one value everywhere."""
    rng = np.random.default_rng(7000 + seed)
    if kind == "narrow":
        return rng.uniform(-4.0, 4.0, nnz).astype(dtype)
    if kind == "wide":
        return rng.uniform(-60.0, 60.0, nnz).astype(dtype)
    assert kind == "equal"
    return np.full(nnz, 0.7, dtype=dtype)


def full_mantissa(rng, shape, dtype):
    v = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, shape)
    return v.astype(dtype)


# ---- matrices
EDGE_LENGTHS = ([0, 0, 1, 2, 3, 4, 5, 0, 7, 8, 9, 15, 16, 17, 31, 32, 33, 0, 0, 63, 64, 65, 127, 128, 129, 255, 256, 257]
                + [300, 1025, 1, 0])
# G - 1, G, G + 1 for every group size; REGS * G and REGS * G + 1 for every register capacity (16 .. 256); 0 and 1; 300, 1025
EDGE_PADDING = {4: [0] * 150, 8: [0] * 68, 16: [0] * 28, 32: [], 64: [1025] * 3}   # rows appended so that the host picks G


def picked_group(num_rows, nnz):
    """The host's choice restated: the smallest G whose registers hold the mean row."""
    mean = -(-nnz // num_rows)
    return next((g for g in GROUPS if g * REGS >= mean), 64)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """edges (the row lengths above; the host picks G = 32) | edges-g4 ... edges-g64 (the same rows, padded with empty rows or
    long ones so that the host picks that G) | any name of _sddmm_ref.matrix.  Treat the result as read-only."""
    if not name.startswith("edges"):
        return sddmm_matrix(name)
    g = int(name.split("-g")[1]) if "-g" in name else 32
    lens = np.array(EDGE_LENGTHS + EDGE_PADDING[g], dtype=np.int64)
    rng = np.random.default_rng(15)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cols = np.concatenate([np.sort(rng.choice(1100, size=int(n), replace=False)) for n in lens]).astype(np.uint32)
    return formats.CSR(lens.shape[0], 1100, ptr, cols, rng.uniform(-1, 1, int(ptr[-1])).astype(np.float32))


EDGE_MATRICES = ["edges"] + [f"edges-g{g}" for g in GROUPS]
