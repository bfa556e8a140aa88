"""The fp64 numerics contract (include/mispmm.h) restated in numpy: every output element is

    C[r][j] = (((+0 + p1) + p2) + ...) + pL,   p = a * b rounded once to fp64, every + rounded once, no FMA,

in the order the reference adds the row's entries (the row list: CSR storage order, COO stable-sorted by row, ELL ascending
column then slot, BSR blocks in storage order and ascending column inside a block).  numpy's float64 `*` and `+` are single
IEEE roundings, and both forms below add strictly in list order.  The leading +0 matters: p1 alone keeps a -0 that +0 + p1
does not."""
import numpy as np


def _f64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    assert x.dtype == np.float64, f"expected float64, got {x.dtype}"
    return x


def ref_rows_accumulate(row_ptrs, col_idxs, vals, b):
    """The contract literally, row by row: the row's products with a +0 row prepended, np.add.accumulate (sequential) along
    the entries, last partial sum.  Slow; for small matrices and for pinning ref_rows."""
    b = np.asarray(b, dtype=np.float64)
    rp = np.asarray(row_ptrs, dtype=np.int64)
    m, n = rp.shape[0] - 1, b.shape[1]
    out = np.zeros((m, n), dtype=np.float64)
    for r in range(m):
        s, e = rp[r], rp[r + 1]
        prods = np.asarray(vals[s:e], dtype=np.float64)[:, None] * b[np.asarray(col_idxs[s:e], dtype=np.int64)]
        out[r] = np.add.accumulate(np.vstack([np.zeros((1, n)), prods]), axis=0)[-1]
    return out


def ref_rows(row_ptrs, col_idxs, vals, b):
    """Same bits as ref_rows_accumulate, vectorised over rows: slot t of every row that has one is added in step t, so each
    row still adds its entries one by one in list order, starting from +0."""
    b = np.asarray(b, dtype=np.float64)
    rp = np.asarray(row_ptrs, dtype=np.int64)
    cols = np.asarray(col_idxs, dtype=np.int64)
    va = np.asarray(vals, dtype=np.float64)
    m, n = rp.shape[0] - 1, b.shape[1]
    out = np.zeros((m, n), dtype=np.float64)
    lens = np.diff(rp)
    with np.errstate(invalid="ignore", over="ignore"):    # Inf - Inf and 0 * Inf are part of the contract
        for t in range(int(lens.max(initial=0))):
            rows = np.nonzero(lens > t)[0]
            at = rp[rows] + t
            out[rows] = out[rows] + va[at][:, None] * b[cols[at]]
    return out


def coo_rows(num_rows, row_idxs, col_idxs, vals):
    """A COO as the row list of its stable sort by row."""
    order = np.argsort(np.asarray(row_idxs), kind="stable")
    rows = np.asarray(row_idxs)[order]
    rp = np.searchsorted(rows, np.arange(num_rows + 1)).astype(np.int64)
    return rp, np.asarray(col_idxs)[order], np.asarray(vals, dtype=np.float64)[order]


def ell_colmajor_rows(num_rows, num_cols, max_col_nnz, row_idxs, vals):
    """A column-major ELL as the row list spmmELLCpu adds: column by column, slot by slot, padding (row index < 0) skipped."""
    ri = np.asarray(row_idxs, dtype=np.uint32).reshape(num_cols, max_col_nnz).astype(np.int64)
    va = np.asarray(vals, dtype=np.float64).reshape(num_cols, max_col_nnz)
    cols = np.repeat(np.arange(num_cols), max_col_nnz).reshape(num_cols, max_col_nnz)
    live = ri < 0x80000000                            # int32(row) >= 0, as `if (row >= 0)` in spmmELLCpu
    r, c, v = ri[live], cols[live], va[live]          # column-major walk order
    order = np.argsort(r, kind="stable")
    rp = np.searchsorted(r[order], np.arange(num_rows + 1)).astype(np.int64)
    return rp, c[order], v[order]


def bsr_rows(num_rows, bR, bC, block_row_ptrs, block_col_idxs, blocks, skip_zeros=True):
    """A BSR as the row list spmmBSRCpu adds: per C row, blocks in storage order, ascending column inside a block.
    skip_zeros: drop the explicit zeros (the zero-skipping list; identical sums unless a zero meets an Inf or NaN of B)."""
    blocks = np.asarray(blocks, dtype=np.float64).reshape(-1, bR, bC)
    rp, cols, vals = [0], [], []
    for br in range(num_rows // bR):
        for i in range(bR):
            for k in range(int(block_row_ptrs[br]), int(block_row_ptrs[br + 1])):
                for j in range(bC):
                    v = blocks[k, i, j]
                    if skip_zeros and v == 0.0:
                        continue
                    cols.append(int(block_col_idxs[k]) * bC + j)
                    vals.append(v)
            rp.append(len(cols))
    return np.asarray(rp, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float64)


def assert_same_bits64(got, want, what=""):
    """uint64 patterns equal wherever `want` is not a NaN (so -0.0 != +0.0), and a NaN wherever it is."""
    got, want = _f64(got), _f64(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    nan = np.isnan(want)
    missing = nan & ~np.isnan(got)
    gb, wb = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    bad = ~nan & (gb != wb)
    if missing.any() or bad.any():
        at = np.argwhere(missing | bad)[:4]
        desc = ", ".join(f"{tuple(int(i) for i in ix)}: got {got[tuple(ix)]!r} (0x{int(gb[tuple(ix)]):016x}) "
                         f"want {want[tuple(ix)]!r} (0x{int(wb[tuple(ix)]):016x})" for ix in at)
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ in their bits, {int(missing.sum())} NaNs missing; {desc}")


def abs_scale(row_ptrs, col_idxs, vals, b):
    """sum |a||b| per output element (the FAST bound's scale), computed in the same list form."""
    with np.errstate(invalid="ignore", over="ignore"):
        return ref_rows(row_ptrs, col_idxs, np.abs(np.asarray(vals, np.float64)), np.abs(np.asarray(b, np.float64)))


def random_f64(rng, shape, lo_exp=-3, hi_exp=3):
    """Full 53-bit mantissas with random signs and exponents: their products round, so an FMA, a contracted mul + add or a
    stray fp32 step cannot pass unseen."""
    mant = rng.random(shape) + 0.5                      # [0.5, 1.5): random low bits everywhere
    exp = rng.integers(lo_exp, hi_exp + 1, size=shape).astype(np.float64)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return sign * mant * np.exp2(exp)
