"""The FAST numerics contract (include/mispmm.h enum mispmm_acc_mode) as something a test can hold a kernel
to: every output element of a single-chain path is

    acc = +0;  acc = fma(a_e, B[col_e][j], acc) for the row's entries e in LIST order;  C[r][j] = acc

with one rounding per step.  oracle.rows_fma is that chain in C (libm fmaf / fma); chain_exact below is the same chain in exact
rational arithmetic and exists only to pin the C functions.  The row list of each format is the one the header gives it: CSR
storage order, COO stable-sorted by row, column-major ELL ascending column then slot with the padding dropped, BSR blocks in
storage order and ascending column inside a block (kernel 1 keeps the explicit zeros, the zero-skipping list drops them).

sharp_values / corpus_is_sharp make the data on which a deviation shows: full mantissas, so nearly every product rounds, and a
measured precondition (on the CPU, with the references alone) that the unfused chain and the reversed chain really do differ
from the contract's chain in a good share of the elements.  any_order_bound is the textbook bound for the paths that promise a
fixed order but not the storage-order chain."""
from fractions import Fraction

import numpy as np

import _ref64

_FORMATS = {np.dtype(np.float32): (24, -126, 127), np.dtype(np.float64): (53, -1022, 1023)}   # precision, emin, emax
UNIT_ROUNDOFF = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
SHARP_SHARE = 0.15


def _oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


# ------------------------------------------------------------------------------------------------ the chain, exactly
def round_fraction(x, dtype):
    """A non-zero Fraction rounded once to `dtype`, round to nearest even, gradual underflow, overflow to infinity.
    Returned as a Python float (exact for both formats)."""
    p, emin, emax = _FORMATS[np.dtype(dtype)]
    sign = -1.0 if x < 0 else 1.0
    ax = -x if x < 0 else x
    e = ax.numerator.bit_length() - ax.denominator.bit_length()       # 2^(e-1) <= ax < 2^(e+1)
    if Fraction(2) ** e > ax:
        e -= 1
    assert Fraction(2) ** e <= ax < Fraction(2) ** (e + 1)
    q = max(e, emin) - (p - 1)                                          # exponent of the last place
    scaled = ax / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    if Fraction(n) * Fraction(2) ** q >= Fraction(2) ** (emax + 1):
        return sign * float("inf")
    return sign * float(Fraction(n) * Fraction(2) ** q)


def fma_exact(a, b, c, dtype):
    """fma(a, b, c) of the IEEE format `dtype`: a * b + c formed exactly, rounded once.  a, b, c are values of that format."""
    dt = np.dtype(dtype).type
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        if np.isfinite(a) and np.isfinite(b):                          # a finite product never moves an Inf or a NaN addend
            return dt(c)
        with np.errstate(invalid="ignore"):                            # no rounding question: the Inf / NaN rules alone decide
            return dt(np.float64(a) * np.float64(b) + np.float64(c))   # the product is +-Inf or NaN here, exactly as in fma
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        # an exact zero sum: the common sign of product and addend if they agree, else +0 (round to nearest)
        prod_neg = (np.signbit(a) != np.signbit(b))
        if Fraction(a) * Fraction(b) == 0 and c == 0 and prod_neg and np.signbit(c):
            return dt(-0.0)
        return dt(0.0)
    return dt(round_fraction(exact, dtype))


def chain_exact(row_ptrs, col_idxs, vals, b):
    """The contract in fractions.Fraction, element by element.  Slow: for a few dozen output elements."""
    vals, b = np.asarray(vals), np.asarray(b)
    assert vals.dtype == b.dtype and vals.dtype in (np.float32, np.float64)
    rp = np.asarray(row_ptrs, dtype=np.int64)
    m, n = rp.shape[0] - 1, b.shape[1]
    out = np.zeros((m, n), dtype=vals.dtype)
    for r in range(m):
        for j in range(n):
            acc = vals.dtype.type(0.0)
            for e in range(rp[r], rp[r + 1]):
                acc = fma_exact(vals[e], b[int(col_idxs[e]), j], acc, vals.dtype)
            out[r, j] = acc
    return out


# ------------------------------------------------------------------------------------------------ other chains (what a wrong kernel computes)
def chain_unfused(row_ptrs, col_idxs, vals, b):
    """Product rounded, then added, in list order from +0 -- in the operands' own dtype (numpy's * and + are single IEEE
    roundings in float32 and float64).  In float32 this is the REFERENCE chain of COO / ELL / BSR."""
    vals, b = np.asarray(vals), np.asarray(b)
    assert vals.dtype == b.dtype and vals.dtype in (np.float32, np.float64)
    rp = np.asarray(row_ptrs, dtype=np.int64)
    cols = np.asarray(col_idxs, dtype=np.int64)
    m, n = rp.shape[0] - 1, b.shape[1]
    out = np.zeros((m, n), dtype=vals.dtype)
    lens = np.diff(rp)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(int(lens.max(initial=0))):
            rows = np.nonzero(lens > t)[0]
            at = rp[rows] + t
            out[rows] = out[rows] + vals[at][:, None] * b[cols[at]]
    return out


def reversed_rows(row_ptrs, col_idxs, vals):
    """The same row list with every row's entries in the opposite order."""
    rp = np.asarray(row_ptrs, dtype=np.int64)
    lens = np.diff(rp)
    row_of = np.repeat(np.arange(lens.shape[0]), lens)
    pos = np.arange(int(rp[-1])) - rp[row_of]
    src = rp[row_of] + lens[row_of] - 1 - pos
    return rp, np.asarray(col_idxs)[src], np.asarray(vals)[src]


# ------------------------------------------------------------------------------------------------ row lists per format
def _typed(rows, dtype):
    rp, cols, vals = rows
    return np.asarray(rp, np.uint32), np.asarray(cols, np.uint32), np.ascontiguousarray(np.asarray(vals).astype(dtype))


def csr_rows(csr, dtype=np.float32):
    return _typed((csr.row_ptrs, csr.col_idxs, csr.data), dtype)


def coo_rows(coo, dtype=np.float32):
    return _typed(_ref64.coo_rows(coo.num_rows, coo.row_idxs, coo.col_idxs, coo.data), dtype)


def ell_colmajor_rows(ell, dtype=np.float32):
    return _typed(_ref64.ell_colmajor_rows(ell.num_rows, ell.num_cols, ell.max_col_nnz, ell.row_idxs, ell.data), dtype)


def ell_rowmajor_rows(ell, dtype=np.float32):
    """A row-major ELL: slot order, padding dropped."""
    cols = np.asarray(ell.col_idxs, np.uint32).reshape(ell.num_rows, -1)
    live = cols != np.uint32(0xFFFFFFFF)
    rp = np.concatenate([[0], np.cumsum(live.sum(axis=1))])
    return _typed((rp, cols[live], np.asarray(ell.data).reshape(ell.num_rows, -1)[live]), dtype)


def bsr_rows(bsr, skip_zeros, dtype=np.float32):
    """skip_zeros=False: what the BSR kernel 1 walks (explicit zeros kept); True: the zero-skipping list."""
    return _typed(_ref64.bsr_rows(bsr.num_rows, bsr.block_row_size, bsr.block_col_size, bsr.block_row_ptrs, bsr.block_col_idxs,
                                  bsr.data, skip_zeros=skip_zeros), dtype)


# ------------------------------------------------------------------------------------------------ data on which deviations show
def sharp_values(rng, shape, dtype):
    """sign * [0.5, 1.5) * 2^e, e in -3..3, every mantissa bit random: products need 48 (106) bits and round, sums of
    neighbours in exponent round again, so fusing, order and the width of a partial sum all reach the last bit."""
    if np.dtype(dtype) == np.float64:
        return _ref64.random_f64(rng, shape)
    assert np.dtype(dtype) == np.float32
    mant = np.minimum((rng.random(shape) + 0.5).astype(np.float32), np.nextafter(np.float32(1.5), np.float32(0)))
    exp = rng.integers(-3, 4, size=shape).astype(np.float32)
    sign = np.where(rng.random(shape) < 0.5, np.float32(-1.0), np.float32(1.0))
    return (sign * mant * np.exp2(exp)).astype(np.float32)            # sign and power of two are exact


def sharpness(row_list, b):
    """(share of elements where the unfused chain differs from the fma chain, the same for the reversed chain, number of
    elements looked at) over the rows of at least two entries.  References only: nothing here runs a kernel."""
    rp, cols, vals = row_list
    orc = _oracle()
    multi = np.diff(np.asarray(rp, np.int64)) >= 2
    count = int(multi.sum()) * b.shape[1]
    if count == 0:
        return 0.0, 0.0, 0
    chain = orc.rows_fma(rp, cols, vals, b)[multi]
    unfused = chain_unfused(rp, cols, vals, b)[multi]
    rrp, rcols, rvals = reversed_rows(rp, cols, vals)
    backwards = orc.rows_fma(rrp, rcols, rvals, b)[multi]
    bits = np.uint32 if chain.dtype == np.float32 else np.uint64
    view = lambda x: np.ascontiguousarray(x).view(bits)                                      # noqa: E731
    return float(np.mean(view(chain) != view(unfused))), float(np.mean(view(chain) != view(backwards))), count


def corpus_is_sharp(row_list, b):
    """The precondition of every bitwise FAST case: on this data an unfused kernel and a kernel that walks a row backwards
    would each differ from the contract in at least SHARP_SHARE of the elements of the rows that have two entries or more.
    A list without such a row discriminates nothing and is not sharp."""
    unfused, backwards, count = sharpness(row_list, b)
    return count > 0 and unfused >= SHARP_SHARE and backwards >= SHARP_SHARE


# ------------------------------------------------------------------------------------------------ the derived bound
def any_order_bound(row_ptrs, abs_scale, dtype=np.float32):
    """gamma_L * sum|a||b| per row of L entries, gamma_L = L u / (1 - L u): the bound on a sum of L fused products in ANY order
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: every term passes at most L roundings).  Derived,
    not measured.  abs_scale: [M, N] float64, sum |a||b| per output element."""
    u = UNIT_ROUNDOFF[np.dtype(dtype)]
    lens = np.diff(np.asarray(row_ptrs, np.int64)).astype(np.float64)
    gamma = lens * u / (1.0 - lens * u)
    return gamma[:, None] * np.asarray(abs_scale, np.float64)


def exact_and_bound(row_list, b):
    """For a float32 list: (the products of the float32 operands -- exact in float64 -- summed in float64 in list order,
    any_order_bound plus that sum's own error L * 2^-53 * sum|a||b|)."""
    rp, cols, vals = row_list
    v64, b64 = np.asarray(vals, np.float64), np.asarray(b, np.float64)
    exact = _ref64.ref_rows(rp, cols, v64, b64)
    scale = _ref64.abs_scale(rp, cols, v64, b64)
    lens = np.diff(np.asarray(rp, np.int64)).astype(np.float64)
    return exact, any_order_bound(rp, scale, np.float32) + (lens * 2.0 ** -53)[:, None] * scale
