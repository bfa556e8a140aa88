"""The block SDDMM contract (include/mispmm.h, section "SDDMM on a BSR pattern, bf16") restated in numpy, the error bounds it
states, bf16 operand makers and the block patterns the tests share.

    out[e][i][j] = sum_n X[R * bS + i][n] * Y[c * bS + j][n]     for every stored block e of block row R, c = blockColIdxs[e]

`exact` is that sum of the bf16 operands' products in the widest float numpy has (np.longdouble; its own error, N 2^-64 S where
the platform has x87 extended, is far below every bound) and S = sum |x||y|.  On integer operands float64 matmul is exact too."""
import functools

import numpy as np

from mispmm import datasets, formats, synth


def block_rows(bsr):
    ptrs = np.asarray(bsr.block_row_ptrs, dtype=np.int64)
    return np.repeat(np.arange(ptrs.shape[0] - 1), np.diff(ptrs))


def _panels(bsr, x, y, lo, hi, dtype):
    """The X and Y row panels of blocks lo .. hi - 1: two [hi - lo, bS, N] arrays."""
    bs = bsr.block_row_size
    rows, cols = block_rows(bsr)[lo:hi], np.asarray(bsr.block_col_idxs, dtype=np.int64)[lo:hi]
    within = np.arange(bs)
    return (np.asarray(x, dtype=dtype)[rows[:, None] * bs + within], np.asarray(y, dtype=dtype)[cols[:, None] * bs + within])


def sddmm_bsr_exact(bsr, x, y, dtype=np.longdouble):
    """(exact, S) per block element, float64 arrays [num_blocks, bS, bS].  dtype=np.float64 takes batched matmul: exact on
    integer operands, and seconds on a large pattern."""
    nb, bs = bsr.num_blocks, bsr.block_row_size
    exact, scale = np.zeros((nb, bs, bs), np.float64), np.zeros((nb, bs, bs), np.float64)
    step = 2048 if np.dtype(dtype) == np.float64 else 8
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, nb, step):
            xp, yp = _panels(bsr, x, y, lo, min(nb, lo + step), dtype)
            if np.dtype(dtype) == np.float64:
                exact[lo:lo + step] = np.matmul(xp, yp.transpose(0, 2, 1))
                scale[lo:lo + step] = np.matmul(np.abs(xp), np.abs(yp).transpose(0, 2, 1))
            else:
                p = xp[:, :, None, :] * yp[:, None, :, :]
                exact[lo:lo + step] = p.sum(axis=-1)
                scale[lo:lo + step] = np.abs(p).sum(axis=-1)
    return exact, scale


def bound(out_bf16, n, exact, scale):
    """The header's bound on |out - exact|: u = 2^-23 per add, g = N u / (1 - N u)."""
    u = n * 2.0 ** -23
    g = u / (1.0 - u)
    return 2.0 ** -8 * np.abs(exact) + (1.0 + 2.0 ** -8) * g * scale if out_bf16 else g * scale


def assert_within(got, out_bf16, n, exact, scale, what=""):
    got = np.asarray(got, dtype=np.float64)
    err, lim = np.abs(got - exact), bound(out_bf16, n, exact, scale)
    worst = float(np.max(err / np.where(lim > 0, lim, 1.0), initial=0.0))
    print(f"{what}: max |out - exact| / bound = {worst:.3g}")
    bad = ~(err <= lim)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound, worst {worst:.3g} x at {np.argwhere(bad)[:4].tolist()}"


# ---- bf16 operands: float32 arrays whose values are bf16 numbers, and their bit patterns
def full_mantissa(rng, shape):
    """Random signs, magnitudes in [0.5, 2) rounded to bf16: all 8 significant bits in use, nothing underflows."""
    v = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, shape)
    return synth.bf16_round(v.astype(np.float32))


def wide_exponent(rng, shape, spread=8):
    """Random signs, 8-bit mantissas, exponents uniform in [-spread, spread]: unlike full_mantissa (whose sums of up to a few
    hundred products are all exactly representable in fp32) this makes the fp32 accumulate round."""
    v = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * rng.uniform(1.0, 2.0, shape) * 2.0 ** rng.integers(-spread, spread + 1, shape)
    return synth.bf16_round(v.astype(np.float32))


def small_ints(rng, shape, most=8):
    """Integers in [-most, most]: bf16 numbers; with most = 8 and N <= 264 every sum is below 2^15, exact in fp32 in any order."""
    return rng.integers(-most, most + 1, shape).astype(np.float32)


def to_bits(v):
    """float32 array of bf16 numbers -> int16 array of bf16 bits."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any(), "not bf16 numbers"
    return (u >> np.uint32(16)).astype(np.uint16).view(np.int16)


def from_bits(b):
    return (np.ascontiguousarray(b).view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


# ---- patterns
def _pattern(bs, nbr, nbc, counts, unsorted_rows, seed):
    rng = np.random.default_rng(seed)
    cols = []
    for r, k in enumerate(counts):
        pick = rng.choice(nbc, size=k, replace=False)
        if r in unsorted_rows:
            while k > 1 and np.all(np.diff(pick) > 0):
                pick = rng.permutation(pick)
        else:
            pick = np.sort(pick)
        cols.append(pick)
    ptrs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    nb = int(ptrs[-1])
    data = small_ints(rng, (nb, bs, bs), most=4)
    return formats.BSR(nbr * bs, nbc * bs, nb * bs * bs, bs, bs, ptrs, np.concatenate(cols).astype(np.uint32), data)


RAGGED16_COUNTS = [3, 0, 1, 7, 0, 5, 2, 4, 0]
RAGGED32_COUNTS = [2, 0, 4, 1, 3]


@functools.lru_cache(maxsize=None)
def pattern(name):
    """ragged16 (16 x 16 blocks, 9 x 7 block rows x columns, RAGGED16_COUNTS blocks per row: empty rows, the last among them,
    rows of more blocks than a workgroup has waves; block columns not ascending in rows 3 and 5) | ragged32 (32 x 32, 5 x 4,
    RAGGED32_COUNTS; row 2 not ascending) | ACTIVSg10K (16 x 16, formats.csr_to_bsr).  Integer values in [-4, 4] in the small
    ones.  Treat the result as read-only."""
    if name == "ragged16":
        return _pattern(16, 9, 7, RAGGED16_COUNTS, (3, 5), 51)
    if name == "ragged32":
        return _pattern(32, 5, 4, RAGGED32_COUNTS, (2,), 52)
    assert name == "ACTIVSg10K"
    return formats.csr_to_bsr(datasets.load_csr("ACTIVSg10K"), 16)
