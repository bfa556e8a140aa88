"""The block row-softmax contract (include/mispmm.h, section "Row softmax on a BSR pattern") restated in numpy, the error bounds
it states, the patterns, masks and operands the tests share.

    z[e][i][j]   = fl32(scale * s[e][i][j] + mask[e][i][j])           one fp32 fma; without a mask the fp32 product
    out[e][i][j] = exp(z - m) / sum_row exp(z - m)                     m the largest z of matrix row R * bS + i
    ds[e][i][j]  = scale * p * (dp - sum_row p * dp)

Matrix row R * bS + i owns element row i of every block of block row R.  `layout(name)` lists every matrix row's elements one
after the other, which turns a block array into the entry array of a CSR whose rows are the matrix rows: the row-wise
restatements of tests/_softmax_ref.py (widest float numpy has) then apply as they are."""
import functools
import os

import numpy as np

from mispmm import formats, synth

from _sddmm_bsr_ref import _pattern, pattern as sddmm_bsr_pattern
from _softmax_ref import LD, softmax_bwd_rows, softmax_rows, spread

HELD = {16: 32, 32: 16}          # C: the blocks of a block row the kernel holds in registers (kHeld in csrc/softmax_bsr.hip)
EDGE_UNSORTED = (5, 9)


def edge_counts(bs):
    c = HELD[bs]
    return [0, 1, 2, 3, 4, 5, 8, 9, c - 1, c, c + 1, 2 * c + 1, 0]


@functools.lru_cache(maxsize=None)
def pattern(name):
    """edges16 | edges32 (blocks per block row: edge_counts -- either side of the waves of a workgroup, of a wave's held
    blocks and of C, more than two walks' worth, empty rows first and last; block rows 5 and 9 not ascending) |
    ragged16 | ragged32 of _sddmm_bsr_ref.pattern | ACTIVSg10K (16 x 16: the block index of tests/golden, no values -- none
    are read).  Treat the result as read-only."""
    if name == "ACTIVSg10K":
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ACTIVSg10K_bsr16_index.npz"))
        rows, cols, nnz, br, bc, _ = (int(x) for x in z["header"])
        return formats.BSR(rows, cols, nnz, br, bc, z["block_row_ptrs"], z["block_col_idxs"], np.zeros((0, br, bc), np.float32))
    if name.startswith("edges"):
        bs = int(name[len("edges"):])
        counts = edge_counts(bs)
        return _pattern(bs, len(counts), 2 * HELD[bs] + 3, counts, EDGE_UNSORTED, 53 + bs)
    return sddmm_bsr_pattern(name)


@functools.lru_cache(maxsize=None)
def layout(name):
    """(row_ptrs, idx): matrix row r owns the elements idx[row_ptrs[r] : row_ptrs[r + 1]] of the flat block array, in storage
    order (block by block, left to right)."""
    bsr = pattern(name)
    bs = bsr.block_row_size
    ptrs = np.asarray(bsr.block_row_ptrs, dtype=np.int64)
    counts = np.diff(ptrs)
    row_ptrs = np.concatenate([[0], np.cumsum(np.repeat(counts * bs, bs))])
    within = np.arange(bs, dtype=np.int64)
    pieces = []
    for lo, hi in zip(ptrs[:-1], ptrs[1:]):
        e = np.arange(lo, hi, dtype=np.int64)
        at = e[None, :, None] * (bs * bs) + within[:, None, None] * bs + within[None, None, :]      # [i][block][j]
        pieces.append(at.reshape(-1))
    idx = np.concatenate(pieces) if pieces else np.zeros(0, np.int64)
    return row_ptrs, idx


def to_rows(name, blocks):
    return np.asarray(blocks).reshape(-1)[layout(name)[1]]


def from_rows(name, v):
    bsr = pattern(name)
    out = np.empty(bsr.num_blocks * bsr.block_row_size ** 2, dtype=v.dtype)
    out[layout(name)[1]] = v
    return out.reshape(bsr.num_blocks, bsr.block_row_size, bsr.block_row_size)


def lengths(name):
    """L per element."""
    bsr = pattern(name)
    counts = np.diff(np.asarray(bsr.block_row_ptrs, dtype=np.int64))
    return np.broadcast_to((np.repeat(counts, counts) * bsr.block_row_size)[:, None, None],
                           (bsr.num_blocks, bsr.block_row_size, bsr.block_row_size))


# ---- the fma that forms z
def fma32(a, b, c):
    """fl32(a * b + c), one rounding, element-wise on float32 arrays.  In float64 the product is exact; the sum is rounded to
    53 bits TO ODD (the rounded sum, moved to its odd neighbour on the side of the two-sum error when it is even and not
    exact), and a value rounded to odd with two bits or more to spare rounds to float32 as the exact value does."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)                    # two-sum: p + c = s + err exactly
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def z_values(scores, mask, scale):
    s = np.asarray(scores, dtype=np.float32)
    if mask is None:
        with np.errstate(invalid="ignore", over="ignore"):
            return np.float32(scale) * s
    return fma32(np.float32(scale), s, mask)


# ---- the contract
def forward(name, z, dtype=LD):
    """(softmax per matrix row in `dtype`, T per element) on the fp32 values z."""
    row_ptrs, _ = layout(name)
    zr = to_rows(name, z)
    return from_rows(name, softmax_rows(row_ptrs, zr, dtype)), from_rows(name, spread(row_ptrs, zr))


def backward(name, p, dp, scale, dtype=LD):
    """(ds, S) per element on the given p, dp and the fp32 scale; S = sum over the row of |p||dp|."""
    row_ptrs, _ = layout(name)
    ds, cap = softmax_bwd_rows(row_ptrs, to_rows(name, p), to_rows(name, dp), dtype)
    return from_rows(name, np.asarray(np.float32(scale)).astype(dtype) * ds), from_rows(name, cap)


def forward_f32(name, z):
    """The forward in plain numpy float32: difference, exp, a left-to-right sum, division, each rounded to float32."""
    return forward(name, z, np.float32)[0]


def backward_f32(name, p, dp, scale):
    return backward(name, np.asarray(p, np.float32), np.asarray(dp, np.float32), scale, np.float32)[0]


def row_sums(name, out):
    """(sum of every non-empty matrix row in the widest float, its length)."""
    row_ptrs, _ = layout(name)
    lens = np.diff(row_ptrs)
    v = to_rows(name, out).astype(LD)
    return (np.add.reduceat(v, row_ptrs[:-1][lens > 0]) if v.shape[0] else v), lens[lens > 0]


# ---- the bounds of the header
def fwd_bound(out_bf16, length, t, exact):
    exact = np.asarray(exact, dtype=np.float64)
    f32 = (length + 8.0 * t + 16.0) * 2.0 ** -24 * exact + 2.0 ** -126
    return 2.0 ** -8 * exact + (1.0 + 2.0 ** -8) * f32 + 2.0 ** -126 if out_bf16 else f32


def bwd_bound(out_bf16, length, p, dp, s, scale, exact):
    scale = float(np.float32(scale))
    u = (length + 5.0) * 2.0 ** -24
    f32 = (scale * u / (1.0 - u) * np.abs(np.asarray(p, np.float64)) * (np.abs(np.asarray(dp, np.float64)) + np.asarray(s, np.float64))
           + (length + 3.0) * 2.0 ** -126 * max(1.0, scale))
    return 2.0 ** -8 * np.abs(np.asarray(exact, np.float64)) + (1.0 + 2.0 ** -8) * f32 + 2.0 ** -126 if out_bf16 else f32


def assert_inside(got, exact, lim, what=""):
    got, exact, lim = np.asarray(got).astype(LD), np.asarray(exact).astype(LD), np.asarray(lim).astype(LD)
    err = np.abs(got - exact)
    worst = float(np.max(err / np.where(lim > 0, lim, 1.0), initial=0.0))
    print(f"{what}: max |err| / bound = {worst:.3g}")
    bad = ~(err <= lim)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound, worst {worst:.3g} x at {np.argwhere(bad)[:4].tolist()}"
    return worst


# ---- operands
def scores(kind, name, seed=0):
    """narrow: uniform in [-4, 4), full mantissa.  wide: uniform in [-60, 60).  equal: one value everywhere.  float32
    [num_blocks, bS, bS]."""
    bsr = pattern(name)
    shape = (bsr.num_blocks, bsr.block_row_size, bsr.block_row_size)
    rng = np.random.default_rng(9000 + seed)
    if kind == "narrow":
        return rng.uniform(-4.0, 4.0, shape).astype(np.float32)
    if kind == "wide":
        return rng.uniform(-60.0, 60.0, shape).astype(np.float32)
    assert kind == "equal"
    return np.full(shape, 0.7, dtype=np.float32)


def random_mask(name, seed=1):
    """A bias in [-2, 2) with about a quarter of the entries -Inf, never a whole matrix row: every row's first element stays."""
    bsr = pattern(name)
    shape = (bsr.num_blocks, bsr.block_row_size, bsr.block_row_size)
    rng = np.random.default_rng(9100 + seed)
    m = rng.uniform(-2.0, 2.0, shape).astype(np.float32)
    hide = rng.random(shape) < 0.25
    row_ptrs, idx = layout(name)
    hide.reshape(-1)[idx[row_ptrs[:-1][np.diff(row_ptrs) > 0]]] = False
    m[hide] = -np.inf
    return m


def causal_mask(name):
    """Block-causal: -Inf above the diagonal inside the blocks on the diagonal (block column == block row), 0 elsewhere."""
    bsr = pattern(name)
    bs = bsr.block_row_size
    ptrs = np.asarray(bsr.block_row_ptrs, dtype=np.int64)
    rows = np.repeat(np.arange(ptrs.shape[0] - 1), np.diff(ptrs))
    m = np.zeros((bsr.num_blocks, bs, bs), np.float32)
    upper = np.triu(np.ones((bs, bs), bool), k=1)
    diag = np.asarray(bsr.block_col_idxs, dtype=np.int64) == rows
    m[diag] = np.where(upper, -np.inf, 0.0).astype(np.float32)
    return m


def full_mantissa(rng, shape):
    v = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, shape)
    return v.astype(np.float32)


def bf16_round(v):
    """float32 -> the nearest bf16 number (ties to even), as float32; a NaN stays a NaN."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), v, synth.bf16_round(np.where(np.isnan(v), np.float32(0), v)))
