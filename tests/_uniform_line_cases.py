"""Operands of the straight-line row-gather tests (tests/test_gpu_uniform_line.py), built on the host from fixed seeds so that
tests/test_uniform_line_cpu.py can check on the CPU, with the oracle alone, what the GPU tests rely on: the FAST corpus is
sharp (an unfused or reversed chain shows in the bits) and the adversarial rows have the closed-form results their
construction promises.  Shapes are the smallest at which the body can go wrong, not a workload's."""
import numpy as np

from mispmm import formats

import _adversarial as adv
from _fma_chain import sharp_values

WIDTHS = (9, 10, 11, 12, 13, 14)            # every row length the straight-line body takes (slot counts 10, 12, 14)
ROW_COUNTS = (1, 7, 8, 9, 33)               # a partial workgroup, one row, row parts of the XCD grid left empty, a short last part
COL_COUNTS = (64, 128, 192, 256, 512)       # the 8 x 1, 4 x 2, 8-lane-group and 1 x 8 tilings
BIG_K = 16400                               # K x 256 B > 4 MiB: N = 256 takes eight 32-column parts (8-lane groups)


def uniform_csr(m, k, width, seed, edges=True):
    """m rows of exactly `width` entries, columns ascending inside a row and drawn over the whole of [0, k); with `edges`,
    row 0 reads column 0 and the last row column k - 1."""
    rng = np.random.default_rng(seed)
    cols = np.stack([np.sort(rng.choice(k, size=width, replace=False)) for _ in range(m)])
    if edges and k > width:
        cols[0, 0] = 0
        cols[m - 1, width - 1] = k - 1
    ptr = (np.arange(m + 1, dtype=np.int64) * width).astype(np.uint32)
    return formats.CSR(m, k, ptr, cols.reshape(-1).astype(np.uint32), sharp_values(rng, m * width, np.float32))


_B = {}


def dense_b(k, n):
    """The first n columns of one seeded [k, 512] sharp operand per k."""
    if k not in _B:
        _B[k] = sharp_values(np.random.default_rng(7700 + k), (k, 512), np.float32)
    return np.ascontiguousarray(_B[k][:, :n])


def padded_ell_csr(width, seed):
    """Rows of 0 .. width entries (every length twice, an all-padding row first and last): its ELL has `width` slots."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[0], np.arange(width + 1), np.arange(width, -1, -1), [width, 0]])
    k = 3 * width
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cols = np.concatenate([np.sort(rng.choice(k, size=int(n), replace=False)) for n in lens]).astype(np.uint32)
    return formats.CSR(lens.shape[0], k, ptr, cols, sharp_values(rng, int(ptr[-1]), np.float32))


# ---------------------------------------------------------------------------------------------- adversarial rows, width 14
ADV_WIDTH, ADV_K = 14, 96
_NAN_ROW, _INF_ROW, _NINF_ROW, _ZERO_ROW, _NZERO_ROW = 0, 90, 91, 92, 93      # B rows with a meaning; row 0 is never referenced


def adversarial(n=128):
    """One uniform matrix of width 14 and its B.  Returns (csr, b, expect) where expect maps a row index to the closed-form
    result row the construction promises (checked against the oracle on the CPU):
      rows 0-1   (3e38, 3e38, -3e38) at slots (0, 7, 13) and (6, 8, 9), zeros between: 3e38 * pattern in fp64 sums, Inf in fp32
      rows 2-3   (1, 2^-30, -1): 2^-30 * pattern in fp64 sums, 0 in fp32
      rows 4-5   (2^24, 1, -2^24) and (1, 2^24, -2^24) across the slot 7 / 8 boundary: pattern
      rows 6-7   (2^60, 1, -2^60) and (1, 2^60, -2^60): +0 (the 1 is lost in either storage order, never recovered)
      row 8      an Inf row of B behind a coefficient 1 and a -Inf row behind a 1: NaN everywhere
      row 9      stored zeros meeting the Inf row: NaN
      row 10     one entry on the +Inf row, finite others: +Inf
      row 11     every product a -0 (negative x +0, positive x -0): +0, never -0
      row 12     -0 coefficients: +0
      rows 13+   random sharp rows (no closed form)
    B row 0 is NaN and no entry references it: a dropped slot that read B after all would show."""
    rng = np.random.default_rng(4242)
    w, k = ADV_WIDTH, ADV_K
    b = sharp_values(rng, (k, n), np.float32)
    b[_NAN_ROW] = np.nan
    b[_INF_ROW], b[_NINF_ROW] = np.inf, -np.inf
    b[_ZERO_ROW], b[_NZERO_ROW] = 0.0, -0.0
    pat = adv.pattern_row(n)
    b[1:30] = pat                                          # B rows 1..29: the pattern (discriminating terms only)
    plain = np.arange(30, 80)                              # B rows 30..79: finite sharp values
    rows, expect = [], {}

    def disc(terms, slots, want):
        """zero coefficients on plain rows, the three terms on pattern rows of their own at the given slots"""
        row = [(int(c), 0.0) for c in np.sort(rng.choice(plain, w, replace=False))]
        for i, (s, v) in enumerate(zip(slots, terms)):
            row[s] = (1 + 3 * len(rows) + i, float(np.float32(v)))
        expect[len(rows)] = np.asarray(want, np.float32)
        rows.append(row)

    def filler(count):
        return [(int(c), float(sharp_values(rng, 1, np.float32)[0])) for c in np.sort(rng.choice(plain, count, replace=False))]
    for slots in ((0, 7, 13), (6, 8, 9)):
        disc((3e38, 3e38, -3e38), slots, np.float32(3e38) * pat)
    for slots in ((0, 7, 13), (7, 8, 12)):
        disc((1.0, 2.0 ** -30, -1.0), slots, np.float32(2.0 ** -30) * pat)
    for terms in ((adv.BIG32, 1.0, -adv.BIG32), (1.0, adv.BIG32, -adv.BIG32)):
        disc(terms, (6, 7, 8), pat)
    for terms in ((adv.BIG64, 1.0, -adv.BIG64), (1.0, adv.BIG64, -adv.BIG64)):
        disc(terms, (0, 8, 13), np.zeros(n, np.float32))
    rows.append(filler(w - 2) + [(_INF_ROW, 1.0), (_NINF_ROW, 1.0)])
    expect[8] = np.full(n, np.nan, np.float32)
    rows.append(filler(w - 1) + [(_INF_ROW, 0.0)])
    expect[9] = np.full(n, np.nan, np.float32)
    rows.append(filler(w - 1) + [(_INF_ROW, 1.0)])
    expect[10] = np.full(n, np.inf, np.float32)
    rows.append([(_ZERO_ROW, -1.5), (_NZERO_ROW, 2.0)] * (w // 2))               # every product is -0; repeated columns
    expect[11] = np.zeros(n, np.float32)
    rows.append([(c, -0.0) for c, _ in filler(w)])
    expect[12] = np.zeros(n, np.float32)
    while len(rows) < 19:                                                       # 19 rows: three workgroups of 8, the last short
        rows.append(filler(w))
    csr = adv.csr_from_rows(rows, k)
    assert np.all(np.diff(csr.row_ptrs.astype(np.int64)) == w) and not np.any(csr.col_idxs == _NAN_ROW)
    return csr, b, expect
