"""Adversarial corpus for the bitwise parity tests (host only, numpy).

Random data rounds the same way in almost every order, so a kernel that re-associates a sum, widens or narrows its
accumulator, starts a sum from -0, or lets a padding slot read real B data passes it.  Each case here is built so that one
of those mistakes changes the bits:

  signed_zero     negative A times +0 / -0 columns of B, -0 values in A, one-entry and empty rows: the reference gives +0
  order           (big, 1, -big) and (1, big, -big) with big = 2^60 (fp64 sequential order) and 2^24 (fp32 sequential order)
                  at positions in different 8-lane groups, 4-wave chunks (share_len 0 / 8 / 30 / 128), ring / LDS phases
                  (around 256 and 512) and either side of the two-body launch's 32-entry boundary
  width           (3e38, 3e38, -3e38) and (1, 2^-30, -1): the CSR (fp64) and COO / ELL / BSR (fp32) results differ
  storage_order   columns descending, in random order, and repeated within a row
  subnormal       subnormal products, inputs and sums
  nonfinite       Inf / NaN in A, Inf - Inf, a stored zero meeting Inf in B
  poisoned_nan / poisoned_inf
                  every B row no stored entry references is NaN / +Inf (the GPU tests add NaN ldb gaps and A arrays whose
                  tails past nnz hold NaN and the index of a poisoned row)
and uniform-width variants (order_uniform, poisoned_uniform) for the paths that take rows of one width only.

A case is (name, CSR, B); the other formats are derived from it.  Every index is in range."""
from dataclasses import dataclass, field

import numpy as np

from mispmm import formats

BIG64, BIG32 = np.float32(2.0 ** 60), np.float32(2.0 ** 24)
N_DEFAULT = 64
# the B rows a discriminator reads: powers of two only (products stay exact), the same in every row so that big and -big
# cancel in every output column; |x| <= 1 so that 3e38 * x is finite
PATTERN = np.array([1.0, -1.0, 0.5, -0.25, 1.0, 0.125, -0.5, 1.0], np.float32)


@dataclass
class Case:
    name: str
    csr: formats.CSR
    b: np.ndarray                       # [K, N] float32
    poison: float = None                # the value of the B rows no entry references (NaN / +Inf), None = not poisoned
    poison_cols: np.ndarray = None      # those rows
    tags: set = field(default_factory=set)

    @property
    def has_duplicates(self):
        rp = self.csr.row_ptrs.astype(np.int64)
        return any(len(set(self.csr.col_idxs[rp[r]:rp[r + 1]].tolist())) != rp[r + 1] - rp[r] for r in range(self.csr.num_rows))

    @property
    def uniform_width(self):
        lens = np.diff(self.csr.row_ptrs.astype(np.int64))
        return int(lens[0]) if lens.size and lens[0] > 0 and np.all(lens == lens[0]) else 0


def csr_from_rows(rows, num_cols):
    """rows: one list of (col, value) per row, in storage order."""
    lens = [len(r) for r in rows]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cols = np.array([c for r in rows for c, _ in r], np.uint32)
    vals = np.array([v for r in rows for _, v in r], np.float32)
    return formats.CSR(len(rows), num_cols, ptr, cols, vals)


def pattern_row(n, scale=1.0):
    return (np.resize(PATTERN, n) * np.float32(scale)).astype(np.float32)


def signed_zero(n=N_DEFAULT):
    m, k = 64, 128
    rng = np.random.default_rng(11)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    b[:, 0::4] = 0.0                                   # output columns whose every term is a signed zero
    b[:, 1::4] = -0.0
    b[96:112] = 0.0                                    # whole B rows of +0 and of -0
    b[112:128] = -0.0
    rows = []
    for r in range(m):
        kind = r % 8
        if kind == 0:
            rows.append([])                                                        # empty row
        elif kind == 1:
            rows.append([(int(rng.integers(0, k)), -float(rng.uniform(0.5, 2)))])   # one negative entry
        elif kind == 2:
            rows.append([(int(c), -0.0) for c in np.sort(rng.choice(k, 3, replace=False))])   # -0 values
        elif kind == 3:                                                            # negatives times zero B rows only
            rows.append([(int(c), -float(rng.uniform(0.5, 2))) for c in np.sort(rng.choice(np.arange(96, 128), 5, replace=False))])
        elif kind == 4:                                                            # long rows of negatives (split / two-body)
            ln = (40, 130, 33, 300)[(r // 8) % 4]
            rows.append([(int(c), -float(rng.uniform(0.5, 2))) for c in np.sort(rng.choice(k, min(ln, k), replace=False))])
        elif kind == 5:
            rows.append([(int(c), float(rng.uniform(0.5, 2))) for c in np.sort(rng.choice(k, 9, replace=False))])
        elif kind == 6:                                                            # x - x: a cancellation to zero
            c0, c1 = np.sort(rng.choice(96, 2, replace=False))
            b[c1] = b[c0]
            rows.append([(int(c0), 1.5), (int(c1), -1.5)])
        else:
            rows.append([(int(rng.integers(0, k)), -1.0)])
    return Case("signed_zero", csr_from_rows(rows, k), b, tags={"zero"})


# (row length, positions of the three discriminating terms in storage order)
ORDER_PLACES = [(3, (0, 1, 2)), (9, (0, 4, 8)), (17, (0, 8, 16)), (24, (7, 8, 23)), (31, (0, 15, 30)), (32, (0, 16, 31)),
                (33, (0, 16, 32)), (40, (5, 20, 35)), (129, (0, 64, 128)), (129, (30, 31, 100)), (200, (29, 30, 180)),
                (300, (74, 75, 225)), (520, (255, 256, 511)), (600, (10, 256, 512)), (600, (511, 512, 513))]


def _disc_rows(rng, k, b, places, bigs, filler_scale=1.0, cols_fn=None):
    rows = []
    for ln, pos in places:
        for big in bigs:
            for vals in ((big, 1.0, -big), (1.0, big, -big)):
                cols = np.sort(rng.choice(k, ln, replace=False)) if cols_fn is None else cols_fn(ln)
                row = [(int(c), float(rng.choice([-3, -2, -1, 1, 2, 3]) * filler_scale)) for c in cols]
                for p, v in zip(pos, vals):
                    row[p] = (row[p][0], float(v))
                    b[row[p][0]] = pattern_row(b.shape[1])
                rows.append(row)
    return rows


def order(n=N_DEFAULT):
    m, k = 96, 640
    rng = np.random.default_rng(12)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    rows = _disc_rows(rng, k, b, ORDER_PLACES, (BIG64, BIG32))
    while len(rows) < m:                                                           # short rows around them
        rows.append([(int(c), float(rng.uniform(-1, 1))) for c in np.sort(rng.choice(k, int(rng.integers(0, 6)), replace=False))])
    return Case("order", csr_from_rows(rows, k), b, tags={"order"})


def order_uniform(n=N_DEFAULT, width=16):
    """Rows of one width (the uniform entry, the LDS tiles, the persistent row walk): a discriminator in every row."""
    m, k = 64, 640
    rng = np.random.default_rng(13)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    places = [(width, p) for p in ((0, 1, 2), (0, 8, width - 1), (7, 8, 9), (1, width - 2, width - 1))]
    rows = []
    while len(rows) < m:
        rows += _disc_rows(rng, k, b, places, (BIG64, BIG32))
    return Case(f"order_uniform{width}", csr_from_rows(rows[:m], k), b, tags={"order", "uniform"})


def width(n=N_DEFAULT):
    """fp64 and fp32 sums of the same terms differ; between the terms, explicit zeros."""
    m, k = 32, 128
    rng = np.random.default_rng(14)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    rows = []
    for terms in ((3e38, 3e38, -3e38), (1.0, 2.0 ** -30, -1.0)):
        for ln, pos in ((3, (0, 1, 2)), (40, (0, 20, 39)), (9, (2, 5, 8)), (130, (0, 64, 129))):
            cols = np.sort(rng.choice(k, min(ln, k), replace=False))
            row = [(int(c), 0.0) for c in cols]
            for p, v in zip(pos, terms):
                p = min(p, len(row) - 1)
                row[p] = (row[p][0], float(np.float32(v)))
                b[row[p][0]] = pattern_row(n)
            rows.append(row)
    while len(rows) < m:
        rows.append([])
    return Case("width", csr_from_rows(rows, k), b, tags={"width"})


def storage_order(n=N_DEFAULT):
    m, k = 32, 128
    rng = np.random.default_rng(15)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    for c in (1, 3, 5, 7, 9, 11):
        b[c] = pattern_row(n)
    rows = [[(5, BIG32), (1, 1.0), (3, -BIG32)],                                     # column order 1 3 5 gives 1, storage order 0
            [(5, BIG64), (1, 1.0), (3, -BIG64)],
            [(11, 1.0), (9, BIG32), (7, -BIG32)],                                    # descending
            [(11, 1.0), (9, BIG64), (7, -BIG64)],
            [(3, BIG32), (7, 1.0), (3, -BIG32)],                                     # a repeated column
            [(3, BIG64), (7, 1.0), (3, -BIG64), (7, 2.0)]]
    for ln in (9, 17, 40, 100):                                                   # longer rows: random and descending order
        cols = list(rng.choice(np.arange(12, k), ln - 3, replace=False))
        row = [(int(c), float(rng.uniform(-1, 1))) for c in cols] + [(9, BIG32), (1, 1.0), (11, -BIG32)]
        perm = rng.permutation(len(row))
        rows.append([row[i] for i in perm])
        rows.append(sorted(row, key=lambda e: -e[0]))
    while len(rows) < m:
        rows.append([(int(c), float(rng.uniform(-1, 1))) for c in rng.choice(k, 4, replace=False)])
    return Case("storage_order", csr_from_rows(rows, k), b, tags={"order", "unsorted"})


def subnormal(n=N_DEFAULT):
    m, k = 32, 128
    rng = np.random.default_rng(16)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    tiny, one = np.arange(0, 32), np.arange(32, 64)
    b[tiny] = pattern_row(n, 2.0 ** -70)
    b[one] = pattern_row(n)
    s = float(2.0 ** -126)
    rows = [[(0, 2.0 ** -70)],                                                    # product 2^-140: subnormal
            [(1, 2.0 ** -60)],                                                    # 2^-130
            [(32, 2.0 ** -140)],                                                  # a subnormal input times 1
            [(33, 2.0 ** -149), (34, 2.0 ** -149), (35, 2.0 ** -149)],            # sums of the smallest subnormal
            [(36, 1.5 * s), (37, -s)],                                            # normal terms, a subnormal sum (2^-127)
            [(int(c), 2.0 ** -75) for c in tiny] + [(int(c), 2.0 ** -149) for c in one[:9]],   # 41 entries: split / two-body
            [(int(c), 2.0 ** -76) for c in tiny[:20]] + [(int(c), -2.0 ** -146) for c in one[:20]],
            [(40, 2.0 ** -126), (41, -(2.0 ** -126 - 2.0 ** -149))]]             # 2^-149 exactly
    while len(rows) < m:
        rows.append([(int(c), float(rng.choice([-1, 1]) * 2.0 ** -float(rng.integers(64, 80)))) for c in rng.choice(tiny, 5, replace=False)])
    return Case("subnormal", csr_from_rows(rows, k), b, tags={"subnormal"})


def nonfinite(n=N_DEFAULT):
    m, k = 32, 128
    rng = np.random.default_rng(17)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    b[:, 5] = 0.0                                                                 # Inf * 0 in every row with an Inf
    c_inf = 100
    b[c_inf] = np.inf                                                             # read only through stored zeros and one entry
    b[c_inf + 1, :] = -np.inf
    inf, nan = float("inf"), float("nan")
    rows = [[(3, inf)], [(3, -inf)], [(4, inf), (6, -inf)], [(7, nan), (8, 1.0)], [(c_inf, 0.0)], [(9, 1.0), (c_inf, 0.0), (10, 2.0)],
            [(c_inf, 1.0), (c_inf + 1, 1.0)], [(c_inf, -0.0)], [(c_inf + 1, 2.0)]]
    for ln, p in ((40, 35), (130, 100), (300, 3)):                               # one non-finite term in a long row
        cols = np.sort(rng.choice(np.arange(0, 100), min(ln, 100), replace=False))
        row = [(int(c), float(rng.uniform(-1, 1))) for c in cols]
        p = min(p, len(row) - 1)
        row[p] = (row[p][0], inf)
        rows.append(row)
        row = list(row)
        row[0] = (row[0][0], nan)
        rows.append(row)
    while len(rows) < m:
        rows.append([(int(c), float(rng.uniform(-1, 1))) for c in np.sort(rng.choice(100, 3, replace=False))])
    return Case("nonfinite", csr_from_rows(rows, k), b, tags={"nonfinite"})


def _poisoned(name, rows_fn, poison, k, n, seed, tags):
    rng = np.random.default_rng(seed)
    # never referenced: B row 0 (where a padding slot that loaded instead of dropping its load would read), two 32-aligned
    # ranges (outside every block of every block shape) and scattered single columns
    poison_cols = np.unique(np.concatenate([[0], np.arange(320, 384), np.arange(k - 64, k), np.arange(7, k - 64, 13)]))
    live = np.setdiff1d(np.arange(k), poison_cols)
    rows = rows_fn(rng, live)
    csr = csr_from_rows(rows, k)
    assert not np.isin(csr.col_idxs, poison_cols).any()
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    b[poison_cols] = poison
    return Case(name, csr, b, poison, poison_cols, tags | {"poisoned"})


def poisoned(poison, n=N_DEFAULT):
    def rows_fn(rng, live):
        rows = []
        for r in range(96):
            ln = int(rng.integers(0, 10))
            if r % 11 == 3:
                ln = (40, 129, 300, 33, 64)[(r // 11) % 5]
            rows.append([(int(c), float(rng.uniform(-2, 2))) for c in np.sort(rng.choice(live, ln, replace=False))])
        return rows
    tag = "nan" if np.isnan(poison) else "inf"
    return _poisoned(f"poisoned_{tag}", rows_fn, poison, 640, n, 18 if tag == "nan" else 19, set())


def poisoned_uniform(poison, n=N_DEFAULT, width=14):
    def rows_fn(rng, live):
        return [[(int(c), float(rng.uniform(-2, 2))) for c in np.sort(rng.choice(live, width, replace=False))] for _ in range(64)]
    tag = "nan" if np.isnan(poison) else "inf"
    return _poisoned(f"poisoned_uniform{width}_{tag}", rows_fn, poison, 640, n, 20, {"uniform"})


def corpus(n=N_DEFAULT):
    return [signed_zero(n), order(n), order_uniform(n), width(n), storage_order(n), subnormal(n), nonfinite(n),
            poisoned(np.float32(np.nan), n), poisoned(np.float32(np.inf), n), poisoned_uniform(np.float32(np.nan), n),
            poisoned_uniform(np.float32(np.inf), n)]


# ------------------------------------------------------------------ the other formats of a case, and their expected bits
def coo_shuffled(csr, seed=0):
    """The COO of `csr` with its entries in a random storage order (rows interleaved, a row's entries in a new order)."""
    coo = formats.csr_to_coo(csr)
    perm = np.random.default_rng(seed).permutation(coo.nnz)
    return formats.COO(coo.num_rows, coo.num_cols, coo.row_idxs[perm], coo.col_idxs[perm], coo.data[perm])


def bsr_of(case, br, bc):
    """(BSR of the case's CSR, the B it is multiplied with): the poisoned rows that fall inside a stored block -- which the
    reference multiplies whole -- are given finite values, so that only rows outside every block stay poisoned."""
    bsr = formats.csr_to_bsr(case.csr, br, bc)
    b = case.b.copy()
    if case.poison is not None:
        inside = np.zeros(case.csr.num_cols, bool)
        for j in np.unique(bsr.block_col_idxs):
            inside[int(j) * bc:(int(j) + 1) * bc] = True
        fix = np.intersect1d(np.nonzero(inside)[0], case.poison_cols)
        b[fix] = np.float32(0.75)
    return bsr, b


def bsr_entries(bsr, nonzero_only=False):
    """The entries of a BSR as (rows, cols, vals) in the order the reference adds them into each row (block by block, then
    the block's columns ascending); nonzero_only: the zero-skipping paths' list (+0 and -0 left out)."""
    rows, cols, vals = [], [], []
    br, bc = bsr.block_row_size, bsr.block_col_size
    for i in range(bsr.num_block_rows):
        for q in range(int(bsr.block_row_ptrs[i]), int(bsr.block_row_ptrs[i + 1])):
            j = int(bsr.block_col_idxs[q])
            rr, cc = np.meshgrid(np.arange(br), np.arange(bc), indexing="ij")
            v = bsr.data[q]
            keep = (v != 0) if nonzero_only else np.ones_like(v, bool)
            rows.append((i * br + rr)[keep])
            cols.append((j * bc + cc)[keep])
            vals.append(v[keep])
    if not rows:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32)
    return (np.concatenate(rows).astype(np.uint32), np.concatenate(cols).astype(np.uint32), np.concatenate(vals).astype(np.float32))


BLOCK_SHAPES = [(1, 1), (2, 2), (4, 4), (8, 8), (16, 16), (32, 32), (2, 4), (4, 2), (1, 8), (8, 16), (16, 8), (32, 4)]
