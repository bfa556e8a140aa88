"""The contracts of mispmm_rows_bf16 (include/mispmm_bf16.h) restated in numpy on top of the project's own oracles, and the
cases the CPU and GPU tests of the row-list product with B in bf16 share.

B widens to fp32 exactly, so with fp32 values of A each arithmetic IS an oracle the project already owns, applied to the
widened B: FAST = oracle.rows_fma, REFERENCE with a double sum = oracle.spmm_csr, REFERENCE with an fp32 sum =
_fma_chain.chain_unfused.  A padding slot (column 0xFFFFFFFF) is a DEAD SLOT: coefficient 0 times a B element of 0 -- here a
row of zeros appended to B that every padding slot is pointed at.  The stored value is chain + (+0)."""
import functools

import numpy as np

import _fma_chain as fc

PAD = 0xFFFFFFFF
MODES = ("fast", "ref64", "ref32")                  # the tag's word -> (acc, ref_sum) of the ops functions
OPS_ARGS = {"fast": ("fast", "f64"), "ref64": ("reference", "f64"), "ref32": ("reference", "f32")}
SEED = 7
MAX_N = 528                                          # widest B of a case: every narrower case is its leading columns


# ------------------------------------------------------------------------------------------------ bf16
def widen(bits):
    """uint16 / int16 bf16 bits -> float32, exactly: the bits moved to the upper half."""
    b = np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << np.uint32(16)
    return b.view(np.float32)


def bf16_bits(x):
    """float32 -> uint16 bf16 bits, one rounding to nearest even; a NaN stays a NaN (quieted, sign and upper payload kept)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(x)
    r[nan] = ((u[nan] >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16)
    return r


def same_bits(got, want):
    """Bit for bit, NaNs compared as NaNs (a NaN's payload is the hardware's business).  got / want: float32, or bf16 bits."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.float32:
        g, w, gn, wn = got.view(np.uint32), want.view(np.uint32), np.isnan(got), np.isnan(want)
    else:
        g, w = got.view(np.uint16), want.view(np.uint16)
        gn, wn = np.isnan(widen(g)), np.isnan(widen(w))
    return g.shape == w.shape and np.array_equal(gn, wn) and np.array_equal(g[~gn], w[~wn])


# ------------------------------------------------------------------------------------------------ the three chains
def dead_slots(row_ptrs, row_nnz, col_idxs, vals, b):
    """The list as the kernel walks it: (rowPtrs, cols, vals, B) with every padding slot pointed at a zero row appended to B
    and its coefficient forced to 0.  row_ptrs None: the uniform list of row_nnz entries per row."""
    cols = np.asarray(col_idxs, np.uint32).reshape(-1).copy()
    vals = np.asarray(vals, np.float32).reshape(-1).copy()
    if row_ptrs is None:
        assert row_nnz > 0 and cols.shape[0] % row_nnz == 0
        row_ptrs = np.arange(cols.shape[0] // row_nnz + 1, dtype=np.uint32) * np.uint32(row_nnz)
    pad = cols == np.uint32(PAD)
    cols[pad] = b.shape[0]
    vals[pad] = 0.0
    return np.asarray(row_ptrs, np.uint32), cols, vals, np.concatenate([b, np.zeros((1, b.shape[1]), np.float32)])


def expected(mode, row_ptrs, col_idxs, vals, b_bits, row_nnz=0):
    """The fp32 C of mispmm_rows_bf16 for the tag word `mode`, by the oracle of that arithmetic on the widened B."""
    rp, cols, va, b = dead_slots(row_ptrs, row_nnz, col_idxs, vals, widen(b_bits))
    if cols.shape[0] == 0:
        return np.zeros((rp.shape[0] - 1, b.shape[1]), np.float32)
    if mode == "fast":
        out = fc._oracle().rows_fma(rp, cols, va, b)
    elif mode == "ref64":
        out = fc._oracle().spmm_csr(rp, cols, va, b)
    else:
        out = fc.chain_unfused(rp, cols, va, b)
    with np.errstate(invalid="ignore"):
        return (out + np.float32(0.0)).astype(np.float32)       # chain + (+0): a -0 sum is stored as +0


# ------------------------------------------------------------------------------------------------ lane widths and tags
def pick(n, ldb, ldc, b_off=0, c_off=0, out_bf16=False):
    """(G, V) as the library picks them; b_off / c_off: the element offsets of B and C from a 16-byte aligned address."""
    cb = 2 if out_bf16 else 4
    b16, c16 = (b_off * 2) % 16 == 0, (c_off * cb) % 16 == 0
    b8, c8 = (b_off * 2) % 8 == 0, (c_off * cb) % 8 == 0
    if n % 8 == 0 and ldb % 8 == 0 and b16 and c16 and ldc % (8 if out_bf16 else 4) == 0:
        v = 8
    elif n % 4 == 0 and ldb % 4 == 0 and b8 and c8 and ldc % (4 if out_bf16 else 2) == 0:
        v = 4
    else:
        v = 1
    need, g = -(-n // v), 8
    while g < 64 and g < need:
        g *= 2
    return g, v


def tag_of(mode, n, ldb=None, ldc=None, b_off=0, c_off=0, out_bf16=False):
    g, v = pick(n, n if ldb is None else ldb, n if ldc is None else ldc, b_off, c_off, out_bf16)
    return f"rows_bf16<G{g},V{v},{mode}>"


def head(tag):
    """The instance of a mispmm_last_kernel() string: its out type and XCD grid dropped."""
    return tag.split(" ")[0]


# tag -> the smallest N (contiguous, aligned operands) that reaches it: one column less lands on another tag
SMALLEST_N = {(8, 8): 8, (16, 8): 72, (32, 8): 136, (64, 8): 264, (8, 4): 4, (16, 4): 36, (32, 4): 68, (64, 4): 132,
              (8, 1): 1, (16, 1): 9, (32, 1): 17, (64, 1): 33}
TAGS = {f"rows_bf16<G{g},V{v},{mode}>": n for (g, v), n in SMALLEST_N.items() for mode in MODES}
WIDTHS = sorted(set(SMALLEST_N.values()) | {520, 65})       # 520, 65: a second block of columns at V8 and V1


# ------------------------------------------------------------------------------------------------ the matrices
class Case:
    """A row list with sharp fp32 values, a sharp B rounded to bf16 (MAX_N columns), and per arithmetic the expected C of
    the full width, computed once: an element of C depends on its own column of B alone, so a case of N columns is the
    leading N columns of everything."""

    def __init__(self, name, num_rows, num_cols, row_ptrs, col_idxs, seed=SEED, max_n=MAX_N):
        rng = np.random.default_rng(seed)
        self.name, self.num_rows, self.num_cols = name, num_rows, num_cols
        self.row_ptrs = np.asarray(row_ptrs, np.uint32)
        self.col_idxs = np.asarray(col_idxs, np.uint32)
        self.vals = fc.sharp_values(rng, self.col_idxs.shape[0], np.float32)
        self.b_bits = bf16_bits(fc.sharp_values(rng, (num_cols, max_n), np.float32))

    @property
    def rows(self):
        return self.row_ptrs, self.col_idxs, self.vals

    def csr(self):
        from mispmm import formats
        return formats.CSR(self.num_rows, self.num_cols, self.row_ptrs, self.col_idxs, self.vals)

    @functools.lru_cache(maxsize=None)
    def expected(self, mode):
        out = expected(mode, self.row_ptrs, self.col_idxs, self.vals, self.b_bits)
        out.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def sharpness(self, n):
        return fc.sharpness(self.rows, widen(self.b_bits[:, :n]))

    def is_sharp(self, n):
        unfused, backwards, count = self.sharpness(n)
        return count > 0 and unfused >= fc.SHARP_SHARE and backwards >= fc.SHARP_SHARE


def _ragged():
    """The 96 x 400 list of smoke(): rows of 0..9 entries and rows of 300, 40, 129 and 77 -- they cross chunk ends at every
    G and a ring end at 8."""
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 10, 96)
    lens[[3, 40, 41, 90]] = [300, 40, 129, 77]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    cols = np.concatenate([np.sort(rng.choice(400, size=n, replace=False)) for n in lens])
    return Case("ragged", 96, 400, ptr, cols)


def _uniform():
    from mispmm import datasets
    csr = datasets.load_csr("n3c5-b6")               # 120 x 210, 7 entries in every row
    return Case("n3c5-b6", csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs)


def _edges():
    """Empty first and last rows (and two in the middle), the others 1..20 entries: 37 x 150."""
    rng = np.random.default_rng(11)
    lens = rng.integers(1, 21, 37)
    lens[[0, 17, 18, 36]] = 0
    ptr = np.concatenate([[0], np.cumsum(lens)])
    cols = np.concatenate([rng.choice(150, size=n, replace=False) for n in lens])     # unsorted columns inside a row
    return Case("edges", 37, 150, ptr, cols)


def _empty():
    return Case("empty", 16, 32, np.zeros(17, np.uint32), np.zeros(0, np.uint32))


_MAKERS = {"ragged": _ragged, "n3c5-b6": _uniform, "edges": _edges, "empty": _empty}


@functools.lru_cache(maxsize=None)
def case(name):
    return _MAKERS[name]()
