"""ALGORITHM of mispmm_sddmm_csr_bf16 (include/mispmm_sddmm_bf16.h) restated in numpy, lane by lane, with the lane-width rule,
the tag, the operands the CPU and GPU tests share, and named breaches (`fault=`) that show what the bit checks can see.

    out[e] = sum_j x[row(e)][j] * y[col(e)][j]          x, y bf16, widened exactly

G lanes own a row; lane l owns columns c * G * V + l * V + v of every chunk c.  Each lane runs one chain from +0 over its
columns in ascending order -- FAST an fp32 fma, REFERENCE an fp64 fma -- and the G sums are added as a butterfly adds them,
lane ^ 1 first.  The fp32 fma is emulated as float32(float64(acc) + float64(x) * float64(y)): the product of two bf16 numbers
has 16 bits and is exact, and on the operands used here (exponents within a few dozen of each other) the double add is exact
too, so the one rounding is the conversion.  In REFERENCE the double product is exact, so `acc + x * y` IS the fused form."""
import functools

import numpy as np

from _sddmm_ref import entry_rows, sddmm_exact
from _spmm_bf16_ref import bf16_bits, same_bits, widen  # noqa: F401  (re-exported for the tests)

MODES = {"fast": "fast", "reference": "ref64"}          # acc of the Python layer -> the tag's word
FAULTS = ("swap_halves", "drop_last_chunk", "drop_eighth_slot", "tree_high_first", "ref_in_f32", "x_next_row", "read_gap")

# the smallest N (contiguous, aligned operands) that reaches each (G, V, chunks held): one lane's columns less is another tag
# (G8 is reached from one lane's columns on: 8 at V8; at V1 the table holds 3, an odd width of more than one column)
SMALLEST_N = {(8, 8, 1): 8, (16, 8, 1): 72, (32, 8, 1): 136, (64, 8, 1): 264, (64, 8, 2): 520, (64, 8, 4): 1032, (64, 8, 0): 2056,
              (8, 1, 1): 3, (16, 1, 1): 9, (32, 1, 1): 17, (64, 1, 1): 33, (64, 1, 2): 65, (64, 1, 4): 129, (64, 1, 0): 257}
V8_WIDTHS = [n for (g, v, c), n in SMALLEST_N.items() if v == 8]
V1_WIDTHS = [n for (g, v, c), n in SMALLEST_N.items() if v == 1]
TAGS = {f"sddmm_csr_bf16<{word},G{g},V{v},C{c}>": n for (g, v, c), n in SMALLEST_N.items() for word in MODES.values()}
INSTANCES = {"sddmm_csr_bf16_kernel": 28}               # 2 arithmetics x 2 lane widths x 7 shapes


# ------------------------------------------------------------------------------------------------ lane widths and tags
def pick_group(n, v):
    need, g = -(-n // v), 8
    while g < 64 and g < need:
        g *= 2
    return g


def pick(n, ldx=None, ldy=None, x_off=0, y_off=0):
    """(G, V, C) as the library picks them; x_off / y_off: element offsets of X and Y from a 16-byte aligned address.
    C: chunks of X's row held in registers, 0 = re-read per batch."""
    ldx, ldy = n if ldx is None else ldx, n if ldy is None else ldy
    wide = n % 8 == 0 and ldx % 8 == 0 and ldy % 8 == 0 and (x_off * 2) % 16 == 0 and (y_off * 2) % 16 == 0
    v = 8 if wide else 1
    g = pick_group(n, v)
    if g < 64:
        return g, v, 1
    chunks = -(-n // (64 * v))
    return g, v, 1 if chunks <= 1 else 2 if chunks == 2 else 4 if chunks <= 4 else 0


def tag_of(acc, n, ldx=None, ldy=None, x_off=0, y_off=0, out_bf16=False):
    g, v, c = pick(n, ldx, ldy, x_off, y_off)
    return f"sddmm_csr_bf16<{MODES[acc]},G{g},V{v},C{c}> {'bf16' if out_bf16 else 'f32'}"


def head(tag):
    """The instance of a mispmm_last_kernel() string: its out type dropped."""
    return tag.split(" ")[0]


# ------------------------------------------------------------------------------------------------ ALGORITHM
def restate(acc, row_ptrs, col_idxs, x_bits, y_bits, n=None, v=None, fault=None):
    """out [nnz] float32 as the kernel computes it.  x_bits [M, ldx], y_bits [K, ldy] bf16 bits of which the first n columns
    are the operands (n defaults to all).  v: the lane width, 8 or 1; by default the rule's for contiguous aligned operands
    of n columns.  fault: one of FAULTS, a deliberate breach of ALGORITHM."""
    assert fault is None or fault in FAULTS, fault
    x_bits, y_bits = np.asarray(x_bits), np.asarray(y_bits)
    n = x_bits.shape[1] if n is None else n
    if v is None:
        v = pick(n)[1]
    rows, cols = entry_rows(row_ptrs), np.asarray(col_idxs, dtype=np.int64)
    nnz = rows.shape[0]
    if n == 0 or nnz == 0:
        return np.zeros(nnz, np.float32)
    g = pick_group(n, v)
    chunks = -(-n // (g * v))
    width = n
    if fault == "read_gap":                              # the columns behind N of a strided operand taken as columns
        width = min(x_bits.shape[1], y_bits.shape[1], chunks * g * v)
    xrows = (rows + 1) % x_bits.shape[0] if fault == "x_next_row" else rows
    x = np.zeros((nnz, chunks * g * v), np.float32)     # a dropped load returns zeros: 0 * 0 = +0
    y = np.zeros((nnz, chunks * g * v), np.float32)
    x[:, :width] = widen(x_bits[:, :width])[xrows]
    y[:, :width] = widen(y_bits[:, :width])[cols]
    if fault == "swap_halves" and v == 8:                # y's element 2i taken from the high half of dword i
        y = y.reshape(nnz, -1, 2)[:, :, ::-1].reshape(nnz, -1)
    if fault == "drop_last_chunk":
        x[:, (chunks - 1) * g * v:] = 0.0
    # [entry, lane, the lane's columns in ascending order]
    lanes = lambda a: a.reshape(nnz, chunks, g, v).transpose(0, 2, 1, 3).reshape(nnz, g, chunks * v)   # noqa: E731
    x, y = lanes(x), lanes(y)
    f32 = acc == "fast" or fault == "ref_in_f32"
    s = np.zeros((nnz, g), np.float32 if f32 else np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i in range(chunks * v):
            t = s.astype(np.float64) + x[:, :, i].astype(np.float64) * y[:, :, i].astype(np.float64)
            s = t.astype(np.float32) if f32 else t
        lane = np.arange(g)
        steps = [1 << k for k in range(g.bit_length() - 1)]
        for k in (steps[::-1] if fault == "tree_high_first" else steps):
            s = s + s[:, lane ^ k]
        out = s[:, 0].astype(np.float32)
    if fault == "drop_eighth_slot":
        rp = np.asarray(row_ptrs, dtype=np.int64)
        slot = np.arange(nnz) - rp[rows]
        full = (slot // 8) * 8 + 8 <= np.diff(rp)[rows]
        out[(slot % 8 == 7) & full] = 0.0
    return out


def rounded_exact(row_ptrs, col_idxs, x_bits, y_bits):
    """(the correctly rounded fp32 value of the real-number sum, exact, S) per entry, for operands whose exact sums fit 53 bits
    (sddmm_exact sums in 64-bit mantissas where the platform has them, in float64 elsewhere: exact either way then)."""
    exact, scale = sddmm_exact(row_ptrs, col_idxs, widen(x_bits), widen(y_bits))
    with np.errstate(over="ignore"):
        return exact.astype(np.float32), exact, scale


# ------------------------------------------------------------------------------------------------ operands
def operands(rng, shape, spread=4):
    """bf16 bits with 8 significant bits (a full bf16 mantissa), random signs, exponents -spread .. spread.  spread = 4:
    every exact sum up to N = 2056 fits 53 bits (16 product bits + 17 of exponent spread + 12); spread = 40: it does not
    (Case.far builds the operands on which the order of a REFERENCE sum shows)."""
    sign = rng.integers(0, 2, shape).astype(np.uint16) << np.uint16(15)
    expo = (rng.integers(-spread, spread + 1, shape) + 127).astype(np.uint16) << np.uint16(7)
    return sign | expo | rng.integers(0, 128, shape).astype(np.uint16)


MAX_N = 2056


class Case:
    """A CSR pattern with operands of MAX_N columns (a case of N columns is their leading N columns) and, per (acc, N), the
    restatement and the correctly rounded exact sum, computed once and read-only."""

    def __init__(self, name, csr, seed, max_n=MAX_N):
        rng = np.random.default_rng(seed)
        self.name, self.csr = name, csr
        self.row_ptrs, self.col_idxs = np.asarray(csr.row_ptrs, np.uint32), np.asarray(csr.col_idxs, np.uint32)
        self.x_bits = operands(rng, (csr.num_rows, max_n))
        self.y_bits = operands(rng, (csr.num_cols, max_n))
        self._x_far = operands(rng, (csr.num_rows, 128), spread=40)
        self._y_far = operands(rng, (csr.num_cols, 128), spread=40)

    def far(self, n):
        """(x_bits, y_bits) of n columns, 16 <= n <= 264, whose REFERENCE sums do not fit a double: h = (n - 8) // 2 columns of
        exponents -40 .. 40, the same h columns again in REVERSED order with y negated (in the same order the lanes' sums
        would cancel to the bit), and n - 2 h columns of the near operands.  The exact sum
        is that of the last columns alone; what an fp64 chain leaves of the others depends on its order."""
        h = (n - 8) // 2
        x = np.concatenate([self._x_far[:, :h], self._x_far[:, :h][:, ::-1], self.x_bits[:, :n - 2 * h]], axis=1)
        y = np.concatenate([self._y_far[:, :h], self._y_far[:, :h][:, ::-1] ^ np.uint16(0x8000), self.y_bits[:, :n - 2 * h]], axis=1)
        return np.ascontiguousarray(x), np.ascontiguousarray(y)

    @functools.lru_cache(maxsize=None)
    def expected(self, acc, n, v=None, far=False):
        x, y = self.far(n) if far else (self.x_bits[:, :n], self.y_bits[:, :n])
        out = restate(acc, self.row_ptrs, self.col_idxs, x, y, v=v)
        out.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def exact(self, n):
        out = rounded_exact(self.row_ptrs, self.col_idxs, self.x_bits[:, :n], self.y_bits[:, :n])
        for a in out:
            a.setflags(write=False)
        return out


def _census():
    """70 x 90, rows of 0-12 entries, the first and the last empty: short rows, more than one workgroup at every G."""
    from _sddmm_ref import _csr
    rng = np.random.default_rng(23)
    lens = rng.integers(0, 13, 70)
    lens[[0, 69]] = 0
    lens[5] = 8                                          # a full batch
    return _csr(70, 90, lens, rng)


@functools.lru_cache(maxsize=None)
def case(name):
    """census | ragged | long | unsorted | tall | flat (the last five: _sddmm_ref.matrix)."""
    from _sddmm_ref import matrix
    if name == "census":
        return Case(name, _census(), 51)
    return Case(name, matrix(name), 52, max_n=40)
