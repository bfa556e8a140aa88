"""The fused CSR attention contract (include/mispmm_attn_csr.h) for the tests: the cases and operands the CPU and GPU tests
share, a float64 masked attention with heads and bias, the algorithm AS BUILT restated in numpy float32 (`fused_f32`), the two
tolerances, and the table of kernel tags.

    z[h][e]   = fma(scale, <q[h][r], k[h][c]>, bias[h][e])         r, c the row and column of entry e
    out[h][r] = sum_e softmax_e(z) v[h][c]                          lse[h][r] = log sum_e exp z

OPERANDS.  q and k are multiples of 2^-8 of magnitude in [0.25, 0.75], so sum |q||k| <= 144 < 2^8 at D = 256 and every score
is exact in fp32 in any order (asserted per case by tests/_attn_csr_tight.py); the scale is the power of two nearest D ** -0.5;
a bias is a multiple of 2^-8.  v has full mantissas.  The cases are therefore at once cases for the composed tolerance and
for the derived tight check.  Rounded scores are met by the test against the four-launch chain (full mantissas throughout).
`finite` bias: uniform in [-4, 4) plus a row offset of 0, +200 or -200 (a softmax does not see it; an exponential taken
against a maximum that was never raised does).  `masked`: the same with -Inf on a fifth of the entries and on the whole of
the first two batches of every second row longer than 16, the last entry of every row left finite."""
import dataclasses
import functools

import numpy as np

from _sddmm_ref import bound as sddmm_bound, entry_rows
from _softmax_bsr_ref import fma32
from _softmax_ref import LD, full_mantissa, fwd_bound, matrix, row_lengths, softmax_rows, spread

BATCH = 8
LOG2E = np.float32(1.44269504088896340736)
U = 2.0 ** -24
PATTERNS = ("edges", "ragged")
WIDTHS = ((8, 64), (64, 8), (40, 72), (3, 5), (1, 1), (128, 128), (256, 256))
BIASES = ("none", "finite", "masked")
HEADS = (1, 3)

FAULTS = ("max_never_updated", "rescale_skips_divisor", "rescale_skips_o", "last_slot_of_full_batch_dropped", "dead_slot_counts_one",
          "bias_before_scale", "head0_bias_for_every_head", "v_from_previous_keys", "lse_from_max_alone", "weights_against_old_max")
HONEST = ("exp_float64", "sums_in_another_order")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    d: int
    dv: int
    bias: str = "none"
    heads: int = 1

    @property
    def id(self):
        return f"{self.name},D{self.d},Dv{self.dv},{self.bias},H{self.heads}"


CASES = tuple(Case(n, d, dv, b, h) for n in PATTERNS for (d, dv) in WIDTHS for b in BIASES for h in HEADS)


def scale_of(d):
    """The power of two nearest D ** -0.5 (the smaller where D is an odd power of two)."""
    return 2.0 ** -int(np.ceil(np.log2(d) / 2.0))


def _grid(rng, shape):
    return (rng.choice(np.array([-1.0, 1.0]), shape) * rng.integers(64, 193, shape) / 256.0).astype(np.float32)


def make_bias(csr, kind, heads, rng):
    """None | [heads, nnz] float32 (heads = 1: the shared bias)."""
    if kind == "none":
        return None
    rows = entry_rows(csr.row_ptrs)
    b = np.floor(rng.uniform(-4.0, 4.0, (heads, csr.nnz)) * 256.0) / 256.0 + np.array([0.0, 200.0, -200.0])[rows % 3]
    if kind == "masked":
        ptrs = np.asarray(csr.row_ptrs, dtype=np.int64)
        lens = np.diff(ptrs)
        pos = np.arange(csr.nnz) - ptrs[:-1][rows]
        masked = rng.random((heads, csr.nnz)) < 0.2
        masked |= ((rows % 2 == 0) & (lens[rows] > 16) & (pos < 16))[None, :]
        masked &= (pos != lens[rows] - 1)[None, :]
        b = np.where(masked, -np.inf, b)
    return b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def operands(case):
    """dict(q [H, M, D], k [1, K, D], v [1, K, Dv], bias None | [nnz] | [H, nnz], scale): k and v are shared by the heads
    (multi-query: head stride 0), `finite` with H > 1 has a bias per head and `masked` a shared one.  Read-only."""
    csr = matrix(case.name)
    rng = np.random.default_rng(9000 + 7 * case.d + case.dv + 100 * case.heads + len(case.bias))
    q = _grid(rng, (case.heads, csr.num_rows, case.d))
    k = _grid(rng, (1, csr.num_cols, case.d))
    v = full_mantissa(rng, (1, csr.num_cols, case.dv), np.float32)
    per_head = case.heads if case.bias == "finite" else 1
    bias = make_bias(csr, case.bias, per_head, rng)
    if bias is not None and per_head == 1:
        bias = bias[0]
    res = dict(q=q, k=k, v=v, bias=bias, scale=scale_of(case.d))
    for x in res.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return res


def _head(x, h):
    return x[h if x.shape[0] > 1 else 0]


def _bias_of(bias, h, nnz, fault=None):
    if bias is None:
        return np.zeros(nnz, np.float32)
    if bias.ndim == 1:
        return bias
    return bias[0 if fault == "head0_bias_for_every_head" else h]


# ---- float64
def scores_f64(csr, q, k, scale, bias, h):
    """(z, S) per entry for head h in float64: z = scale <q, k> + bias, S = scale sum |q||k| + |finite bias|."""
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    qs = _head(q, h).astype(np.float64) * scale
    kk = _head(k, h).astype(np.float64)
    b = _bias_of(bias, h, csr.nnz).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        z = (qs[rows] * kk[cols]).sum(axis=1) + b
        s_abs = (np.abs(qs[rows]) * np.abs(kk[cols])).sum(axis=1) + np.where(np.isfinite(b), np.abs(b), 0.0)
    return z, s_abs


def attention_f64(csr, q, k, v, scale, bias=None):
    """(out [H, M, Dv], lse [H, M]) in float64: masked attention on the pattern, entry by entry, so that a (row, column) pair
    stored twice counts twice; special values as numpy has them, which are torch's.  An empty row: a zero row and -Inf."""
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    heads = q.shape[0]
    out = np.zeros((heads, csr.num_rows, v.shape[2]))
    lse = np.full((heads, csr.num_rows), -np.inf)
    for h in range(heads):
        z, _ = scores_f64(csr, q, k, scale, bias, h)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            p = softmax_rows(csr.row_ptrs, z).astype(np.float64)
            np.add.at(out[h], rows, p[:, None] * _head(v, h).astype(np.float64)[cols])
            top = np.full(csr.num_rows, -np.inf)
            np.fmax.at(top, rows, z)
            shift = np.where(np.isinf(top), 0.0, top)
            total = np.zeros(csr.num_rows)
            np.add.at(total, rows, np.exp(z - shift[rows]))
            lens = np.diff(np.asarray(csr.row_ptrs, dtype=np.int64))
            lse[h] = np.where(lens > 0, shift + np.log(total), -np.inf)
    return out, lse


def dense_f64(csr, q, k, v, scale, bias=None):
    """The same through dense [M, K] matrices (no pair stored twice): what `attention_f64` is held equal to on the CPU."""
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    heads = q.shape[0]
    out = np.zeros((heads, csr.num_rows, v.shape[2]))
    for h in range(heads):
        z = np.full((csr.num_rows, csr.num_cols), -np.inf)
        s = (_head(q, h).astype(np.float64) * scale) @ _head(k, h).astype(np.float64).T
        z[rows, cols] = s[rows, cols] + _bias_of(bias, h, csr.nnz).astype(np.float64)
        top = z.max(axis=1, keepdims=True)
        with np.errstate(invalid="ignore"):
            e = np.exp(z - np.where(np.isinf(top), 0.0, top))
            p = np.where(np.isneginf(top), 0.0, e / np.where(np.isneginf(top), 1.0, e.sum(axis=1, keepdims=True)))
        out[h] = p @ _head(v, h).astype(np.float64)
    return out


# ---- the tolerances
def out_tolerance(csr, q, k, v, scale, bias=None):
    """[H, M, Dv]: the `out` component of tests/test_gpu_softmax.py::_attention_tolerances with acc="fast", nothing added,
    restated for heads and a bias.  There u2 = 2 u is the two roundings of q' = fl(q * fl(scale)); here the scale multiplies S
    inside one fma with the bias, so the u2 terms go from q' to z: they stand on |scale| sum |q||k| + |bias| (one rounding of the
    fma, one of the scale).  Without a bias the numbers are the original's.  A -Inf bias is exact: its entry has no error."""
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    length = row_lengths(csr.row_ptrs)
    u2 = 2 * U
    tol = np.zeros((q.shape[0], csr.num_rows, v.shape[2]))
    for h in range(q.shape[0]):
        z, s_abs = scores_f64(csr, q, k, scale, bias, h)
        live = ~np.isneginf(z)
        e_s = np.where(live, sddmm_bound(np.float32, "fast", q.shape[2], np.where(live, z, 0.0), s_abs * (1 + u2)) + u2 * s_abs, 0.0)
        p = softmax_rows(csr.row_ptrs, z).astype(np.float64)
        e_row = np.zeros(csr.num_rows)
        np.maximum.at(e_row, rows, e_s)
        shift = np.expm1(2 * e_row[rows])
        e_p = p * shift + fwd_bound(np.float32, "fast", length, spread(csr.row_ptrs, z) + 2 * e_row[rows], p * (1 + shift))
        va = np.abs(_head(v, h)).astype(np.float64)[cols]
        np.add.at(tol[h], rows, (1e-5 * (p + e_p) + e_p)[:, None] * va)
    return 1.01 * tol + 1e-30


def lse_tolerance(csr, q, k, scale, bias=None):
    """[H, M]: E_z + (L + 8 T + 16) 2^-24 + 2 2^-24 (|lse| + ln L + 1), times 1.01 -- the header's bound, derived as that of
    mispmm_attn.h: E_z the largest score error of the row, the SDDMM's FAST bound on |scale| sum |q||k| plus the fma's rounding."""
    rows = entry_rows(csr.row_ptrs)
    lens = np.diff(np.asarray(csr.row_ptrs, dtype=np.int64)).astype(np.float64)
    tol = np.zeros((q.shape[0], csr.num_rows))
    v1 = np.zeros((1, csr.num_cols, 1), np.float32)
    lse = attention_f64(csr, q, k, v1, scale, bias)[1]
    for h in range(q.shape[0]):
        z, s_abs = scores_f64(csr, q, k, scale, bias, h)
        live = ~np.isneginf(z)
        e_s = np.where(live, sddmm_bound(np.float32, "fast", q.shape[2], np.where(live, z, 0.0), s_abs * (1 + 2 * U)) + 2 * U * s_abs, 0.0)
        e_row, t_row = np.zeros(csr.num_rows), np.zeros(csr.num_rows)
        np.maximum.at(e_row, rows, e_s)
        np.maximum.at(t_row, rows, spread(csr.row_ptrs, z))
        with np.errstate(invalid="ignore", divide="ignore"):
            tol[h] = e_row + (lens + 8 * t_row + 16) * U + 2 * U * (np.abs(np.where(np.isfinite(lse[h]), lse[h], 0.0)) + np.log(np.maximum(lens, 1)) + 1)
    return 1.01 * tol


# ---- the algorithm as built
def batch_table(csr):
    """(idx [M, nb * 8] entry of every slot (0 where dead), live [M, nb * 8], batches [M]) of the rows padded to whole batches."""
    ptrs = np.asarray(csr.row_ptrs, dtype=np.int64)
    lens = np.diff(ptrs)
    nb = max(1, int(-(-lens.max(initial=0) // BATCH)))
    pos = np.arange(nb * BATCH)[None, :]
    live = pos < lens[:, None]
    return np.where(live, ptrs[:-1, None] + pos, 0), live, -(-lens // BATCH)


def _exp32(t, in64):
    """v_exp_f32(fl(t * fl(log2 e))) restated with np.exp2; in64: the exponential in float64, rounded once."""
    t = np.asarray(t, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if in64:
            return np.exp(t.astype(np.float64)).astype(np.float32)
        return np.exp2(t * LOG2E)


def scores_f32(csr, q, k, scale, bias, h, fault=None):
    """z per entry in float32.  S is restated as the correctly rounded dot product: the kernel's fma chain and tree differ from
    it inside the SDDMM's FAST bound, and on exact-score operands not at all."""
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (_head(q, h).astype(np.float64)[rows] * _head(k, h).astype(np.float64)[cols]).sum(axis=1).astype(np.float32)
        b = _bias_of(bias, h, csr.nnz, fault)
        if fault == "bias_before_scale":
            return np.float32(scale) * (s + b)
        return fma32(np.float32(scale), s, b)


def fused_f32(csr, q, k, v, scale, bias=None, fault=None):
    """(out [H, M, Dv], lse [H, M]) in float32, batch by batch as attn_csr.hip goes: the same batch of 8, the running maximum
    folded per batch, mu = m or 0, alpha exactly 1 while m is -Inf, the weights' tree ((w0 + w1) + (w2 + w3)) + ((w4 + w5) +
    (w6 + w7)), l = fl(fl(l * alpha) + t), O = fl(alpha * O) then one fma per entry in order, O / l, mu + log l.
    fault: None, one of FAULTS (a deliberate mistake, tests/_attn_csr_mutants.py) or of HONEST (a variant that keeps the
    header's words)."""
    if fault is not None and fault not in FAULTS and fault not in HONEST:
        raise ValueError(f"unknown fault {fault!r}")
    f32 = np.float32
    idx, live, batches = batch_table(csr)
    cols = np.asarray(csr.col_idxs, dtype=np.int64)
    heads, m_rows, dv = q.shape[0], csr.num_rows, v.shape[2]
    out, lse = np.zeros((heads, m_rows, dv), f32), np.full((heads, m_rows), -np.inf, f32)
    ninf = f32(-np.inf)
    nb = idx.shape[1] // BATCH
    for h in range(heads):
        z = scores_f32(csr, q, k, scale, bias, h, fault)
        zt = np.where(live, z[idx] if csr.nnz else ninf, ninf).astype(f32)
        vg = np.where(live[:, :, None], _head(v, h)[cols[idx]] if csr.nnz else 0.0, 0.0).astype(f32)
        m, mu, l = np.full(m_rows, ninf), np.zeros(m_rows, f32), np.zeros(m_rows, f32)
        o = np.zeros((m_rows, dv), f32)
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            for b in range(nb):
                sl = slice(b * BATCH, (b + 1) * BATCH)
                active = b < batches
                zb, lv = zt[:, sl].copy(), live[:, sl]
                vb = vg[:, slice(max(b - 1, 0) * BATCH, max(b, 1) * BATCH) if fault == "v_from_previous_keys" else sl]
                if fault == "last_slot_of_full_batch_dropped":
                    zb[lv.all(axis=1), BATCH - 1] = ninf
                m_new = m if fault == "max_never_updated" else np.fmax(m, np.fmax.reduce(zb, axis=1))
                mu_new = np.where(np.isinf(m_new), f32(0), m_new).astype(f32)
                alpha = np.where(np.isneginf(m), f32(1), _exp32(mu - mu_new, fault == "exp_float64")).astype(f32)
                w = _exp32(zb - (mu if fault == "weights_against_old_max" else mu_new)[:, None], fault == "exp_float64")
                wd = np.where(lv, w, f32(1)) if fault == "dead_slot_counts_one" else w
                if fault == "sums_in_another_order":
                    t = wd[:, 7]
                    for j in range(6, -1, -1):
                        t = t + wd[:, j]
                else:
                    t = ((wd[:, 0] + wd[:, 1]) + (wd[:, 2] + wd[:, 3])) + ((wd[:, 4] + wd[:, 5]) + (wd[:, 6] + wd[:, 7]))
                l_new = (l if fault == "rescale_skips_divisor" else l * alpha) + t
                o_new = o if fault == "rescale_skips_o" else o * alpha[:, None]
                for j in (range(BATCH - 1, -1, -1) if fault == "sums_in_another_order" else range(BATCH)):
                    o_new = fma32(w[:, j, None], vb[:, j, :], o_new)
                m, mu = np.where(active, m_new, m), np.where(active, mu_new, mu)
                l, o = np.where(active, l_new, l).astype(f32), np.where(active[:, None], o_new, o).astype(f32)
            stored = batches > 0
            out[h] = np.where(stored[:, None], o / np.where(stored, l, f32(1))[:, None], f32(0))
            lse[h] = np.where(stored, mu if fault == "lse_from_max_alone" else mu + np.log(l), ninf)
    return out, lse


# ---- the kernel tags
def tag_of(d, dv, aligned):
    """mispmm_last_kernel() for (D, Dv, operands 16-byte aligned with strides in multiples of 4): the host's choice restated."""
    vec = 4 if aligned and d % 4 == 0 and dv % 4 == 0 else 1
    need = -(-max(d, dv) // vec)
    g = next((x for x in (8, 16, 32, 64) if x >= need), 64)
    chunks = 1 if g < 64 else -(-max(d, dv) // (64 * vec))
    return f"attn_csr<f32,G{g},V{vec},C{1 if chunks <= 1 else 2 if chunks == 2 else 4}>"


# tag -> the smallest (D, Dv, aligned) that reaches it
TAGS = {
    "attn_csr<f32,G8,V4,C1>": (4, 4, True), "attn_csr<f32,G16,V4,C1>": (4, 36, True), "attn_csr<f32,G32,V4,C1>": (4, 68, True),
    "attn_csr<f32,G64,V4,C1>": (4, 132, True),
    "attn_csr<f32,G8,V1,C1>": (1, 1, False), "attn_csr<f32,G16,V1,C1>": (1, 9, False), "attn_csr<f32,G32,V1,C1>": (1, 17, False),
    "attn_csr<f32,G64,V1,C1>": (1, 33, False), "attn_csr<f32,G64,V1,C2>": (1, 65, False), "attn_csr<f32,G64,V1,C4>": (1, 129, False),
}
