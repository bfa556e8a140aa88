"""The fused block-sparse attention backward (include/mispmm_attn_bwd.h) for the tests: the six patterns (the four of
tests/_attn_fused_ref.py and the transposes of the two `edges` patterns, whose block COLUMNS then hold 0, 1, 2, 3, 4, 5, 8, 9,
C - 1, C, C + 1 and 2C + 1 blocks, empty ones first and last), masks and operands, the table of kernel tags, the derived
tolerance bwd_tolerances, and the backward AS BUILT restated in numpy float32.

bwd_tolerances: first-order propagation in float64, in the manner of
tests/test_gpu_softmax_bsr.py::_attention_tolerances and with its constants: r8 = 2^-8 per rounding to bf16, g_n = n 2^-23 /
(1 - n 2^-23) for an fp32 dot product of n terms in any order, the SDDMM bound of mispmm.h, u = 2^-24, every propagated factor
evaluated at (value + its own error), and 1.01 on the whole; evaluated on arrays over A's stored elements, block by block.
With z, lse, P = exp(z - lse), dP = <dO, V>, delta = <dO, O>, dS = scale P (dP - delta) in real arithmetic on the bf16 inputs:
    E_z      scale E_s + u |scale s| + u |z|                     the forward's z: SDDMM over D terms, rounded scale, the fma
    E_lse    max_row E_z + (L + 8 T + 16) u + 2 u (|lse| + ln L + 1)                                  mispmm_attn.h
    E_P      P expm1(E_a) + (3 t + 2) u P exp(E_a) + 2^-126,  E_a = E_z + E_lse, t = |z - lse| + E_a     the difference, the product
             with log2 e and v_exp_f32, as mispmm_softmax_bsr_f32 counts them; where P enters dV: + r8 (P + E_P)
    E_dP     SDDMM bound over Dv terms (+ <E_g, |V|> where grad_out was rounded from float32, E_g = r8 |dO|)
    E_delta  g_Dv sum (|dO| + E_g)(|O| + E_out) + sum (|dO| + E_g) E_out + sum E_g |O|     E_out: the forward's `out` tolerance for the out
             type in use (the `out` component of _attention_tolerances, evaluated block by block here).  The three-launch chain has
             no such term: its dS uses <P, dP> of the P it read.
    E_dS     scale (E_P X + P (E_dP + E_delta)) + (4 u + r8) scale (P + E_P) X + 2^-126,  X = |dP - delta| + E_dP + E_delta
             four fp32 roundings (the difference, two products, the fp32 scale), then one rounding to bf16
    dQ       sum_key E_dS |K| + g_L sum (|dS| + E_dS) |K|,  L the keys of the row;  dK, dV: the same over the rows that store the
             key, dV with P (+ sum P E_g |.| where grad_out was rounded); a bf16 gradient: + r8 (|exact| + tolerance).

forward_f32, delta_f32, _weights and backward_f32 take `fault=`: a name of tests/_attn_mutants.py, a deliberate breach of the header
put into THIS code and not a copy of it, for tests/test_attn_mutants_cpu.py; None (the default) is the algorithm and keeps its bits."""
import functools
import itertools

import numpy as np

from mispmm import formats, ops

import _attn_mutants
from _attn_fused_ref import _exp32, bf16_trunc, fused_rows, mfma_add
from _sddmm_bsr_ref import bound as sddmm_bsr_bound, full_mantissa as bf16_full_mantissa
from _softmax_bsr_ref import bf16_round, fma32, fwd_bound, pattern

PATTERNS = ["ragged16", "ragged32", "edges16", "edges32", "edgesT16", "edgesT32"]
WIDTHS = [(8, 64), (64, 8), (128, 128), (40, 72)]
MASKS = ["none", "causal", "leading"]


@functools.lru_cache(maxsize=None)
def bwd_pattern(name):
    """(bsr of A, bsr of A^T, perm).  edgesT16 | edgesT32: the transposes of edges16 | edges32.  Read-only."""
    if name.startswith("edgesT"):
        a = ops.bsr_transpose(pattern("edges" + name[len("edgesT"):]))[0]
        a = formats.BSR(a.num_rows, a.num_cols, a.nnz, a.block_row_size, a.block_col_size, a.block_row_ptrs, a.block_col_idxs,
                        np.zeros((a.num_blocks, a.block_row_size, a.block_col_size), np.float32))
    else:
        a = pattern(name)
        if name == "ACTIVSg10K":                                # the index alone is kept there; no value is read here either
            a = formats.BSR(a.num_rows, a.num_cols, a.nnz, a.block_row_size, a.block_col_size, a.block_row_ptrs, a.block_col_idxs,
                            np.zeros((a.num_blocks, a.block_row_size, a.block_col_size), np.float32))
    at, perm = ops.bsr_transpose(a)
    return a, at, perm


@functools.lru_cache(maxsize=None)
def mask_of(name, kind):
    """none | causal (-Inf above the diagonal inside the blocks on the diagonal) | leading (-Inf over the whole of the first
    ceil(n / 2) blocks of every block row of n >= 2 blocks), as tests/_attn_fused_ref.py has them.  Read-only."""
    if kind == "none":
        return None
    a = bwd_pattern(name)[0]
    bs = a.block_row_size
    ptrs = np.asarray(a.block_row_ptrs, dtype=np.int64)
    m = np.zeros((a.num_blocks, bs, bs), np.float32)
    if kind == "causal":
        rows = np.repeat(np.arange(ptrs.shape[0] - 1), np.diff(ptrs))
        diag = np.asarray(a.block_col_idxs, dtype=np.int64) == rows
        m[diag] = np.where(np.triu(np.ones((bs, bs), bool), k=1), -np.inf, 0.0).astype(np.float32)
        return m
    assert kind == "leading"
    for lo, hi in zip(ptrs[:-1], ptrs[1:]):
        if hi - lo >= 2:
            m[lo:lo + (hi - lo + 1) // 2] = -np.inf
    return m


@functools.lru_cache(maxsize=None)
def operands(name, d, dv, heads=1):
    """(q, k, v, grad_out) float32 arrays of bf16 numbers, [H, rows, width].  Read-only."""
    a = bwd_pattern(name)[0]
    rng = np.random.default_rng(700 + d + 7 * dv + 1000 * heads)
    return (bf16_full_mantissa(rng, (heads, a.num_rows, d)), bf16_full_mantissa(rng, (heads, a.num_cols, d)),
            bf16_full_mantissa(rng, (heads, a.num_cols, dv)), bf16_full_mantissa(rng, (heads, a.num_rows, dv)))


# ---- tags
def _shape_tag(bs, d, dv, mask):
    return f"<b{bs},{'mask' if mask else 'nomask'},D{2 if d <= 64 else 4},V{2 if dv <= 64 else 4}>"


def rows_tag(bs, d, dv, mask):
    return "attn_bsr_bwd_rows" + _shape_tag(bs, d, dv, mask)


def cols_tag(bs, d, dv, mask):
    return "attn_bsr_bwd_cols" + _shape_tag(bs, d, dv, mask)


def tag_of(bs, d, dv, mask, need=(True, True, True)):
    """mispmm_last_kernel() after a call: the launches made, joined.  The row pass runs with dq or dk, the column pass with dk or dv."""
    made = ([rows_tag(bs, d, dv, mask)] if need[0] or need[1] else []) + ([cols_tag(bs, d, dv, mask)] if need[1] or need[2] else [])
    return " + ".join(made)


# every tag the dispatcher can form -> the smallest (bS, D, Dv, mask) that reaches it (the types of out and of the gradients
# are run-time branches of an instance, not instances)
TAGS = {}
for _bs, _d, _dv, _mask in itertools.product((16, 32), (8, 72), (8, 72), (False, True)):
    TAGS[rows_tag(_bs, _d, _dv, _mask)] = (_bs, _d, _dv, _mask)
    TAGS[cols_tag(_bs, _d, _dv, _mask)] = (_bs, _d, _dv, _mask)


# ---- block-wise helpers: arrays over A's stored elements, [num_blocks, bS, bS], so that ACTIVSg10K can be had too
class _Blocks:
    def __init__(self, name):
        a, at, perm = bwd_pattern(name)
        self.a, self.bs, self.nb = a, a.block_row_size, a.num_blocks
        self.ptrs = np.asarray(a.block_row_ptrs, dtype=np.int64)
        self.tptrs = np.asarray(at.block_row_ptrs, dtype=np.int64)
        self.perm = np.asarray(perm, dtype=np.int64)
        self.rows_of = np.repeat(np.arange(self.ptrs.shape[0] - 1), np.diff(self.ptrs))
        self.cols_of = np.asarray(a.block_col_idxs, dtype=np.int64)
        self.within = np.arange(self.bs)
        self.chunks = [slice(lo, min(lo + 4096, self.nb)) for lo in range(0, self.nb, 4096)]
        self.n_row = np.repeat(np.diff(self.ptrs) * self.bs, self.bs).astype(np.float64)           # keys of a matrix row
        self.n_col = np.repeat(np.diff(self.tptrs) * self.bs, self.bs).astype(np.float64)          # rows that store a key

    def sampled(self, x, y):                                   # [num_blocks, bS, bS]: <x_r, y_c>
        out = np.empty((self.nb, self.bs, self.bs))
        for c in self.chunks:
            out[c] = np.matmul(x[self.rows_of[c, None] * self.bs + self.within], y[self.cols_of[c, None] * self.bs + self.within].transpose(0, 2, 1))
        return out

    def _gathered(self, per, ptrs, count):
        out = np.zeros((count, self.bs, per.shape[2]))
        filled = np.diff(ptrs) > 0
        if per.shape[0]:
            out[filled] = np.add.reduceat(per, ptrs[:-1][filled], axis=0)
        return out.reshape(-1, per.shape[2])

    def times(self, blocks, y):                                # [M, n]: (the block array as a matrix) @ y
        per = np.empty((self.nb, self.bs, y.shape[1]))
        for c in self.chunks:
            per[c] = np.matmul(blocks[c], y[self.cols_of[c, None] * self.bs + self.within])
        return self._gathered(per, self.ptrs, self.ptrs.shape[0] - 1)

    def times_t(self, blocks, x):                              # [K, n]: (the block array as a matrix)^T @ x
        per = np.empty((self.nb, self.bs, x.shape[1]))
        for c in self.chunks:
            per[c] = np.matmul(blocks[c].transpose(0, 2, 1), x[self.rows_of[c, None] * self.bs + self.within])
        return self._gathered(per[self.perm], self.tptrs, self.tptrs.shape[0] - 1)

    def row_reduce(self, blocks, ufunc, empty):                # [M]: ufunc over the stored elements of every matrix row
        inner = ufunc.reduce(blocks, axis=2)                   # [num_blocks, bS]
        out = np.full((self.ptrs.shape[0] - 1, self.bs), empty, dtype=np.float64)
        filled = np.diff(self.ptrs) > 0
        if inner.shape[0]:
            out[filled] = ufunc.reduceat(inner, self.ptrs[:-1][filled], axis=0)
        return out.reshape(-1)

    def of_row(self, vec):                                     # a per-row value beside every stored element of the row
        return vec.reshape(-1, self.bs)[self.rows_of][:, :, None]


@functools.lru_cache(maxsize=None)
def _blocks(name):
    return _Blocks(name)


def bwd_tolerances(name, q, k, v, g, scale, mask, out_bf16, grads_bf16, g_rounded=False):
    """(tol_dq [M, D], tol_dk [K, D], tol_dv [K, Dv]) in float64: the module docstring, formula for formula, on arrays over A's
    stored elements."""
    f64 = np.float64
    b = _blocks(name)
    q, k, v, g = (x.astype(f64) for x in (q, k, v, g))
    u, r8 = 2.0 ** -24, 2.0 ** -8
    gamma = lambda n: n * 2.0 ** -23 / (1.0 - n * 2.0 ** -23)                              # noqa: E731
    s, s_abs = b.sampled(q, k), b.sampled(np.abs(q), np.abs(k))
    z = scale * s + (0.0 if mask is None else mask.astype(f64))
    live = np.isfinite(z)
    zf = np.where(live, z, 0.0)
    e_z = np.where(live, scale * sddmm_bsr_bound(False, q.shape[1], s, s_abs) + u * np.abs(scale * s) + u * np.abs(zf), 0.0)
    zr = np.where(live, z, -np.inf)
    top = b.row_reduce(zr, np.maximum, 0.0)
    top = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        lse = top + np.log(np.maximum(b.row_reduce(np.exp(zr - b.of_row(top)), np.add, 1.0), 2.0 ** -1000))
    low = b.row_reduce(np.where(live, z, np.inf), np.minimum, 0.0)
    spread = np.where(np.isfinite(low), top - low, 0.0)
    n_row, n_col = b.n_row, b.n_col
    e_row = b.row_reduce(e_z, np.maximum, 0.0)
    e_lse = e_row + (n_row + 8.0 * spread + 16.0) * u + 2.0 * u * (np.abs(lse) + np.log(np.maximum(n_row, 1.0)) + 1.0)
    arg = np.where(live, z - b.of_row(lse), 0.0)
    p = np.where(live, np.exp(arg), 0.0)
    # P of the backward: exp of an argument off by at most E_z + E_lse, then the kernel's own roundings
    e_arg = e_z + b.of_row(e_lse)
    t = np.abs(arg) + e_arg
    e_p = np.where(live, p * np.expm1(e_arg) + (3.0 * t + 2.0) * u * p * np.exp(e_arg) + 2.0 ** -126, 0.0)
    # the forward's tolerance on out, as _attention_tolerances composes it (P normalised by the row's sum, rounded to bf16)
    shift = np.expm1(2.0 * b.of_row(e_row))
    e_pf = np.where(live, p * shift + fwd_bound(True, b.of_row(n_row), b.of_row(spread + 2.0 * e_row), p * (1.0 + shift)), 0.0)
    out = b.times(p, v)
    e_out = gamma(n_row)[:, None] * b.times(p + e_pf, np.abs(v)) + b.times(e_pf, np.abs(v))
    if out_bf16:
        e_out = e_out + r8 * (np.abs(out) + e_out)
    e_out = 1.01 * e_out + 1e-30
    e_g = r8 * np.abs(g) if g_rounded else np.zeros_like(g)
    gh = np.abs(g) + e_g
    dp, dp_abs = b.sampled(g, v), b.sampled(gh, np.abs(v))
    e_dp = sddmm_bsr_bound(False, v.shape[1], dp, dp_abs) + b.sampled(e_g, np.abs(v))
    delta = np.sum(g * out, axis=1)
    e_delta = gamma(float(v.shape[1])) * np.sum(gh * (np.abs(out) + e_out), axis=1) + np.sum(gh * e_out, axis=1) + np.sum(e_g * np.abs(out), axis=1)
    diff = np.abs(dp - b.of_row(delta)) + e_dp + b.of_row(e_delta)
    ds = scale * p * (dp - b.of_row(delta))
    ds_hat = scale * (p + e_p) * diff
    e_ds = np.where(live, scale * (e_p * diff + p * (e_dp + b.of_row(e_delta))) + (4.0 * u + r8) * ds_hat + 2.0 ** -126, 0.0)
    dsh = np.abs(ds) + e_ds
    tol_dq = gamma(n_row)[:, None] * b.times(dsh, np.abs(k)) + b.times(e_ds, np.abs(k))
    tol_dk = gamma(n_col)[:, None] * b.times_t(dsh, np.abs(q)) + b.times_t(e_ds, np.abs(q))
    e_pv = np.where(live, e_p + r8 * (p + e_p), 0.0)
    tol_dv = gamma(n_col)[:, None] * b.times_t(p + e_pv, gh) + b.times_t(e_pv, gh) + b.times_t(p, e_g)
    tols = [tol_dq, tol_dk, tol_dv]
    if grads_bf16:
        exact = (b.times(ds, k), b.times_t(ds, q), b.times_t(p, g))
        tols = [tol + r8 * (np.abs(x) + tol) for x, tol in zip(exact, tols)]
    return [1.01 * x + 1e-30 for x in tols]


def chain_grad_tolerances(name, q, k, v, g, scale, mask):
    """The (dq, dk, dv) components of tests/test_gpu_softmax_bsr.py::_attention_tolerances (the three-launch chain's composed
    tolerances), formula for formula, on arrays over A's stored elements instead of densified matrices, so that they can be had
    on ACTIVSg10K; tests/test_attn_fused_bwd_cpu.py holds the two equal on the small patterns.  `name`: a pattern of
    _softmax_bsr_ref.pattern."""
    from _softmax_bsr_ref import bwd_bound, forward, layout, lengths, to_rows
    f64 = np.float64
    b = _blocks(name)
    q, k, v, g = (x.astype(f64) for x in (q, k, v, g))
    r8 = 2.0 ** -8
    gamma = lambda n: n * 2.0 ** -23 / (1.0 - n * 2.0 ** -23)                              # noqa: E731
    length = lengths(name).astype(f64)
    row_ptrs, idx = layout(name)

    def per_row(blocks, ufunc=np.add):
        vr = to_rows(name, blocks)
        lens = np.diff(row_ptrs)
        red = ufunc.reduceat(vr, row_ptrs[:-1][lens > 0])
        flat = np.empty(blocks.size)
        flat[idx] = np.repeat(red, lens[lens > 0])
        return flat.reshape(blocks.shape)

    s, s_abs = b.sampled(q, k), b.sampled(np.abs(q), np.abs(k))
    e_s = sddmm_bsr_bound(False, q.shape[1], s, s_abs)
    z = scale * s + (0.0 if mask is None else mask.astype(f64))
    finite = np.isfinite(z)
    e_z = np.where(finite, scale * e_s + 2.0 ** -24 * np.abs(scale * s) + 2.0 ** -24 * np.abs(np.where(finite, z, 0.0)), 0.0)
    p, t = forward(name, np.where(finite, z, -np.inf), f64)
    e_row = per_row(e_z, np.maximum)
    shift = np.expm1(2 * e_row)
    e_p = p * shift + fwd_bound(True, length, t + 2 * e_row, p * (1 + shift))
    ph = p + e_p
    n_row, n_col = b.n_row[:, None], b.n_col[:, None]
    e_g = r8 * np.abs(g)
    gh = np.abs(g) + e_g
    dv = b.times_t(p, g)
    tol_dv = gamma(n_col) * b.times_t(ph, gh) + b.times_t(e_p, gh) + b.times_t(p, e_g)
    dp, dp_abs = b.sampled(g, v), b.sampled(gh, np.abs(v))
    e_dp = sddmm_bsr_bound(False, v.shape[1], dp, dp_abs) + b.sampled(e_g, np.abs(v))
    ds = scale * p * (dp - per_row(p * dp))
    dph = np.abs(dp) + e_dp
    cap_h = per_row(ph * dph)
    e_dot = per_row(e_p * dph + ph * e_dp)
    e_ds = (bwd_bound(True, length, ph, dph, cap_h, scale, scale * ph * (dph + cap_h))
            + scale * (e_p * (dph + cap_h) + ph * (e_dp + e_dot)))
    dsh = np.abs(ds) + e_ds
    dq = b.times(ds, k)
    tol_dq = gamma(n_row) * b.times(dsh, np.abs(k)) + b.times(e_ds, np.abs(k))
    dk = b.times_t(ds, q)
    tol_dk = gamma(n_col) * b.times_t(dsh, np.abs(q)) + b.times_t(e_ds, np.abs(q))
    rounded = lambda value, tol: tol + r8 * (np.abs(value) + tol)                          # noqa: E731
    return [1.01 * x + 1e-30 for x in (rounded(dq, tol_dq), rounded(dk, tol_dk), rounded(dv, tol_dv))]


# ---- the algorithm as built, numpy float32
def _block_rows(bsr):
    ptrs = np.asarray(bsr.block_row_ptrs, dtype=np.int64)
    cols = np.asarray(bsr.block_col_idxs, dtype=np.int64)
    bs = bsr.block_row_size
    for r, (lo, hi) in enumerate(zip(ptrs[:-1], ptrs[1:])):
        yield r, lo, hi, (cols[lo:hi, None] * bs + np.arange(bs)).reshape(-1)


def forward_f32(name, q, k, v, mask, scale, fault=None):
    """tests/_attn_fused_ref.py::fused_f32 on any of the six patterns: (out [M, Dv], lse [M]) of one head, numpy float32 -- one
    body, fused_rows, behind both."""
    return fused_rows(bwd_pattern(name)[0], q, k, v, mask, scale, fault)


def delta_f32(g, out, fault=None):
    """delta as the row pass forms it: lane gq of a row sums columns 32 s + 8 gq .. + 7 of every 32-column step s ascending by fma,
    the four lanes meet as (g0 + g1) + (g2 + g3).  out: float32 (a bf16 out widened exactly)."""
    _attn_mutants.check(fault, _attn_mutants.BACKWARD)
    f32 = np.float32
    if fault == "delta_from_bf16_out":
        out = bf16_round(out)
    rows, dv = g.shape
    lane = np.zeros((rows, 4), f32)
    for s in range(0, dv, 32):
        for gq in range(4):
            for c in range(s + 8 * gq, min(s + 8 * gq + 8, dv)):
                lane[:, gq] = fma32(g[:, c], out[:, c], lane[:, gq])
    delta = (lane[:, 0] + lane[:, 1]) + (lane[:, 2] + lane[:, 3])
    return delta * f32(1 + 2.0 ** -9) if fault == "delta_scaled" else delta


def _weights(z, dp, lse, delta, scale, fault=None):
    """(bf16 P, bf16 dS) as float32 arrays; lse, delta broadcast against z."""
    _attn_mutants.check(fault, _attn_mutants.BACKWARD)
    f32 = np.float32
    if fault == "lse_shifted":
        lse = lse + f32(2.0 ** -9)
    with np.errstate(invalid="ignore", over="ignore"):
        p = _exp32(z - lse, fault)
        pin = bf16_round(p) if fault == "p_bf16_before_ds" else p
        ds = (pin * (dp - delta).astype(f32)).astype(f32) * f32(scale)
    return (bf16_trunc(p) if fault == "p_truncated" else bf16_round(p)), (bf16_trunc(ds) if fault == "ds_truncated" else bf16_round(ds))


def backward_f32(name, q, k, v, g, out, lse, mask, scale, grads_bf16, fault=None):
    """(dq, dk, dv) of one head by the two passes as built, in numpy float32: 32-key resp. 32-query steps in storage order, P and
    dS rounded to bf16 before the second products, fp32 accumulators from +0.  The sum inside an MFMA is taken in float64 and
    rounded once (the order inside the instruction is its own).  out, lse: what the forward stored (float32 arrays).  g: grad_out;
    a float32 one is rounded to bf16 here, as the Python layer does before the call (one that holds bf16 numbers keeps its bits).
    fault: a name of tests/_attn_mutants.py (BACKWARD or HONEST); None: the algorithm."""
    _attn_mutants.check(fault, _attn_mutants.BACKWARD)
    f32, f64 = np.float32, np.float64
    a, at, perm = bwd_pattern(name)
    bs = a.block_row_size
    if fault != "grad_out_unrounded":
        g = bf16_round(g)
    if fault == "bwd_scale_bf16":
        scale = bf16_round(f32(scale))
    delta = delta_f32(g, out, fault)
    dq = np.zeros((a.num_rows, q.shape[1]), f32)
    dk = np.zeros((a.num_cols, q.shape[1]), f32)
    dv = np.zeros((a.num_cols, v.shape[1]), f32)
    acc = np.zeros((bs, q.shape[1]), f32)
    for r, lo, hi, keys in _block_rows(a):
        if hi == lo:
            continue
        rows = slice(r * bs, (r + 1) * bs)
        s = (q[rows].astype(f64) @ k[keys].T.astype(f64)).astype(f32)
        z = f32(scale) * s if mask is None else fma32(f32(scale), s, mask[lo:hi].transpose(1, 0, 2).reshape(bs, -1))
        dp = (g[rows].astype(f64) @ v[keys].T.astype(f64)).astype(f32)
        _, dsb = _weights(z, dp, lse[rows, None], delta[rows, None], scale, fault)
        if fault != "dq_acc_carried":
            acc = np.zeros((bs, q.shape[1]), f32)
        for c in range(0, keys.shape[0], 32):
            acc = mfma_add(acc, dsb[:, c:c + 32], k[keys[c:c + 32]], fault)
        dq[rows] = acc
    for c, lo, hi, qs in _block_rows(at):
        if hi == lo:
            continue
        keys = slice(c * bs, (c + 1) * bs)
        s = (q[qs].astype(f64) @ k[keys].T.astype(f64)).astype(f32)                          # [queries, keys]
        if mask is None:
            z = f32(scale) * s
        else:
            blocks = mask[perm[lo:hi].astype(np.int64)]
            z = fma32(f32(scale), s, (blocks.transpose(0, 2, 1) if fault == "mask_transposed_cols" else blocks).reshape(-1, bs))
        dp = (g[qs].astype(f64) @ v[keys].T.astype(f64)).astype(f32)
        pb, dsb = _weights(z, dp, lse[qs, None], delta[qs, None], scale, fault)
        if fault == "last_query_dropped":
            pb, dsb = pb.copy(), dsb.copy()
            pb[-1], dsb[-1] = 0, 0
        acck, accv = np.zeros((bs, q.shape[1]), f32), np.zeros((bs, v.shape[1]), f32)
        for at_ in range(0, qs.shape[0], 32):
            step = qs[at_:at_ + 32]
            acck = mfma_add(acck, dsb[at_:at_ + 32].T, q[step], fault)
            accv = mfma_add(accv, pb[at_:at_ + 32].T, g[step], fault)
        dk[keys], dv[keys] = acck, accv
    if grads_bf16:
        dq, dk, dv = bf16_round(dq), bf16_round(dk), bf16_round(dv)
    return dq, dk, dv
