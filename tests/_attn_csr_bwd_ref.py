"""The fused CSR attention backward contract (include/mispmm_attn_csr_bwd.h) for the tests: the cases and operands the CPU and
GPU tests share, float64 masked attention differentiated analytically (`backward_f64`), both passes AS BUILT restated in numpy
float32 (`backward_f32`), the derived tolerances (`bwd_tolerances`), and the table of kernel tags.

    P[e] = exp(z[e] - lse[r])    dP[e] = <g[r], v[c]>    delta[r] = <g[r], out[r]>    dS[e] = scale P[e] (dP[e] - delta[r])
    dq[r] = sum_row dS k[c]      dk[c] = sum_column dS q[r]                          dv[c] = sum_column P g[r]

OPERANDS are those of tests/_attn_csr_ref.py (q, k multiples of 2^-8 so that every score is exact in fp32, a power-of-two scale,
v with full mantissas, the three kinds of bias) plus a grad_out `g` with full mantissas.  PATTERNS adds `edgesT`, the transpose
of `edges` built here in numpy: it is what gives the COLUMN pass of the backward columns of 0, 1, ..., 8, 9, ..., 257, 300 and
1025 entries, empty ones first and last (the column pass of `edgesT` walks the rows of `edges`).

TOLERANCES (`bwd_tolerances`), per element of dq, dk, dv: first-order propagation in float64 of the header's NUMERICS, nothing
measured.  With u = 2^-24, g_n = n u / (1 - n u), tiny = 2^-126, per entry e of row r, t = z - lse:
    E_z      the forward's: the FAST SDDMM bound on |scale| sum |q||k| plus the fma's rounding (as _attn_csr_ref.lse_tolerance)
    E_lse    _attn_csr_ref.lse_tolerance of the row: the kernel reads the STORED lse
    E_P      P expm1(E_z + E_lse + (3 |t| + 3) u) + tiny        one rounding of z - lse, the rounded log2 e and its product, v_exp_f32
    E_dP     g_Dv sum |g||v| + Dv tiny
    E_delta  g_Dv sum |g||o| + sum |g| E_out + Dv tiny          E_out = _attn_csr_ref.out_tolerance: the kernel reads the STORED out
    E_dS     |scale| (E_P (|x| + E_x) + P E_x + 3 u P |x|) + 3 tiny,   x = dP - delta, E_x = E_dP + E_delta
    dq       sum_row (E_dS |k|) + g_L sum_row |dS||k| + L tiny           L the entries of the row
    dk       sum_col (E_dS |q|) + g_L sum_col |dS||q| + L tiny           L the entries of the column
    dv       sum_col (E_P |g|)  + g_L sum_col P |g|   + L tiny
times 1.01 for the second order.  A masked entry (z = -Inf beside a finite lse) is exact: P = +0, no error."""
import functools

import numpy as np

import _attn_csr_ref as ref
from _sddmm_ref import bound as sddmm_bound, entry_rows
from _softmax_bsr_ref import fma32
from _softmax_ref import full_mantissa, matrix as _matrix, softmax_rows

from mispmm import formats

U = 2.0 ** -24
TINY = 2.0 ** -126
BATCH = ref.BATCH
PATTERNS = ("edges", "edgesT", "ragged")
WIDTHS, BIASES, HEADS = ref.WIDTHS, ref.BIASES, ref.HEADS
Case = ref.Case
CASES = tuple(Case(n, d, dv, b, h) for n in PATTERNS for (d, dv) in WIDTHS for b in BIASES for h in HEADS)

FAULTS = ("delta_from_the_wrong_row", "delta_omitted", "head0_lse_for_every_head", "bias_not_permuted", "head0_bias_for_every_head",
          "last_slot_of_full_batch_dropped", "dead_slot_counts_one", "scale_missing_from_ds", "dk_from_k", "accumulator_carried_over")
HONEST = ("exp_float64", "sums_in_another_order")


def transpose(csr):
    """(A^T's pattern, perm): entry t of A^T is entry perm[t] of A; the entries of a column keep A's storage order."""
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    perm = np.argsort(cols, kind="stable")
    ptrs = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=csr.num_cols))])
    t = formats.CSR(csr.num_cols, csr.num_rows, ptrs.astype(np.uint32), rows[perm].astype(np.uint32), np.asarray(csr.data)[perm])
    return t, perm.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """`edgesT`: the transpose of `edges`; any other name: _softmax_ref.matrix.  Read-only."""
    if name == "edgesT":
        return transpose(_matrix("edges"))[0]
    return _matrix(name)


@functools.lru_cache(maxsize=None)
def transposed(name):
    return transpose(matrix(name))


@functools.lru_cache(maxsize=None)
def operands(case):
    """dict(q [H, M, D], k [1, K, D], v [1, K, Dv], g [H, M, Dv], bias None | [nnz] | [H, nnz], scale): the recipe of
    _attn_csr_ref.operands (k, v shared by the heads; `finite` with H > 1 a bias per head, `masked` a shared one) plus g."""
    csr = matrix(case.name)
    rng = np.random.default_rng(9100 + 7 * case.d + case.dv + 100 * case.heads + len(case.bias) + 1000 * PATTERNS.index(case.name))
    q = ref._grid(rng, (case.heads, csr.num_rows, case.d))
    k = ref._grid(rng, (1, csr.num_cols, case.d))
    v = full_mantissa(rng, (1, csr.num_cols, case.dv), np.float32)
    g = full_mantissa(rng, (case.heads, csr.num_rows, case.dv), np.float32)
    per_head = case.heads if case.bias == "finite" else 1
    bias = ref.make_bias(csr, case.bias, per_head, rng)
    if bias is not None and per_head == 1:
        bias = bias[0]
    res = dict(q=q, k=k, v=v, g=g, bias=bias, scale=ref.scale_of(case.d))
    for x in res.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return res


def _scatter(n, index, values):
    out = np.zeros((n,) + values.shape[1:])
    np.add.at(out, index, values)
    return out


# ---- float64
def backward_f64(csr, q, k, v, g, scale, bias=None):
    """(dq [H, M, D], dk [H, K, D], dv [H, K, Dv]) in float64: dense masked attention on the pattern differentiated
    analytically, entry by entry (a pair stored twice counts twice).  dk and dv per head, also where k and v are shared."""
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    heads = q.shape[0]
    dq, dk, dv = np.zeros((heads, csr.num_rows, q.shape[2])), np.zeros((heads, csr.num_cols, q.shape[2])), np.zeros((heads, csr.num_cols, v.shape[2]))
    for h in range(heads):
        z, _ = ref.scores_f64(csr, q, k, scale, bias, h)
        qh, kh, vh, gh = (ref._head(x, h).astype(np.float64) for x in (q, k, v, g))
        with np.errstate(invalid="ignore", over="ignore"):
            p = softmax_rows(csr.row_ptrs, z).astype(np.float64)
            dp = (gh[rows] * vh[cols]).sum(axis=1)
            delta = _scatter(csr.num_rows, rows, p * dp)
            ds = scale * p * (dp - delta[rows])
        dq[h] = _scatter(csr.num_rows, rows, ds[:, None] * kh[cols])
        dk[h] = _scatter(csr.num_cols, cols, ds[:, None] * qh[rows])
        dv[h] = _scatter(csr.num_cols, cols, p[:, None] * gh[rows])
    return dq, dk, dv


def gamma_u(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def propagate(csr, q, k, v, g, scale, bias, out, lse, e_z, e_lse, e_out, exp_extra, gam):
    """The gradients in float64 from (out, lse) by the header's formulas and their first-order error bounds, per head:
    ((dq, dk, dv), (tol dq, tol dk, tol dv)).  out [H, M, Dv] and lse [H, M]: float64 (exact ones, or a kernel's stored ones);
    e_z [H][nnz], e_lse [H, M], e_out [H, M, Dv]: what z, lse and out may be off by; exp_extra: the roundings charged to the
    exponential besides 3 |t| u (3 for the header's bound: the difference, the product with log2 e, the instruction);
    gam(n): the relative bound on an fp32 sum of n terms.  A row whose lse is not finite has no bound (NaN)."""
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    lens = np.diff(np.asarray(csr.row_ptrs, dtype=np.int64)).astype(np.float64)
    clens = np.bincount(cols, minlength=csr.num_cols).astype(np.float64)
    heads, d, dv_w = q.shape[0], q.shape[2], v.shape[2]
    grads = [np.zeros((heads, csr.num_rows, d)), np.zeros((heads, csr.num_cols, d)), np.zeros((heads, csr.num_cols, dv_w))]
    tols = [np.zeros_like(x) for x in grads]
    for h in range(heads):
        z = ref.scores_f32(csr, q, k, scale, bias, h).astype(np.float64) if e_z is None else ref.scores_f64(csr, q, k, scale, bias, h)[0]
        qh, kh, vh, gh = (ref._head(x, h).astype(np.float64) for x in (q, k, v, g))
        masked = np.isneginf(z)
        with np.errstate(invalid="ignore", over="ignore"):
            if e_z is None:         # the kernel's own argument: one fp32 rounding of an exact z minus the stored lse
                t = np.where(masked, 0.0, (z.astype(np.float32) - lse[h][rows].astype(np.float32)).astype(np.float64))
            else:
                t = np.where(masked, 0.0, z - lse[h][rows])
            p = np.where(masked, 0.0, np.exp(t))
            rel = (0.0 if e_z is None else e_z[h] + e_lse[h][rows]) + (3.0 * np.abs(t) + exp_extra) * U
            e_p = np.where(masked, 0.0, p * np.expm1(rel) + TINY)
            dp = (gh[rows] * vh[cols]).sum(axis=1)
            e_dp = gam(dv_w) * (np.abs(gh[rows]) * np.abs(vh[cols])).sum(axis=1) + dv_w * TINY
            delta = (gh * out[h]).sum(axis=1)
            e_delta = gam(dv_w) * (np.abs(gh) * np.abs(out[h])).sum(axis=1) + dv_w * TINY
            if e_out is not None:
                e_delta = e_delta + (np.abs(gh) * e_out[h]).sum(axis=1)
            x, e_x = dp - delta[rows], e_dp + e_delta[rows]
            ds = np.where(masked, 0.0, scale * p * x)
            e_ds = np.where(masked, 0.0, abs(scale) * (e_p * (np.abs(x) + e_x) + p * e_x + 3.0 * U * p * np.abs(x)) + 3.0 * TINY)
        grads[0][h] = _scatter(csr.num_rows, rows, ds[:, None] * kh[cols])
        grads[1][h] = _scatter(csr.num_cols, cols, ds[:, None] * qh[rows])
        grads[2][h] = _scatter(csr.num_cols, cols, p[:, None] * gh[rows])
        tols[0][h] = (_scatter(csr.num_rows, rows, e_ds[:, None] * np.abs(kh[cols])) + gam(lens)[:, None] * _scatter(csr.num_rows, rows, np.abs(ds)[:, None] * np.abs(kh[cols]))
                      + lens[:, None] * TINY)
        tols[1][h] = (_scatter(csr.num_cols, cols, e_ds[:, None] * np.abs(qh[rows])) + gam(clens)[:, None] * _scatter(csr.num_cols, cols, np.abs(ds)[:, None] * np.abs(qh[rows]))
                      + clens[:, None] * TINY)
        tols[2][h] = (_scatter(csr.num_cols, cols, e_p[:, None] * np.abs(gh[rows])) + gam(clens)[:, None] * _scatter(csr.num_cols, cols, p[:, None] * np.abs(gh[rows]))
                      + clens[:, None] * TINY)
    return tuple(grads), tuple(1.01 * t for t in tols)


def score_errors(csr, q, k, scale, bias):
    """E_z per head and entry, as _attn_csr_ref.lse_tolerance takes it; 0 on a masked entry."""
    res = []
    for h in range(q.shape[0]):
        z, s_abs = ref.scores_f64(csr, q, k, scale, bias, h)
        live = ~np.isneginf(z)
        res.append(np.where(live, sddmm_bound(np.float32, "fast", q.shape[2], np.where(live, z, 0.0), s_abs * (1 + 2 * U)) + 2 * U * s_abs, 0.0))
    return res


def bwd_tolerances(csr, q, k, v, g, scale, bias=None):
    """(tol dq, tol dk, tol dv), the docstring's derivation around the exact float64 forward."""
    out, lse = ref.attention_f64(csr, q, k, v, scale, bias)
    e_out = ref.out_tolerance(csr, q, k, v, scale, bias)
    e_lse = ref.lse_tolerance(csr, q, k, scale, bias)
    with np.errstate(invalid="ignore"):
        lse = np.where(np.isneginf(lse), 0.0, lse)               # an empty row: no entry reads it
    return propagate(csr, q, k, v, g, scale, bias, out, lse, score_errors(csr, q, k, scale, bias), e_lse, e_out, 3.0, gamma_u)[1]


# ---- both passes as built
def _slots(csr):
    idx, live, batches = ref.batch_table(csr)
    ptrs = np.asarray(csr.row_ptrs, dtype=np.int64)
    first = np.minimum(ptrs[:-1], max(csr.nnz - 1, 0))            # what a dead slot's fetch re-reads: the row's first entry
    return idx, live, first


def backward_f32(csr, q, k, v, g, scale, bias, out, lse, fault=None):
    """(dq, dk, dv) in float32 from the forward's stored out [H, M, Dv] and lse [H, M] (float32), as attn_csr_bwd.hip goes: z one
    fma, P = v_exp_f32(fl(fl(z - lse) log2 e)), dS = fl(fl(P fl(dP - delta)) scale), every accumulator from +0 by one fma per
    entry in storage order -- the row pass on A's pattern, the column pass on A^T's with the bias read through perm.  s, dP and
    delta are restated as correctly rounded dot products: the kernel's chains and trees differ from them inside g_n.
    fault: None, one of FAULTS (tests/_attn_csr_bwd_mutants.py) or of HONEST."""
    if fault is not None and fault not in FAULTS and fault not in HONEST:
        raise ValueError(f"unknown fault {fault!r}")
    f32 = np.float32
    t_csr, perm = transpose(csr)
    perm = perm.astype(np.int64)
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    heads, d, dv_w = q.shape[0], q.shape[2], v.shape[2]
    dq, dk, dv = np.zeros((heads, csr.num_rows, d), f32), np.zeros((heads, csr.num_cols, d), f32), np.zeros((heads, csr.num_cols, dv_w), f32)
    sc = f32(scale)
    in64 = fault == "exp_float64"

    def accumulate(table, weights, gathered):
        """fma chain over the slots of every row of `table` in order: sum_j weights[:, j] * gathered[:, j, :]."""
        idx, live, _ = table
        acc = np.zeros((idx.shape[0], gathered.shape[2]), f32)
        order = range(idx.shape[1] - 1, -1, -1) if fault == "sums_in_another_order" else range(idx.shape[1])
        for j in order:
            acc = fma32(weights[:, j, None], gathered[:, j, :], acc)
        if fault == "accumulator_carried_over":                 # the group's registers are not cleared between its rows
            acc[1:] = acc[1:] + acc[:-1]
        return acc

    def per_slot(table, r_of_e, c_of_e, h, lse_h, delta, bias_index):
        """(P, dS) per slot of the table, dead slots +0, and the slots' live mask."""
        idx, live, first = table
        e = np.where(live, idx, first[:, None])                   # a dead slot re-reads the first entry
        r, c = r_of_e[e], c_of_e[e]
        qh, kh, vh, gh = (ref._head(x, h) for x in (q, k, v, g))
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            s = (qh.astype(np.float64)[r] * kh.astype(np.float64)[c]).sum(axis=2).astype(f32)
            b = ref._bias_of(bias, h, csr.nnz, fault)[bias_index(e)]
            z = fma32(sc, s, b)
            lr = lse_h[r]
            p = np.where(np.isfinite(lr), ref._exp32((z - lr).astype(f32), in64), f32(np.nan)).astype(f32)
            dp = (gh.astype(np.float64)[r] * vh.astype(np.float64)[c]).sum(axis=2).astype(f32)
            dr = delta[(r + 1) % csr.num_rows] if fault == "delta_from_the_wrong_row" else delta[r]
            x = dp if fault == "delta_omitted" else (dp - dr).astype(f32)
            ds = (p * x).astype(f32)
            if fault != "scale_missing_from_ds":
                ds = (ds * sc).astype(f32)
            keep = live.copy()
            if fault == "last_slot_of_full_batch_dropped":
                full = live.reshape(live.shape[0], -1, BATCH).all(axis=2)
                keep = (live.reshape(live.shape[0], -1, BATCH) & ~(full[:, :, None] & (np.arange(BATCH) == BATCH - 1))).reshape(live.shape)
            if fault == "dead_slot_counts_one":                   # the re-read entry with P = 1 instead of +0, in started batches
                started = np.repeat(live.reshape(live.shape[0], -1, BATCH).any(axis=2), BATCH, axis=1)
                extra = started & ~live
                p = np.where(extra, f32(1), p)
                ds = np.where(extra, (x * sc).astype(f32), ds)
                keep = keep | extra
            p, ds = np.where(keep, p, f32(0)).astype(f32), np.where(keep, ds, f32(0)).astype(f32)
        return p, ds, r, c, keep

    table_a, table_t = _slots(csr), _slots(t_csr)
    for h in range(heads):
        gh, qh, kh = ref._head(g, h), ref._head(q, h), ref._head(k, h)
        lse_h = lse[0 if fault == "head0_lse_for_every_head" else h].astype(f32)
        with np.errstate(invalid="ignore", over="ignore"):
            delta = (gh.astype(np.float64) * out[h].astype(np.float64)).sum(axis=1).astype(f32)
        ident = lambda e: e                                                                     # noqa: E731
        _, ds, r, c, keep = per_slot(table_a, rows, cols, h, lse_h, delta, ident)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            dq[h] = accumulate(table_a, ds, np.where(keep[:, :, None], kh[c], f32(0)))
            # the column pass: entry t of A^T is entry perm[t] of A
            through = ident if fault == "bias_not_permuted" else (lambda t: perm[t])            # noqa: E731
            p, ds, r, c, keep = per_slot(table_t, rows[perm], cols[perm], h, lse_h, delta, through)
            dv[h] = accumulate(table_t, p, np.where(keep[:, :, None], gh[r], f32(0)))
            dk[h] = accumulate(table_t, ds, np.where(keep[:, :, None], (kh[c] if fault == "dk_from_k" else qh[r]), f32(0)))
    return dq, dk, dv


# ---- the kernel tags
def tags_of(d, dv, aligned, need=(True, True, True)):
    """The tags a call leaves behind, in launch order (mispmm_last_kernel() is the last one)."""
    shape = ref.tag_of(d, dv, aligned)[len("attn_csr"):]
    row, col = need[0] or need[1], need[1] or need[2]
    return ["attn_csr_bwd_row" + shape] * row + ["attn_csr_bwd_col" + shape] * col


# tag -> the smallest (D, Dv, aligned) that reaches it: the forward's table, per pass
TAGS = {f"attn_csr_bwd_{kind}" + tag[len("attn_csr"):]: shape for kind in ("row", "col") for tag, shape in ref.TAGS.items()}
