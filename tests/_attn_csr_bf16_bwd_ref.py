"""The fused bf16 CSR attention backward contract (include/mispmm_attn_csr_bf16_bwd.h) for the tests: the cases and operands the
CPU and GPU tests share, the checks, both passes AS BUILT restated in numpy with the lane grouping of V8 and V1, the
bf16-specific faults, and the table of kernel tags.

bf16 widens to fp32 exactly, so the contract IS the ALGORITHM of include/mispmm_attn_csr_bwd.h on the widened operands and every
reference is one the project already owns, evaluated on them: `backward_f64` and `bwd_tolerances` of _attn_csr_bwd_ref, which
take operands; the derived tight check of _attn_csr_bwd_tight, whose `reference` is bound to that module's case table and is
restated here in its few lines on THESE operands.  Nothing here is measured on a kernel.

OPERANDS: q and k from _attn_csr_ref._grid (n / 256 with 64 <= |n| <= 192: they ARE bf16 values and every score is exact in
fp32 in any order), the power-of-two scale, `make_bias`; v and grad_out `g` have full mantissas ROUNDED TO bf16, and every
reference reads the rounded ones.  PATTERNS are those of the fp32 backward (`edgesT` gives the column pass its columns of 0,
1, ..., 8, 9, ..., 257, 300 and 1025 entries), WIDTHS those of the bf16 forward (every V8 G, every V1 G, C2 and C4).
LAYOUT on the device: `padded_bits` of _attn_csr_bf16_ref (a buffer 8 columns wider, NaN bits in the pad).
A bf16 gradient is the fp32 gradient rounded once to nearest even (`_spmm_bf16_ref.bf16_bits`)."""
import functools

import numpy as np

import _attn_csr_bf16_ref as fref
import _attn_csr_bwd_ref as bref
import _attn_csr_ref as ref
import _attn_csr_tight as tight
from _attn_csr_bf16_ref import bf16_bits, widen
from _sddmm_ref import entry_rows
from _softmax_bsr_ref import fma32
from _softmax_ref import full_mantissa

from mispmm import synth

PATTERNS = bref.PATTERNS                 # edges, edgesT, ragged
WIDTHS = fref.WIDTHS
BIASES, HEADS, PAD = fref.BIASES, fref.HEADS, fref.PAD
BATCH = ref.BATCH
GRADS = ("dq", "dk", "dv")
GRAD_SENTINEL_BF16 = 0x7FDE              # what the pad columns of a bf16 gradient hold before the call, and after
Case = ref.Case
CASES = tuple(Case(n, d, dv, b, h) for n in PATTERNS for (d, dv) in WIDTHS for b in BIASES for h in HEADS)
matrix, transposed = bref.matrix, bref.transposed

# deliberate bf16-specific faults of the restatement: name -> the words of mispmm_attn_csr_bf16_bwd.h it breaks
FAULTS = {
    "q_pair_swapped": "COLUMN PASS: `dK = fma(dS_i, q[r_i], dK)` per column -- the halves of every 32-bit pair of a gathered Q row exchanged.",
    "g_pair_swapped": "COLUMN PASS: `dV = fma(P_i, g[r_i], dV)` per column -- the halves of every 32-bit pair of a gathered grad_out row exchanged.",
    "g_at_v_stride": "OPERANDS: `a row stride (ld*) ... of its own` -- grad_out's rows are gathered at ldv's stride (ldg != ldv in the case).",
    "grads_truncated": "OPERANDS: a bf16 gradient is `rounded once to nearest even` -- the low 16 bits are cut off instead.",
    "out_read_as_bf16": "OPERANDS: `out ... fp32` -- the row of out is read as if its elements were 2 bytes wide.",
}
FP32_FAULTS = bref.FAULTS                # the fp32 backward's ten: the restatement below carries every one
HONEST = bref.HONEST


@functools.lru_cache(maxsize=None)
def operands(case):
    """dict(q [H, M, D], k [1, K, D], v [1, K, Dv], g [H, M, Dv], bias None | [nnz] | [H, nnz], scale), float32 arrays of bf16
    values: the recipe of _attn_csr_bwd_ref.operands with v and g rounded to bf16.  Read-only."""
    csr = matrix(case.name)
    rng = np.random.default_rng(29100 + 7 * case.d + case.dv + 100 * case.heads + len(case.bias) + 1000 * PATTERNS.index(case.name))
    q = ref._grid(rng, (case.heads, csr.num_rows, case.d))
    k = ref._grid(rng, (1, csr.num_cols, case.d))
    rounded = lambda shape: synth.bf16_round(full_mantissa(rng, shape, np.float32).reshape(-1)).reshape(shape).astype(np.float32)   # noqa: E731
    v = rounded((1, csr.num_cols, case.dv))
    g = rounded((case.heads, csr.num_rows, case.dv))
    per_head = case.heads if case.bias == "finite" else 1
    bias = ref.make_bias(csr, case.bias, per_head, rng)
    if bias is not None and per_head == 1:
        bias = bias[0]
    res = dict(q=q, k=k, v=v, g=g, bias=bias, scale=ref.scale_of(case.d))
    for x in res.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return res


def one_hot_g(case):
    """A grad_out [H, M, Dv] of bf16 values whose rows each hold ONE non-zero column (full 8-bit mantissas): dP is one exact
    product of two bf16 values and delta one rounded product plus exact zeros, in any lane grouping."""
    csr = matrix(case.name)
    rng = np.random.default_rng(29900 + case.d + case.dv + case.heads)
    g = np.zeros((case.heads, csr.num_rows, case.dv), np.float32)
    at = rng.integers(0, case.dv, (case.heads, csr.num_rows))
    val = synth.bf16_round(full_mantissa(rng, (case.heads * csr.num_rows,), np.float32)).reshape(case.heads, csr.num_rows).astype(np.float32)
    np.put_along_axis(g, at[:, :, None], val[:, :, None], axis=2)
    return g


# ---- the checks, functions of (got, case), on THESE operands
def _args(case):
    op = operands(case)
    return matrix(case.name), op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"]


@functools.lru_cache(maxsize=None)
def expected(case):
    """((dq, dk, dv), (tolerances)) of a case in float64; read-only."""
    return bref.backward_f64(*_args(case)), bref.bwd_tolerances(*_args(case))


def bwd_composed(got, case):
    """dq, dk, dv against float64 inside bwd_tolerances: (ok, worst |err| / tolerance per output)."""
    want, tols = expected(case)
    res = [tight._worst(got[n], w, t) for n, w, t in zip(GRADS, want, tols)]
    return all(ok for ok, _ in res), tuple(worst for _, worst in res)


def tight_reference(case, out, lse):
    """_attn_csr_bwd_tight.reference on these operands: ((dq, dk, dv), (tolerances)) in float64 around a forward's stored out
    [H, M, Dv] and lse [H, M]."""
    csr, q, k, v, g, scale, bias = _args(case)
    assert tight.exact_scores(csr, q, k, scale, bias), "the scores are not exact in fp32 -- use narrower operands"
    with np.errstate(invalid="ignore"):
        lse64 = np.where(np.isneginf(lse), 0.0, lse.astype(np.float64))          # an empty row: no entry reads it
    return bref.propagate(csr, q, k, v, g, scale, bias, out.astype(np.float64), lse64, None, None, None, 2.0, tight.gamma)


def tight_backward(got, case):
    """dq, dk, dv against the derived reference around got["out"], got["lse"]: (ok, worst |err| / tolerance per output)."""
    want, tols = tight_reference(case, got["out"], got["lse"])
    res = [tight._worst(got[n], w, t) for n, w, t in zip(GRADS, want, tols)]
    return all(ok for ok, _ in res), tuple(worst for _, worst in res)


def coverage(case, out, lse):
    """The share of the elements of dq, dk, dv whose tight reference and tolerance are finite numbers."""
    want, tols = tight_reference(case, out, lse)
    return sum(int((np.isfinite(w) & np.isfinite(t)).sum()) for w, t in zip(want, tols)) / sum(w.size for w in want)


def bf16_composed(got, case):
    """The bf16 gradients, widened, against float64 inside bwd_tolerances plus one bf16 rounding."""
    want, tols = expected(case)
    res = [tight._worst(widen(np.ascontiguousarray(got[n + "_bf16"]).view(np.uint16)), w, fref.with_one_bf16_rounding(w, t)) for n, w, t in zip(GRADS, want, tols)]
    return all(ok for ok, _ in res), tuple(worst for _, worst in res)


def rounded_once(got, case=None):
    """Every bf16 gradient is the fp32 gradient rounded once to nearest even, bit for bit, NaN for NaN: (ok, elements that differ)."""
    wrong = []
    for n in GRADS:
        want = bf16_bits(got[n])
        bits = np.ascontiguousarray(got[n + "_bf16"]).view(np.uint16)
        nan = np.isnan(widen(want))
        wrong.append(float((nan != np.isnan(widen(bits))).sum() + (bits[~nan] != want[~nan]).sum()))
    return not any(wrong), tuple(wrong)


CHECKS = {"bwd_tolerances": bwd_composed, "tight_backward": tight_backward, "bf16_plus_one_rounding": bf16_composed, "rounded_once": rounded_once}


# ---- the lane group restated
def lanes_of(d, dv, vec):
    """(G, chunks) of a call: G the smallest of 8, 16, 32, 64 with G * vec >= max(D, Dv); chunks of G * vec columns held."""
    width = max(d, dv)
    g = next((x for x in (8, 16, 32, 64) if x * vec >= width), 64)
    chunks = -(-width // (g * vec))
    return g, (1 if chunks <= 1 else 2 if chunks == 2 else 4)


def lane_dot(x, y, g, vec, chunks):
    """<x, y> over the last axis as a lane group sums it: lane l holds columns c * G * vec + l * vec + (0 .. vec - 1) of every
    chunk c and sums their products by ONE fma chain from +0, chunks then columns ascending; the lanes' sums meet in the tree
    lanes 1, 2, 4, ... apart.  float32 in, float32 out."""
    width = x.shape[-1]
    full = g * vec * chunks
    assert width <= full
    pad = [(0, 0)] * (x.ndim - 1) + [(0, full - width)]
    x, y = (np.pad(np.asarray(t, dtype=np.float32), pad).reshape(t.shape[:-1] + (chunks, g, vec)) for t in (x, y))
    acc = np.zeros(x.shape[:-3] + (g,), np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for c in range(chunks):
            for e in range(vec):
                acc = fma32(x[..., c, :, e], y[..., c, :, e], acc).astype(np.float32)
        while acc.shape[-1] > 1:
            acc = (acc[..., 0::2] + acc[..., 1::2]).astype(np.float32)
    return acc[..., 0]


def _swap_pairs(x):
    y = x.copy()
    n = x.shape[-1] // 2 * 2
    y[..., 0:n:2], y[..., 1:n:2] = x[..., 1:n:2], x[..., 0:n:2]
    return y


def _rows_at_stride(x, ld_own, ld_used):
    """Rows of x [M, W], stored with row stride ld_own (NaN in the pad between rows, as the suite lays it out), read at row
    stride ld_used; a read past the descriptor's span returns zeros, as a buffer load does."""
    rows, width = x.shape
    flat = np.full(rows * ld_own, np.nan, np.float32)
    flat[(np.arange(rows)[:, None] * ld_own + np.arange(width)[None, :]).ravel()] = x.ravel()
    end = (rows - 1) * ld_own + width
    want = np.arange(rows)[:, None] * ld_used + np.arange(width)[None, :]
    return np.where(want < end, flat[np.minimum(want, flat.shape[0] - 1)], np.float32(0)).astype(np.float32)


def _out_as_bf16(out_h):
    """A row of fp32 out read as if it were bf16: column j is half j of the row's first words, widened."""
    halves = np.ascontiguousarray(out_h, dtype=np.float32).view(np.uint16).reshape(out_h.shape[0], -1)     # little-endian: low half first
    return widen(halves[:, :out_h.shape[1]])


def backward_as_built(csr, q, k, v, g, scale, bias, out, lse, vec, fault=None, ldg=None, ldv=None):
    """(dq, dk, dv, delta) in float32 from the forward's stored fp32 out [H, M, Dv] and lse [H, M], as attn_csr_bf16_bwd.hip goes
    on lanes of `vec` columns (8 or 1): _attn_csr_bwd_ref.backward_f32 restated with s, dP and delta summed AS THE LANE GROUP
    sums them (`lane_dot`) instead of correctly rounded.  z one fma, P = v_exp_f32(fl(fl(z - lse) log2 e)), NaN where lse is not
    finite, dS = fl(fl(P fl(dP - delta)) scale), dead slots +0, every accumulator from +0 by one fma per entry in storage
    order; the column pass on A^T's pattern with the bias read through perm.
    fault: None, one of FAULTS, of FP32_FAULTS or of HONEST.  ldg, ldv: the row strides `g_at_v_stride` confuses."""
    if fault is not None and fault not in FAULTS and fault not in FP32_FAULTS and fault not in HONEST:
        raise ValueError(f"unknown fault {fault!r}")
    f32 = np.float32
    t_csr, perm = bref.transpose(csr)
    perm = perm.astype(np.int64)
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    heads, d, dv_w = q.shape[0], q.shape[2], v.shape[2]
    lanes, chunks = lanes_of(d, dv_w, vec)
    dot = lambda x, y: lane_dot(x, y, lanes, vec, chunks)                      # noqa: E731
    dq, dk, dv = np.zeros((heads, csr.num_rows, d), f32), np.zeros((heads, csr.num_cols, d), f32), np.zeros((heads, csr.num_cols, dv_w), f32)
    deltas = np.zeros((heads, csr.num_rows), f32)
    sc = f32(scale)
    in64 = fault == "exp_float64"

    def accumulate(table, weights, gathered):
        idx, live, _ = table
        acc = np.zeros((idx.shape[0], gathered.shape[2]), f32)
        order = range(idx.shape[1] - 1, -1, -1) if fault == "sums_in_another_order" else range(idx.shape[1])
        for j in order:
            acc = fma32(weights[:, j, None], gathered[:, j, :], acc)
        if fault == "accumulator_carried_over":
            acc[1:] = acc[1:] + acc[:-1]
        return acc

    def per_slot(table, r_of_e, c_of_e, h, lse_h, delta, bias_index, qh, gh):
        """(P, dS) per slot of the table, dead slots +0; qh, gh: Q and grad_out as this pass reads their rows."""
        idx, live, first = table
        e = np.where(live, idx, first[:, None])
        r, c = r_of_e[e], c_of_e[e]
        kh, vh = ref._head(k, h), ref._head(v, h)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            s_e = dot(qh[r_of_e], kh[c_of_e])                       # per entry, then laid into the slots
            dp_e = dot(gh[r_of_e], vh[c_of_e])
            s, dp = s_e[e], dp_e[e]
            b = ref._bias_of(bias, h, csr.nnz, fault)[bias_index(e)]
            z = fma32(sc, s, b)
            lr = lse_h[r]
            p = np.where(np.isfinite(lr), ref._exp32((z - lr).astype(f32), in64), f32(np.nan)).astype(f32)
            dr = delta[(r + 1) % csr.num_rows] if fault == "delta_from_the_wrong_row" else delta[r]
            x = dp if fault == "delta_omitted" else (dp - dr).astype(f32)
            ds = (p * x).astype(f32)
            if fault != "scale_missing_from_ds":
                ds = (ds * sc).astype(f32)
            keep = live.copy()
            if fault == "last_slot_of_full_batch_dropped":
                full = live.reshape(live.shape[0], -1, BATCH).all(axis=2)
                keep = (live.reshape(live.shape[0], -1, BATCH) & ~(full[:, :, None] & (np.arange(BATCH) == BATCH - 1))).reshape(live.shape)
            if fault == "dead_slot_counts_one":
                started = np.repeat(live.reshape(live.shape[0], -1, BATCH).any(axis=2), BATCH, axis=1)
                extra = started & ~live
                p = np.where(extra, f32(1), p)
                ds = np.where(extra, (x * sc).astype(f32), ds)
                keep = keep | extra
            p, ds = np.where(keep, p, f32(0)).astype(f32), np.where(keep, ds, f32(0)).astype(f32)
        return p, ds, r, c, keep

    table_a, table_t = bref._slots(csr), bref._slots(t_csr)
    for h in range(heads):
        gh, qh, kh = ref._head(g, h), ref._head(q, h), ref._head(k, h)
        lse_h = lse[0 if fault == "head0_lse_for_every_head" else h].astype(f32)
        oh = _out_as_bf16(out[h]) if fault == "out_read_as_bf16" else out[h]
        with np.errstate(invalid="ignore", over="ignore"):
            delta = dot(gh, oh)
        deltas[h] = delta
        ident = lambda e: e                                                                     # noqa: E731
        _, ds, r, c, keep = per_slot(table_a, rows, cols, h, lse_h, delta, ident, qh, gh)
        # what the column pass gathers
        q_col = _swap_pairs(qh) if fault == "q_pair_swapped" else qh
        g_col = _swap_pairs(gh) if fault == "g_pair_swapped" else _rows_at_stride(gh, ldg, ldv) if fault == "g_at_v_stride" else gh
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            dq[h] = accumulate(table_a, ds, np.where(keep[:, :, None], kh[c], f32(0)))
            through = ident if fault == "bias_not_permuted" else (lambda t: perm[t])            # noqa: E731
            p, ds, r, c, keep = per_slot(table_t, rows[perm], cols[perm], h, lse_h, delta, through, q_col, g_col)
            dv[h] = accumulate(table_t, p, np.where(keep[:, :, None], g_col[r], f32(0)))
            dk[h] = accumulate(table_t, ds, np.where(keep[:, :, None], (kh[c] if fault == "dk_from_k" else q_col[r]), f32(0)))
    return dq, dk, dv, deltas


def vec_of(case, aligned=True):
    return 8 if aligned and case.d % 8 == 0 and case.dv % 8 == 0 else 1


@functools.lru_cache(maxsize=None)
def forward_restated(case):
    csr, q, k, v, _, scale, bias = _args(case)
    return ref.fused_f32(csr, q, k, v, scale, bias)


@functools.lru_cache(maxsize=8)
def restated(case, fault=None, vec=None):
    """The restated backward on the restated forward's out and lse: dict(out, lse, delta, dq, dk, dv, dq_bf16, dk_bf16, dv_bf16);
    vec: the lane width (default: what the suite's padded layout reaches)."""
    csr, q, k, v, g, scale, bias = _args(case)
    out, lse = forward_restated(case)
    # the suite's layout: g a view of [M, H, Dv + PAD] storage, v one head of [K, Dv + PAD]
    dq, dk, dv, delta = backward_as_built(csr, q, k, v, g, scale, bias, out, lse, vec or vec_of(case), fault,
                                          ldg=case.heads * (case.dv + PAD), ldv=case.dv + PAD)
    res = dict(out=out, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)
    for n in GRADS:
        if fault == "grads_truncated":
            res[n + "_bf16"] = (np.ascontiguousarray(res[n]).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
        else:
            res[n + "_bf16"] = bf16_bits(res[n])
    return res


# ---- the kernel tags
def tags_of(d, dv, aligned, need=(True, True, True)):
    """The tags a call leaves behind, in launch order (mispmm_last_kernel() is the last one)."""
    shape = fref.tag_of(d, dv, aligned)[len("attn_csr_bf16"):]
    row, col = need[0] or need[1], need[1] or need[2]
    return ["attn_csr_bf16_bwd_row" + shape] * row + ["attn_csr_bf16_bwd_col" + shape] * col


# tag -> the smallest (D, Dv, aligned) that reaches it: the forward's table, per pass
TAGS = {f"attn_csr_bf16_bwd_{kind}" + tag[len("attn_csr_bf16"):]: shape for kind in ("row", "col") for tag, shape in fref.TAGS.items()}


def fp32_tag(tag):
    """The fp32 backward's tag of the same pass, G, V1 and C, or None where the bf16 tag is V8."""
    if ",V8," in tag:
        return None
    kind, rest = tag[len("attn_csr_bf16_bwd_"):].split("<")
    return f"attn_csr_bwd_{kind}<f32,{rest}"
