"""The bias gradient of the fused CSR attention (include/mispmm_attn_csr_dbias.h) for the tests: the cases and operands the CPU
and GPU tests share, dBias in float64 (`dbias_f64`), the kernel AS BUILT restated in numpy float32 (`dbias_f32`, in the manner
of _attn_csr_bwd_ref.backward_f32), the derived tolerance (`dbias_tolerance`), dq rebuilt from dBias (`dq_from_dbias`: what the
GPU test holds equal to the backward's dq bit for bit), the checks both tests run, and the table of kernel tags.

    z[e] = fma(scale, <q[r], k[c]>, bias[e])   P[e] = exp(z[e] - lse[r])   dP[e] = <g[r], v[c]>   delta[r] = <g[r], out[r]>
    dBias[e] = P[e] (dP[e] - delta[r])                                                            (no scale: dz / dbias = 1)

CASES are _attn_csr_bwd_ref.CASES on the patterns `edges` and `ragged` (the kernel is a row pass: `edgesT` adds no row length),
OPERANDS those of _attn_csr_bwd_ref.operands; for bf16, q, k, v and g rounded to bf16 first (q and k are bf16 values already).

TOLERANCE (`dbias_tolerance`), per entry, nothing measured.  The symbols are those of _attn_csr_bwd_ref's docstring:
    E_dBias = E_P (|x| + E_x) + P E_x + 2 u P |x| + 2 tiny,      x = dP - delta, E_x = E_dP + E_delta
times 1.01 for the second order: the header's dS bound with one rounding fewer and no scale.  A masked entry is exact."""
import functools

import numpy as np

import _attn_csr_bf16_ref as fref
import _attn_csr_bwd_ref as bref
import _attn_csr_ref as ref
from _sddmm_ref import entry_rows
from _softmax_bsr_ref import fma32

from mispmm import synth

U, TINY, BATCH = bref.U, bref.TINY, ref.BATCH
PATTERNS = ("edges", "ragged")
ELEMS = ("f32", "bf16")
Case = ref.Case
CASES = tuple(c for c in bref.CASES if c.name in PATTERNS)
matrix = bref.matrix

SENTINEL = np.uint32(0x7FC0D81A)        # a NaN of a recognisable payload: what dBias and its guards hold before a call

FAULTS = ("scale_multiplied_in", "delta_omitted", "delta_from_the_wrong_row", "head0_lse_for_every_head", "head0_bias_for_every_head",
          "last_slot_of_full_batch_not_stored", "dead_slot_stored", "stored_at_previous_batch_offset")
HONEST = ("exp_float64", "sums_in_another_order")


@functools.lru_cache(maxsize=None)
def operands(case, elem="f32"):
    """_attn_csr_bwd_ref.operands(case); elem == "bf16": q, k, v and g rounded to bf16 (float32 arrays of bf16 values).  Read-only."""
    op = dict(bref.operands(case))
    if elem == "bf16":
        for n in ("q", "k", "v", "g"):
            op[n] = synth.bf16_round(op[n].reshape(-1)).reshape(op[n].shape)
            op[n].setflags(write=False)
    return op


# ---- float64
def _entry_terms(csr, q, k, v, g, scale, bias, h, out_h, lse_h):
    """(z, P, dP, delta[rows], masked) per entry of head h in float64 from out [M, Dv] and lse [M] (float64)."""
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    z = ref.scores_f64(csr, q, k, scale, bias, h)[0]
    vh, gh = (ref._head(x, h).astype(np.float64) for x in (v, g))
    masked = np.isneginf(z)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(masked, 0.0, z - lse_h[rows])
        p = np.where(masked, 0.0, np.exp(t))
        dp = (gh[rows] * vh[cols]).sum(axis=1)
        delta = (gh * out_h).sum(axis=1)
    return z, t, p, dp, delta, masked


def _exact_forward(csr, q, k, v, scale, bias):
    out, lse = ref.attention_f64(csr, q, k, v, scale, bias)
    with np.errstate(invalid="ignore"):
        return out, np.where(np.isneginf(lse), 0.0, lse)            # an empty row: no entry reads it


def dbias_f64(csr, q, k, v, g, scale, bias=None):
    """dBias [H, nnz] in float64 by the formulas above around the exact float64 forward (a pair stored twice counts twice)."""
    out, lse = _exact_forward(csr, q, k, v, scale, bias)
    res = np.zeros((q.shape[0], csr.nnz))
    rows = entry_rows(csr.row_ptrs)
    for h in range(q.shape[0]):
        _, _, p, dp, delta, masked = _entry_terms(csr, q, k, v, g, scale, bias, h, out[h], lse[h])
        with np.errstate(invalid="ignore"):
            res[h] = np.where(masked, 0.0, p * (dp - delta[rows]))
    return res


def dbias_tolerance(csr, q, k, v, g, scale, bias=None):
    """E_dBias [H, nnz], the docstring's derivation around the exact float64 forward: E_z, E_lse, E_out, E_P, E_dP and E_delta
    exactly as _attn_csr_bwd_ref.propagate takes them for bwd_tolerances."""
    out, lse = _exact_forward(csr, q, k, v, scale, bias)
    e_out = ref.out_tolerance(csr, q, k, v, scale, bias)
    e_lse = ref.lse_tolerance(csr, q, k, scale, bias)
    e_z = bref.score_errors(csr, q, k, scale, bias)
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    dv_w = v.shape[2]
    tol = np.zeros((q.shape[0], csr.nnz))
    for h in range(q.shape[0]):
        _, t, p, dp, delta, masked = _entry_terms(csr, q, k, v, g, scale, bias, h, out[h], lse[h])
        vh, gh = (ref._head(x, h).astype(np.float64) for x in (v, g))
        with np.errstate(invalid="ignore", over="ignore"):
            rel = e_z[h] + e_lse[h][rows] + (3.0 * np.abs(t) + 3.0) * U
            e_p = np.where(masked, 0.0, p * np.expm1(rel) + TINY)
            e_dp = bref.gamma_u(dv_w) * (np.abs(gh[rows]) * np.abs(vh[cols])).sum(axis=1) + dv_w * TINY
            e_delta = bref.gamma_u(dv_w) * (np.abs(gh) * np.abs(out[h])).sum(axis=1) + dv_w * TINY + (np.abs(gh) * e_out[h]).sum(axis=1)
            x, e_x = dp - delta[rows], e_dp + e_delta[rows]
            tol[h] = np.where(masked, 0.0, e_p * (np.abs(x) + e_x) + p * e_x + 2.0 * U * p * np.abs(x) + 2.0 * TINY)
    return 1.01 * tol


# ---- the kernel as built
def _dot32(x, y, reverse):
    """<x, y> along the last axis in float32: correctly rounded (the kernel's chain and tree differ from it inside g_n), or
    `reverse`: summed in float32, last column first."""
    if not reverse:
        return (x.astype(np.float64) * y.astype(np.float64)).sum(axis=-1).astype(np.float32)
    acc = np.zeros(x.shape[:-1], np.float32)
    for c in range(x.shape[-1] - 1, -1, -1):
        acc = fma32(x[..., c], y[..., c], acc).astype(np.float32)
    return acc


def dbias_f32(csr, q, k, v, g, scale, bias, out, lse, fault=None, head_stride=None, with_p=False):
    """dBias as attn_csr_dbias.hpp goes, in float32 from the forward's stored out [H, M, Dv] and lse [H, M]: a uint32 view-able
    float32 buffer [H, head_stride] (head_stride >= nnz, default nnz) that holds SENTINEL before the stores -- so a store that
    is missed or lands elsewhere shows.  z one fma, P = v_exp_f32(fl(fl(z - lse) log2 e)), delta per row, dBias =
    fl(P fl(dP - delta)); s, dP and delta restated as correctly rounded dot products.  Slots of a row's batches in order; a
    live slot stores to base + position.  fault: None, one of FAULTS or of HONEST.  with_p: also P per entry [H, nnz]."""
    if fault is not None and fault not in FAULTS and fault not in HONEST:
        raise ValueError(f"unknown fault {fault!r}")
    f32 = np.float32
    heads, nnz = q.shape[0], csr.nnz
    stride = nnz if head_stride is None else head_stride
    buf = np.full((heads, stride), SENTINEL, np.uint32).view(f32)
    p_all = np.zeros((heads, nnz), f32)
    idx, live, batches = ref.batch_table(csr)
    ptrs = np.asarray(csr.row_ptrs, dtype=np.int64)
    first = np.minimum(ptrs[:-1], max(nnz - 1, 0))
    rows_e, cols_e = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    sc = f32(scale)
    reverse = fault == "sums_in_another_order"
    pos = np.arange(idx.shape[1])[None, :]
    started = (pos // BATCH) < batches[:, None]
    for h in range(heads):
        qh, kh, vh, gh = (ref._head(x, h) for x in (q, k, v, g))
        lse_h = lse[0 if fault == "head0_lse_for_every_head" else h].astype(f32)
        e = np.where(live, idx, first[:, None])                      # a dead slot re-reads the row's first entry
        r, c = rows_e[e], cols_e[e]
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            delta = _dot32(gh, out[h].astype(f32), reverse)
            s = _dot32(qh[r], kh[c], reverse)
            b = ref._bias_of(bias, h, nnz, fault)[e]
            z = fma32(sc, s, b)
            lr = lse_h[r]
            p = np.where(np.isfinite(lr), ref._exp32((z - lr).astype(f32), fault == "exp_float64"), f32(np.nan)).astype(f32)
            dp = _dot32(gh[r], vh[c], reverse)
            dr = delta[(r + 1) % csr.num_rows] if fault == "delta_from_the_wrong_row" else delta[r]
            x = dp if fault == "delta_omitted" else (dp - dr).astype(f32)
            val = (p * x).astype(f32)
            if fault == "scale_multiplied_in":
                val = (val * sc).astype(f32)
        p_all[h, idx[live]] = p[live]
        where = ptrs[:-1, None] + pos                                # base + s0 + sub
        store = live.copy()
        if fault == "last_slot_of_full_batch_not_stored":
            full = live.reshape(live.shape[0], -1, BATCH).all(axis=2)
            store &= ~np.repeat(full, BATCH, axis=1) | (pos % BATCH != BATCH - 1)
        if fault == "stored_at_previous_batch_offset":
            where = np.where(pos >= BATCH, where - BATCH, where)
        buf[h, where[store]] = val[store]
        if fault == "dead_slot_stored":                              # ... after the rows' own stores: the clobber is what remains
            extra = started & ~live & (where < stride)
            buf[h, where[extra]] = val[extra]
    return (buf, p_all) if with_p else buf


def dq_from_dbias(csr, dbias, k, scale):
    """dq [H, M, D] in float32 as the backward's row pass forms it, from dBias [H, nnz]: dS = fl(dBias scale) (exact for a scale
    that is a power of two, short of a subnormal), dq = fma32(dS_i, K[c_i], dq) from +0 in storage order, batch after batch of
    the row's OWN batches -- a dead slot of the last one is fma(+0, +0, dq), as in the kernel (dS replaced by +0, the K row
    dropped: zeros)."""
    f32 = np.float32
    idx, live, batches = ref.batch_table(csr)
    cols = np.asarray(csr.col_idxs, dtype=np.int64)
    heads, d = dbias.shape[0], k.shape[2]
    dq = np.zeros((heads, csr.num_rows, d), f32)
    if csr.nnz == 0:
        return dq
    for h in range(heads):
        kh = ref._head(k, h)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            ds = np.where(live, (dbias[h].astype(f32) * f32(scale)).astype(f32)[idx], f32(0)).astype(f32)
            acc = np.zeros((csr.num_rows, d), f32)
            for j in range(idx.shape[1]):
                active = j // BATCH < batches
                if not active.any():
                    break
                kj = np.where(live[:, j, None], kh[cols[idx[:, j]]], f32(0)).astype(f32)
                new = fma32(ds[:, j, None], kj, acc).astype(f32)
                acc = np.where(active[:, None], new, acc)
            dq[h] = acc
    return dq


# ---- the checks of the CPU test (on the restatement and its mutants) and of the GPU test (on the kernel)
@functools.lru_cache(maxsize=None)
def expected(case, elem="f32"):
    """(dBias float64 [H, nnz], E_dBias [H, nnz]) of a case; read-only."""
    op, csr = operands(case, elem), matrix(case.name)
    args = (csr, op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"])
    res = dbias_f64(*args), dbias_tolerance(*args)
    for x in res:
        x.setflags(write=False)
    return res


def finite_rows(csr, lse):
    """[H, nnz] bool: the entries of rows whose stored lse is finite."""
    return np.isfinite(np.asarray(lse))[:, entry_rows(csr.row_ptrs)]


def inside_tolerance(got, case, elem="f32"):
    """got: dict(dbias [H, >= nnz], lse [H, M]).  Every entry of a row with a finite lse within E_dBias of float64, a NaN
    counting as outside: (ok, worst |err| / tolerance)."""
    csr = matrix(case.name)
    want, tol = expected(case, elem)
    x = np.asarray(got["dbias"])[:, :csr.nnz].astype(np.float64)
    take = finite_rows(csr, got["lse"])
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(x - want)
        ok = np.where(take, err <= tol, True)
        ratio = np.where(take & (err > 0), err / np.where(tol > 0, tol, TINY), 0.0)
    return bool(ok.all()), float(np.nanmax(ratio, initial=0.0))


def all_written(got, case, elem="f32"):
    """Every one of the H * nnz entries holds something other than SENTINEL, and every word past nnz of a head still does:
    (ok, entries left + guard words changed)."""
    csr = matrix(case.name)
    bits = np.ascontiguousarray(got["dbias"]).view(np.uint32)
    left = int((bits[:, :csr.nnz] == SENTINEL).sum())
    changed = int((bits[:, csr.nnz:] != SENTINEL).sum())
    return left == 0 and changed == 0, left + changed


def rebuilds_dq(got, case, elem="f32"):
    """got also holds dq [H, M, D]: the backward's row pass on the same operands.  dq rebuilt from dBias equals it in every bit
    on every row with a finite lse: (ok, elements that differ)."""
    op, csr = operands(case, elem), matrix(case.name)
    mine = dq_from_dbias(csr, np.asarray(got["dbias"])[:, :csr.nnz], op["k"], op["scale"])
    lens = np.diff(np.asarray(csr.row_ptrs, dtype=np.int64))
    take = (np.isfinite(np.asarray(got["lse"])) | (lens == 0)[None, :])[:, :, None]
    differ = (mine.view(np.uint32) != np.ascontiguousarray(got["dq"], dtype=np.float32).view(np.uint32)) & take
    return not differ.any(), int(differ.sum())


CHECKS = {"inside_tolerance": inside_tolerance, "all_written": all_written, "rebuilds_dq": rebuilds_dq}


@functools.lru_cache(maxsize=None)
def forward_restated(case, elem="f32"):
    """(out, lse) of _attn_csr_ref.fused_f32 on the case's operands: what the restatements read.  Read-only."""
    op = operands(case, elem)
    res = ref.fused_f32(matrix(case.name), op["q"], op["k"], op["v"], op["scale"], op["bias"])
    for x in res:
        x.setflags(write=False)
    return res


def restated(case, elem="f32", fault=None, with_p=False):
    """dict(dbias, lse, dq[, p]): dbias_f32 and the backward's restated dq (_attn_csr_bwd_ref.backward_f32, honest) on one out, lse."""
    op, csr = operands(case, elem), matrix(case.name)
    out, lse = forward_restated(case, elem)
    args = (csr, op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"], out, lse)
    res = dbias_f32(*args, fault=fault, with_p=with_p)
    got = dict(dbias=res[0] if with_p else res, lse=lse, dq=_restated_dq(case, elem))
    if with_p:
        got["p"] = res[1]
    return got


@functools.lru_cache(maxsize=None)
def _restated_dq(case, elem):
    """dq of _attn_csr_bwd_ref.backward_f32, the project's restatement of the backward that already exists: written without
    a thought of dBias, so that `rebuilds_dq` on the restatements compares two things.  Read-only."""
    op, csr = operands(case, elem), matrix(case.name)
    out, lse = forward_restated(case, elem)
    dq = bref.backward_f32(csr, op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"], out, lse)[0]
    dq.setflags(write=False)
    return dq


# ---- the kernel tags
def tag_of(elem, d, dv, aligned):
    """mispmm_last_kernel() for (D, Dv, operands 16-byte aligned with strides in multiples of the lane width): the host's choice
    restated by the forward's tables, which the backward's rule is."""
    shape = (ref.tag_of(d, dv, aligned)[len("attn_csr<f32,"):] if elem == "f32" else fref.tag_of(d, dv, aligned)[len("attn_csr_bf16<"):])
    return f"attn_csr_dbias<{elem}," + shape


# tag -> (elem, the smallest (D, Dv, aligned) that reaches it): the forwards' tables
TAGS = {tag_of("f32", *shape): ("f32", shape) for shape in ref.TAGS.values()}
TAGS.update({tag_of("bf16", *shape): ("bf16", shape) for shape in fref.TAGS.values()})
