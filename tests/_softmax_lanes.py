"""The two row-softmax kernels restated in numpy IN THEIR OWN LANE ORDER, after the words of csrc/softmax_csr.hip and
csrc/softmax_bsr.hip (include/mispmm.h, sections "Row softmax on a CSR pattern" and "Row softmax on a BSR pattern").

CSR.  G lanes own a row (G = _softmax_ref.picked_group).  A row of L <= 4 G entries is taken by its group, W = G; a longer one
by the whole wave, W = 64.  Lane l of the W holds entries l, l + W, l + 2 W, ...: up to 4 W entries from registers (slots
j = 0..3), beyond that in walks of 4 W = 256 entries a step (max; sum; write -- backward: sum; write), the exponentials
computed again on the last walk: to the same bits, so one code below serves both.  A lane sums in ascending order from +0, a
slot past the row's end adding +0; the W lanes then meet in a butterfly of xor moves 1, 2, 4, ..., W / 2.
    f32,ref64  everything in float64, rounded to float32 once.      f32,fast  float32; exp2 of fl(t * fl(log2 e)); fma
    f64,ref    float64; product and add rounded apart (backward).   f64,fast  float64; fma
BSR.  One workgroup of 4 waves per block row; wave w takes blocks w, w + 4, ...; a lane holds 4 consecutive elements of an
element row, G = bS / 4 lanes to a row (at 32 x 32 a lane holds four element rows, 8 apart, each summed for itself).  A lane
sums block by block, then left to right; the G lanes meet in a butterfly; the waves as ((w0 + w1) + w2) + w3.  A block row
of up to C blocks (32 at bS 16, 16 at bS 32) is held, a longer one walked: the blocks past the end of a held row add +0, so
again one code serves both and `held` / `walk` only says where a fault can sit.  fp32 throughout, as f32,fast.

np.exp, np.exp2 stand for the device's exp and v_exp_f32: each within the ulp the header allows, not the same last bit.  The
backward has no exponential: its bits are the kernel's.

Every function takes fault=None, a name of FAULTS (tests/_softmax_mutants.py says which words of the header each breaks) or
of HONEST (variants that keep the contract).  None leaves every bit alone; an unknown name raises ValueError."""
import numpy as np

from _softmax_bsr_ref import HELD, bf16_round, fma32
from _softmax_ref import REGS

WAVE = 64
WAVES = 4                                   # waves of a BSR workgroup
LOG2E = np.float32(1.44269504088896340736)
ARITH = ("f32,ref64", "f32,fast", "f64,ref", "f64,fast")     # the second part of the kernel's tag

CSR_FWD_FAULTS = ("max_never_subtracted", "max_from_first_walk_step", "max_from_own_group", "second_walk_one_step_short",
                  "last_register_slot_dropped", "last_entry_dropped", "dead_slot_counts_one", "butterfly_skips_widest_step",
                  "ref_exp_in_fp32", "ref_sum_rounded_to_fp32", "f64_sum_in_fp32", "fast_log2e_in_bf16",
                  "fast_scaled_before_difference", "division_by_rounded_reciprocal")
CSR_BWD_FAULTS = ("dot_from_first_walk_step", "dot_misses_last_slot", "ref_dot_in_fp32", "single_entry_row_keeps_dp",
                  "ds_from_p_dp_minus_dot", "fast_dot_unfused")
BSR_FWD_FAULTS = ("z_two_roundings", "z_without_mask_on_second_pass", "mask_scaled_with_scores", "max_shared_in_block_row",
                  "wave3_lost", "block_c_dropped_when_full", "walk_starts_at_w_plus_4", "bf16_out_truncated",
                  "bf16_out_from_bf16_sum")
BSR_BWD_FAULTS = ("scale_applied_twice", "scale_dropped", "bf16_p_read_as_high_half", "dot_over_first_c_blocks",
                  "bf16_ds_truncated", "bsr_dot_unfused")
FAULTS = CSR_FWD_FAULTS + CSR_BWD_FAULTS + BSR_FWD_FAULTS + BSR_BWD_FAULTS
HONEST = ("exp_float64", "sums_in_another_order", "butterfly_widest_step_first")


def _known(fault):
    if fault is not None and fault not in FAULTS and fault not in HONEST:
        raise ValueError(f"unknown fault {fault!r}")


# ---- exact fused multiply-add in float64 (Boldo & Melquiond: the low parts summed to odd, then one rounding)
def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def _two_prod(a, b):
    split = 134217729.0                      # 2^27 + 1 (Veltkamp)
    p = a * b
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma64(a, b, c):
    """fl64(a * b + c), one rounding, element-wise; operands far from overflow and underflow (p, dp of a softmax)."""
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        ph, pl = _two_prod(a, b)
        th, tl = _two_sum(c, ph)
        v, err = _two_sum(tl, pl)
        odd = np.isfinite(v) & (err != 0) & ((v.view(np.int64) & 1) == 0)
        v = np.where(odd, np.nextafter(v, np.where(err > 0, np.inf, -np.inf)), v)
        out = th + v
        return np.where(np.isfinite(ph) & np.isfinite(out), out, a * b + c)


def butterfly(v, f, width, skip_widest=False, widest_first=False):
    """f over the `width` lanes of the last axis by xor moves 1, 2, ..., width / 2: every lane ends with the result."""
    idx = np.arange(v.shape[-1])
    moves = [k for k in (1, 2, 4, 8, 16, 32) if k < width]
    if skip_widest:
        moves = moves[:-1]
    for k in (reversed(moves) if widest_first else moves):
        v = f(v, v[..., idx ^ k])
    return v


def _types(arith):
    if arith not in ARITH:
        raise ValueError(f"unknown arithmetic {arith!r}")
    return (np.float32 if arith.startswith("f32") else np.float64), (np.float32 if arith == "f32,fast" else np.float64)


def _exp(t, arith, fault):
    """The arithmetic's exponential of t (already in its type A)."""
    if arith == "f32,fast":
        if fault == "exp_float64":
            return np.exp(t.astype(np.float64)).astype(np.float32)
        c = np.float32(bf16_round(LOG2E)) if fault == "fast_log2e_in_bf16" else LOG2E
        return np.exp2((t * c).astype(np.float32))
    if fault == "ref_exp_in_fp32" and arith == "f32,ref64":
        return np.exp(t.astype(np.float32)).astype(np.float64)
    if fault == "exp_float64":
        return np.exp(t.astype(np.longdouble)).astype(np.float64)
    return np.exp(t)


def csr_shape(length, group):
    """(W, steps): the lanes that own a row of `length` entries and its walk steps of 4 W entries (1: from registers)."""
    w = group if length <= REGS * group else WAVE
    return w, max(1, -(-length // (REGS * w)))


def _laid_out(v, length, w, steps, fill):
    """A row as [step][slot j][lane]: entry step * 4 W + j * W + lane."""
    pad = np.full(steps * REGS * w, fill, dtype=v.dtype)
    pad[:length] = v
    return pad.reshape(steps, REGS, w)


def _lane_sum(terms, zero, add, reverse=False):
    """A lane's chain from +0 over [step][slot] in ascending order (descending: the honest other order)."""
    acc = zero
    order = [(st, j) for st in range(terms[0].shape[0]) for j in range(REGS)]
    for st, j in (reversed(order) if reverse else order):
        acc = add(acc, *(x[st, j] for x in terms))
    return acc


def csr_forward(row_ptrs, scores, arith, group, fault=None):
    _known(fault)
    t_out, a = _types(arith)
    rp = np.asarray(row_ptrs, dtype=np.int64)
    s_all = np.asarray(scores)
    out = np.zeros(s_all.shape[0], dtype=t_out)
    sum_type = np.float32 if (fault == "f64_sum_in_fp32" and arith.startswith("f64")) else a
    with np.errstate(all="ignore"):
        for lo, hi in zip(rp[:-1], rp[1:]):
            length = int(hi - lo)
            if length == 0:
                continue
            w, steps = csr_shape(length, group)
            s = _laid_out(s_all[lo:hi].astype(a), length, w, steps, -np.inf)
            live = _laid_out(np.ones(length, bool), length, w, steps, False)
            top = s[:1] if (fault == "max_from_first_walk_step" and steps > 1) else s
            m = np.fmax.reduce(top.reshape(-1, w), axis=0, initial=-np.inf)                  # fmax drops a NaN
            m = butterfly(m, np.fmax, group if (fault == "max_from_own_group" and w == WAVE) else w)
            if fault == "max_never_subtracted":
                m = np.zeros_like(m)
            if fault == "fast_scaled_before_difference" and arith == "f32,fast":
                e = np.exp2(((s * LOG2E).astype(a) - (m * LOG2E).astype(a)).astype(a))
            else:
                e = _exp((s - m).astype(a), arith, fault)
            e = np.where(live, e, a(0))
            terms = e.astype(sum_type)
            if fault == "dead_slot_counts_one":
                terms = np.where(live, terms, sum_type(1))
            if fault == "last_entry_dropped":
                terms = terms.copy()
                terms.reshape(steps, REGS, w)[(length - 1) // (REGS * w), (length - 1) % (REGS * w) // w, (length - 1) % w] = 0
            if fault == "last_register_slot_dropped" and length == REGS * w:
                terms = terms.copy()
                terms[:, REGS - 1] = 0
            if fault == "second_walk_one_step_short" and steps > 1:
                terms = terms[:-1]
            total = _lane_sum((terms,), np.zeros(w, sum_type), lambda acc, x: (acc + x).astype(sum_type), fault == "sums_in_another_order")
            total = butterfly(total, lambda x, y: (x + y).astype(sum_type), w, fault == "butterfly_skips_widest_step",
                              fault == "butterfly_widest_step_first").astype(a)
            if fault == "ref_sum_rounded_to_fp32" and arith == "f32,ref64":
                total = total.astype(np.float32).astype(a)
            q = e * (a(1) / total).astype(a) if fault == "division_by_rounded_reciprocal" else e / total
            out[lo:hi] = q.astype(a).reshape(-1)[:length].astype(t_out)
    return out


def _mac(arith, fault):
    if arith == "f32,ref64":
        if fault == "ref_dot_in_fp32":
            return lambda acc, x, y: (acc.astype(np.float32) + (x * y).astype(np.float32)).astype(np.float32).astype(np.float64)
        return lambda acc, x, y: acc + x * y                 # an fp32 x fp32 product is exact in fp64: one rounding, at the add
    if arith == "f64,ref" or fault == "fast_dot_unfused":
        return lambda acc, x, y: acc + x * y                 # product and add rounded apart, each in the arithmetic's type
    if arith == "f32,fast":
        return lambda acc, x, y: fma32(x, y, acc)
    return lambda acc, x, y: fma64(x, y, acc)


def csr_backward(row_ptrs, p, dp, arith, group, fault=None):
    _known(fault)
    t_out, a = _types(arith)
    rp = np.asarray(row_ptrs, dtype=np.int64)
    p_all, d_all = np.asarray(p), np.asarray(dp)
    out = np.zeros(p_all.shape[0], dtype=t_out)
    mac = _mac(arith, fault)
    with np.errstate(all="ignore"):
        for lo, hi in zip(rp[:-1], rp[1:]):
            length = int(hi - lo)
            if length == 0:
                continue
            w, steps = csr_shape(length, group)
            pv = _laid_out(p_all[lo:hi].astype(a), length, w, steps, 0)
            dv = _laid_out(d_all[lo:hi].astype(a), length, w, steps, 0)
            ps, ds_ = pv, dv
            if fault == "dot_from_first_walk_step" and steps > 1:
                ps, ds_ = pv[:1], dv[:1]
            if fault == "dot_misses_last_slot":
                ps = ps.copy()
                at = ((length - 1) // (REGS * w), (length - 1) % (REGS * w) // w, (length - 1) % w)
                if at[0] < ps.shape[0]:
                    ps[at] = 0
            dot = _lane_sum((ps, ds_), np.zeros(w, a), lambda acc, x, y: np.asarray(mac(acc, x, y)).astype(a), fault == "sums_in_another_order")
            dot = butterfly(dot, lambda x, y: (x + y).astype(a), w, widest_first=fault == "butterfly_widest_step_first")
            if fault == "ds_from_p_dp_minus_dot":
                q = (pv * dv).astype(a) - dot
            elif fault == "single_entry_row_keeps_dp" and length == 1:
                q = pv * dv
            else:
                q = pv * (dv - dot).astype(a)
            out[lo:hi] = q.astype(a).reshape(-1)[:length].astype(t_out)
    return out


# ---- BSR
def _z(scores, mask, scale, fault):
    s = np.asarray(scores, dtype=np.float32)
    scale = np.float32(scale)
    with np.errstate(all="ignore"):
        if mask is None:
            return (scale * s).astype(np.float32)
        mask = np.asarray(mask, dtype=np.float32)
        if fault == "z_two_roundings":
            return ((scale * s).astype(np.float32) + mask).astype(np.float32)
        if fault == "mask_scaled_with_scores":
            return (np.float64(scale) * (s.astype(np.float64) + mask.astype(np.float64))).astype(np.float32)
        return fma32(scale, s, mask)


def _dealt(v, n, bs, fill):
    """A block row's [n][bS][bS] as [round][wave][element row][lane g][4]: block round * 4 + wave, column 4 g + j."""
    rounds = -(-n // WAVES)
    pad = np.full((rounds * WAVES, bs, bs), fill, dtype=v.dtype)
    pad[:n] = v
    return pad.reshape(rounds, WAVES, bs, bs // 4, 4)


def _block_row_sum(terms, add, bs, fault):
    """terms: arrays [round][wave][row][g][4].  The lane's chain (block by block, then left to right) from +0, the butterfly
    over the G lanes, the waves as ((w0 + w1) + w2) + w3: [row]."""
    g = bs // 4
    acc = np.zeros((WAVES, bs, g), np.float32)
    order = [(b, j) for b in range(terms[0].shape[0]) for j in range(4)]
    for b, j in (reversed(order) if fault == "sums_in_another_order" else order):
        acc = add(acc, *(x[b, :, :, :, j] for x in terms))
    acc = butterfly(acc, lambda x, y: (x + y).astype(np.float32), g, widest_first=fault == "butterfly_widest_step_first")
    total = ((acc[0] + acc[1]).astype(np.float32) + acc[2]).astype(np.float32)
    if fault != "wave3_lost":
        total = (total + acc[3]).astype(np.float32)
    return total[:, 0]


def _truncate_bf16(v):
    return (np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def bsr_forward(block_row_ptrs, bs, scores, mask, scale, out_bf16=False, fault=None):
    """float32 [num_blocks, bS, bS]; with out_bf16 the bf16 numbers the kernel stores, as float32."""
    _known(fault)
    ptrs = np.asarray(block_row_ptrs, dtype=np.int64)
    z_all = _z(scores, mask, scale, fault)
    bare = _z(scores, None, scale, None)
    out = np.zeros(z_all.shape, np.float32)
    with np.errstate(all="ignore"):
        for lo, hi in zip(ptrs[:-1], ptrs[1:]):
            n = int(hi - lo)
            if n == 0:
                continue
            walks = n > HELD[bs]
            z = _dealt(z_all[lo:hi], n, bs, -np.inf)
            there = _dealt(np.ones((n, bs, bs), bool), n, bs, False)
            m = np.fmax.reduce(z.transpose(2, 0, 1, 3, 4).reshape(bs, -1), axis=1, initial=-np.inf)
            if fault == "max_shared_in_block_row":
                m = np.full_like(m, np.fmax.reduce(m))
            m5 = m[None, None, :, None, None]
            e = np.where(there, _exp((z - m5).astype(np.float32), "f32,fast", fault), np.float32(0))
            terms = e
            if fault == "z_without_mask_on_second_pass" and walks and mask is not None:
                terms = np.where(there, _exp((_dealt(bare[lo:hi], n, bs, -np.inf) - m5).astype(np.float32), "f32,fast", None), np.float32(0))
            if fault == "block_c_dropped_when_full" and n == HELD[bs]:
                terms = terms.copy()
                terms[(n - 1) // WAVES, (n - 1) % WAVES] = 0
            if fault == "walk_starts_at_w_plus_4" and walks:
                terms = terms.copy()
                terms[0] = 0
            total = _block_row_sum((terms,), lambda acc, x: (acc + x).astype(np.float32), bs, fault)
            if fault == "bf16_out_from_bf16_sum" and out_bf16:
                total = bf16_round(total)
            q = (e / total[None, None, :, None, None]).astype(np.float32)
            out[lo:hi] = q.reshape(-1, bs, bs)[:n]
    if out_bf16:
        return _truncate_bf16(out) if fault == "bf16_out_truncated" else bf16_round(out)
    return out


def bsr_backward(block_row_ptrs, bs, p, dp, scale, p_bf16=False, ds_bf16=False, fault=None):
    """p: float32 values (bf16 numbers where p_bf16).  float32 [num_blocks, bS, bS]; with ds_bf16 the bf16 numbers stored."""
    _known(fault)
    ptrs = np.asarray(block_row_ptrs, dtype=np.int64)
    p_all, d_all = np.asarray(p, dtype=np.float32), np.asarray(dp, dtype=np.float32)
    if fault == "bf16_p_read_as_high_half" and p_bf16:
        flat = p_all.reshape(-1)
        p_all = flat[(2 * np.arange(flat.shape[0]) + 1) % flat.shape[0]].reshape(p_all.shape)     # element k: the high half of word k
    scale = np.float32(scale)
    out = np.zeros(p_all.shape, np.float32)
    with np.errstate(all="ignore"):
        for lo, hi in zip(ptrs[:-1], ptrs[1:]):
            n = int(hi - lo)
            if n == 0:
                continue
            pv, dv = _dealt(p_all[lo:hi], n, bs, 0), _dealt(d_all[lo:hi], n, bs, 0)
            ps = pv
            if fault == "dot_over_first_c_blocks" and n > HELD[bs]:
                ps = pv.copy()
                ps.reshape(-1, bs, bs // 4, 4)[HELD[bs]:] = 0
            mac = (lambda acc, x, y: (acc + (x * y).astype(np.float32)).astype(np.float32)) if fault == "bsr_dot_unfused" else (lambda acc, x, y: fma32(x, y, acc))
            dot = _block_row_sum((ps, dv), mac, bs, fault)
            t = (dv - dot[None, None, :, None, None]).astype(np.float32)
            q = (pv * t).astype(np.float32)
            if fault != "scale_dropped":
                q = (scale * q).astype(np.float32)
            if fault == "scale_applied_twice":
                q = (scale * q).astype(np.float32)
            out[lo:hi] = q.reshape(-1, bs, bs)[:n]
    if ds_bf16:
        return _truncate_bf16(out) if fault == "bf16_ds_truncated" else bf16_round(out)
    return out
