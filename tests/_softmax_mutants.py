"""Deliberate faults for the lane-order restatements of the two row-softmax kernels (tests/_softmax_lanes.py) and the numerical
checks the GPU suites apply to the kernels' output, as functions of (got, case) -- the CPU harness
tests/test_softmax_mutants_cpu.py and tests/test_gpu_softmax_tight.py call the same code.  A fault is a name handed to a
restatement as `fault=`; every name carries one sentence that cites, in backquotes, the words of include/mispmm.h (sections
"Row softmax on a CSR pattern" and "Row softmax on a BSR pattern") it breaks: a kernel that made the same mistake would break
the contract in the same way.  HONEST: variants that keep the words and differ only where the header leaves room.

The checks come in the suite's order.  OLD is what tests/test_gpu_softmax.py and tests/test_gpu_softmax_bsr.py held before the
tight file: the stated bounds, the row sums, the exactness anchors, the special values.  NEW is tests/_softmax_tight.py."""
import collections
import functools

import numpy as np

import _softmax_bsr_ref as bref
import _softmax_lanes as lanes
import _softmax_ref as cref
import _softmax_tight as tight
from _softmax_tight import BsrCase, CsrCase

FAULTS = {
    # ---- CSR forward
    "max_never_subtracted": "forward: `exp(s[e] - m_r)` -- m_r = 0: the row's maximum is never subtracted.",
    "max_from_first_walk_step": "forward: `m_r the largest score of row r` -- of its first 256 entries: the first walk stops after one step.",
    "max_from_own_group": "forward: `m_r the largest score of row r` -- where the whole wave owns the row the maximum's butterfly still spans "
                          "G lanes: every group of lanes subtracts its own.",
    "second_walk_one_step_short": "forward: `sum_{e' in row r} exp(s[e'] - m_r)` -- the second walk ends one step of 256 early.",
    "last_register_slot_dropped": "`Any M, any nnz, any row length` -- a row of exactly 4 W entries loses slot j = 3 from its sum.",
    "last_entry_dropped": "`row r owns the elements [rowPtrs[r], rowPtrs[r + 1])` -- the sum stops before the entry at L - 1.",
    "dead_slot_counts_one": "`The quotients of a row sum to 1 within L u` -- a slot past the row's end counts exp(0) = 1 instead of +0.",
    "butterfly_skips_widest_step": "`the lanes of a row meet in a fixed tree` -- the tree lacks its widest step: each half of the lanes keeps its own sum.",
    "ref_exp_in_fp32": "f32 REFERENCE: `exp (the device library's double exp, 1 ulp)` -- the exponential is taken in fp32.",
    "ref_sum_rounded_to_fp32": "f32 REFERENCE: `sum in a fixed order and division in fp64; rounded to fp32 once` -- the sum is rounded to fp32 "
                               "before the division: twice.",
    "f64_sum_in_fp32": "f64: `fp64 throughout, the same arithmetic in both modes` -- the sum is kept in fp32.",
    "fast_log2e_in_bf16": "f32 FAST: `exp as v_exp_f32 of fl(t * log2 e)` -- the constant is log2 e rounded to bf16.",
    "fast_scaled_before_difference": "f32 FAST: `exp as v_exp_f32 of fl(t * log2 e)` -- of fl(fl(s log2 e) - fl(m log2 e)): the scores are scaled "
                                     "before the difference, which then carries the roundings of |s| and |m| instead of |t|.",
    "division_by_rounded_reciprocal": "Derivation: `the division u` -- the quotient is the product with the rounded reciprocal of the sum: 2 u.",
    # ---- CSR backward
    "dot_from_first_walk_step": "backward: `sum_{e' in row r} p[e'] * dp[e']` -- over the first 256 entries: the first walk stops after one step.",
    "dot_misses_last_slot": "backward: `sum_{e' in row r} p[e'] * dp[e']` -- without the entry at L - 1.",
    "ref_dot_in_fp32": "f32 REFERENCE: `products (exact) and sums in fp64, rounded once` -- products and sums in fp32.",
    "single_entry_row_keeps_dp": "backward: `ds[e] = p[e] * (dp[e] - sum_{e' in row r} p[e'] * dp[e'])` -- a row of one entry stores p * dp; it "
                                 "must be exactly p * 0.",
    "ds_from_p_dp_minus_dot": "backward: `p[e] * (dp[e] - sum_{e' in row r} p[e'] * dp[e'])` -- p * dp - dot: the factor p misses the dot.",
    "fast_dot_unfused": "FAST: `FAST fma ... an fp32 fma chain` -- the product is rounded before the add.",
    # ---- BSR forward
    "z_two_roundings": "z: `one fp32 fma` -- fl(fl(scale * s) + mask): two roundings.",
    "z_without_mask_on_second_pass": "`a longer one is walked three times (backward: twice), to the same bits` -- the second walk forms z without the mask.",
    "mask_scaled_with_scores": "z: `fl32(scale * s[e][i][j] + mask[e][i][j])` -- scale * (s + mask): the mask is scaled too.",
    "max_shared_in_block_row": "`m the largest z of the matrix row` -- of the whole block row: one maximum serves its bS matrix rows.",
    "wave3_lost": "`((w0 + w1) + w2) + w3 over the workgroup's waves` -- (w0 + w1) + w2: wave 3 is lost.",
    "block_c_dropped_when_full": "`A block row of up to C blocks ... is read once and held in registers` -- a row of exactly C blocks loses its last "
                                 "block from the sum.",
    "walk_starts_at_w_plus_4": "forward: `sum_row exp(z - m)` -- the second walk of wave w starts at block w + 4.",
    "bf16_out_truncated": "`a bf16 result is the fp32 result rounded once, to nearest even` -- truncated.",
    "bf16_out_from_bf16_sum": "`the fp32 result rounded once` -- the divisor is rounded to bf16 first: the result carries two roundings.",
    # ---- BSR backward
    "scale_applied_twice": "backward: `ds[e][i][j] = scale * p * (dp - sum_row p * dp)` -- scale * scale * p * (...).",
    "scale_dropped": "backward: `ds[e][i][j] = scale * p * (dp - sum_row p * dp)` -- p * (...) without the scale.",
    "bf16_p_read_as_high_half": "`a bf16 p is widened exactly` -- element k is the high half of the k-th 32-bit word: bf16 element 2 k + 1.",
    "dot_over_first_c_blocks": "backward: `sum_row p * dp` -- over the block row's first C blocks only.",
    "bf16_ds_truncated": "`rounded once, to nearest even, with the rounding of mispmm_f32_to_bf16` -- the bf16 ds is truncated.",
    "bsr_dot_unfused": "`the backward's row sum is an fp32 fma chain` -- the product is rounded before the add.",
}
HONEST = {
    "exp_float64": "the exponentials taken in a wider type (float64 for fp32, the widest float for fp64) and rounded once: inside the 1 ulp "
                   "the header gives the device's exp and v_exp_f32.",
    "sums_in_another_order": "a lane sums its entries in descending order: another fixed order, which `(L - 1) u whatever its order` allows.",
    "butterfly_widest_step_first": "the lanes meet in the butterfly's moves taken from the widest: another fixed tree.",
}
assert set(FAULTS) == set(lanes.FAULTS) and set(HONEST) == set(lanes.HONEST)

# A division by multiplication with the correctly rounded reciprocal is NOT honest: the header's derivation counts `the
# division u`, one rounding, and the product with a rounded reciprocal has two.  It is in FAULTS.  It is also the one fault no
# check can see, and UNSEEN says why; the CPU harness asserts that it is the only one.
UNSEEN = {
    "division_by_rounded_reciprocal": "the stated bounds keep a margin of (L + 2 T + 12) u over their own derivation, so one more u is inside "
                                      "them, and no tolerance derived as a worst case resolves a single u beside the exponentials' 2 u each; "
                                      "wherever the answer is exact (tie rows, equal scores, rows of one entry) every numerator is a power of "
                                      "two, and fl(2^k * fl(1 / sum)) = fl(2^k / sum): the same bits.  f32 REFERENCE rounds the fp64 quotient "
                                      "to fp32, which hides 2^-53.",
}

# Faults no output of SOME case can expose, and why; each is still caught on another case (UNSEEN apart).
EQUIVALENT_WHERE = {
    "max_never_subtracted": "in real arithmetic every m gives the same softmax; where no exponential overflows the accumulator's type or "
                            "underflows it (the suite's scores stay inside +-60, REFERENCE and f64 compute in fp64) only roundings differ.",
    "max_from_first_walk_step": "the same; and a row of up to 256 entries has one step.  The suite's +Inf sits at entry 7 of its row.",
    "max_from_own_group": "where G lanes own the row, or G = 64, the group is the owner; and where every group of lanes holds the same maximum "
                          "(tie rows whose tied entries reach every group).",
    "second_walk_one_step_short": "a row of up to 4 W entries is not walked.",
    "last_register_slot_dropped": "every row whose length is not exactly 4 W.",
    "butterfly_skips_widest_step": "a row that lives in one half of its lanes: L <= W / 2.",
    "ref_exp_in_fp32": "f32 FAST and both f64 modes do not take this path.",
    "ref_sum_rounded_to_fp32": "a sum that fp32 holds exactly: tie rows, equal scores.",
    "f64_sum_in_fp32": "the same; and the f32 kernels.",
    "fast_log2e_in_bf16": "t = 0: the maxima of a row, tie rows.  REFERENCE and f64 have no such constant.",
    "ref_dot_in_fp32": "products and sums that fp32 holds exactly: tie rows.",
    "fast_scaled_before_difference": "s = m: the maxima of a row, tie rows.  REFERENCE and f64 do not scale.",
    "single_entry_row_keeps_dp": "every row of more than one entry.",
    "fast_dot_unfused": "products that the type holds exactly: tie rows.  REFERENCE: f64 rounds apart by contract, f32 has exact products.",
    "bsr_dot_unfused": "products that fp32 holds exactly: tie rows, a bf16 p times small integers.",
    "z_two_roundings": "without a mask; and with a power-of-two scale, where scale * s is exact and both forms are one rounding of the same "
                       "number -- the suite's scale 0.125 and 1.0.",
    "z_without_mask_on_second_pass": "without a mask; block rows of up to C blocks are not walked.",
    "mask_scaled_with_scores": "without a mask, or with scale = 1.",
    "max_shared_in_block_row": "as max_never_subtracted: real arithmetic does not see which finite maximum is subtracted.",
    "wave3_lost": "block rows of up to 3 blocks: wave 3 holds nothing.",
    "block_c_dropped_when_full": "every block row that does not hold exactly C blocks.",
    "walk_starts_at_w_plus_4": "block rows of up to C blocks.",
    "bf16_out_truncated": "fp32 out; results that bf16 holds exactly (tie rows: 1 / t).",
    "bf16_out_from_bf16_sum": "fp32 out; sums that bf16 holds exactly (tie rows: t).",
    "scale_applied_twice": "scale = 1.",
    "scale_dropped": "scale = 1.",
    "bf16_p_read_as_high_half": "an fp32 p.",
    "dot_over_first_c_blocks": "block rows of up to C blocks.",
    "bf16_ds_truncated": "fp32 ds.",
}

CSR_NAMES = ("edges", "edges-g4", "edges-g8", "edges-g16", "edges-g64")
BSR_NAMES = ("edges16", "edges32")
BSR_SCALES = (1.0, 0.125, 0.3)
OLD = ("stated_bound", "row_sums", "anchors", "specials")
NEW = ("tight", "tie_rows", "offset_rows", "lane_bits")


def family_of(fault):
    for fam, names in (("csr_fwd", lanes.CSR_FWD_FAULTS), ("csr_bwd", lanes.CSR_BWD_FAULTS), ("bsr_fwd", lanes.BSR_FWD_FAULTS),
                       ("bsr_bwd", lanes.BSR_BWD_FAULTS)):
        if fault in names:
            return (fam,)
    return ("csr_fwd", "csr_bwd", "bsr_fwd", "bsr_bwd")            # an honest variant: everywhere


def case_id(case):
    return ",".join(str(x) for x in case)


@functools.lru_cache(maxsize=None)
def cases_of(check, family):
    """The cases a check runs on, in the suite's order."""
    kernel, direction = family.split("_")
    if kernel == "csr":
        def every(kinds):
            return tuple(CsrCase(direction, n, k, a) for n in CSR_NAMES for k in kinds for a in lanes.ARITH)
        if direction == "fwd":
            kinds = {"stated_bound": ("narrow", "wide"), "row_sums": ("narrow", "wide"), "anchors": ("equal", "wide"), "specials": ("specials",),
                     "tight": ("narrow", "wide", "specials"), "tie_rows": tuple(f"tie{t}" for t in tight.TIES), "offset_rows": ("offset",),
                     "lane_bits": ()}
        else:
            kinds = {"stated_bound": ("narrow", "wide"), "row_sums": (), "anchors": ("zero_dp",), "specials": (),
                     "tight": ("narrow", "wide"), "tie_rows": tuple(f"tie{t}" for t in tight.TIES), "offset_rows": ("offset",),
                     "lane_bits": ("narrow", "offset")}
        return every(kinds[check])
    both = (False, True)
    if direction == "fwd":
        def fwd(kind, scales, masks):
            return tuple(BsrCase("fwd", n, kind, s, m, False, o) for n in BSR_NAMES for m in masks for s in scales for o in both)
        if check in ("stated_bound", "tight"):
            return fwd("narrow", BSR_SCALES, both) + fwd("wide", BSR_SCALES, both) + (fwd("specials", (0.3,), (True,)) if check == "tight" else ())
        if check == "row_sums":
            return tuple(c for c in cases_of("stated_bound", family) if not c.out_bf16)
        if check == "anchors":
            return fwd("equal", (0.3,), (False,))
        if check == "specials":
            return fwd("specials", (0.3,), (True,))
        if check == "tie_rows":
            return tuple(c for t in tight.TIES for c in fwd(f"tie{t}", (tight.TIE_SCALE,), both))
        if check == "lane_bits":
            return ()
        return fwd("offset", (0.3,), (True,)) + fwd("offset", (0.125,), (False,))

    def bwd(kind, scales):
        return tuple(BsrCase("bwd", n, kind, s, False, pb, o) for n in BSR_NAMES for s in scales for pb in both for o in both)
    if check in ("stated_bound", "tight"):
        return bwd("narrow", (1.0, 0.3)) + bwd("wide", (1.0, 0.3))
    if check == "anchors":
        return bwd("zero_dp", (0.3,))
    if check == "tie_rows":
        return tuple(c for t in tight.TIES for c in bwd(f"tie{t}", (tight.TIE_SCALE,)))
    if check == "offset_rows":
        return bwd("offset", (0.125,))
    if check == "lane_bits":
        return bwd("narrow", (1.0, 0.3)) + bwd("offset", (0.125,))
    return ()


def restate(case, fault=None):
    """The lane-order restatement on a case's operands; bf16 results as float32 values."""
    if isinstance(case, CsrCase):
        op = tight.csr_operands(case)
        if case.direction == "fwd":
            return lanes.csr_forward(op["row_ptrs"], op["s"], case.arith, op["group"], fault)
        return lanes.csr_backward(op["row_ptrs"], op["p"], op["dp"], case.arith, op["group"], fault)
    op = tight.bsr_operands(case)
    if case.direction == "fwd":
        return lanes.bsr_forward(op["ptrs"], op["bs"], op["s"], op["mask"], case.scale, case.out_bf16, fault)
    return lanes.bsr_backward(op["ptrs"], op["bs"], op["p"], op["dp"], case.scale, case.p_bf16, case.out_bf16, fault)


@functools.lru_cache(maxsize=1024)
def restated(case, fault=None):
    out = restate(case, fault)
    out.setflags(write=False)
    return out


# ---- OLD: what the two GPU suites held before the tight file
def stated_bound(got, case):
    """Inside the header's bound, on the elements the contract leaves finite: (ok, worst |err| / bound)."""
    exact, _, dead = tight.reference(case)
    live = ~dead
    with np.errstate(invalid="ignore"):
        err = np.abs(np.asarray(got).astype(cref.LD)[live] - exact[live]).astype(np.float64)
    err = np.where(np.isnan(err), np.inf, err)
    lim = tight.stated_bound(case)[live]
    return bool(np.all(err <= lim)), float(np.max(np.where(err == 0, 0.0, err / lim), initial=0.0))


def row_sums(got, case):
    """Every row's quotients sum to 1 within L u of the out type's mode."""
    if isinstance(case, CsrCase):
        sums, lens = cref.row_sums(tight.csr_operands(case)["row_ptrs"], got)
        u = 2.0 ** -24 if case.arith.startswith("f32") else 2.0 ** -53
    else:
        sums, lens = bref.row_sums(case.name, got)
        u = 2.0 ** -24
    off = np.abs(sums - 1).astype(np.float64)
    off = np.where(np.isnan(off), np.inf, off)
    return bool(np.all(off <= lens * u)), float(np.max(off / (lens * u), initial=0.0))


def anchors(got, case):
    """Equal scores: the correctly rounded 1 / L (CSR: REFERENCE and f64; BSR: the fp32 quotient, then bf16).  A row of one entry:
    exactly 1.  The backward of an all-zero dp: all +0."""
    got = np.asarray(got)
    if case.kind == "zero_dp":
        return bool(not got.any() and not np.signbit(got).any()), 0.0
    if isinstance(case, CsrCase):
        length = cref.row_lengths(tight.csr_operands(case)["row_ptrs"])
        if case.kind == "wide":
            return bool(np.all(got[length == 1] == 1.0)), 0.0
        if case.arith == "f32,fast":
            return True, 0.0
        want = (cref.LD(1.0) / length.astype(cref.LD)).astype(got.dtype)
        return bool(np.array_equal(got, want)), 0.0
    want = (np.float32(1.0) / bref.lengths(case.name).astype(np.float32)).astype(np.float32)
    return bool(np.array_equal(got, bref.bf16_round(want) if case.out_bf16 else want)), 0.0


def specials(got, case):
    """NaN exactly where the contract says (CSR: the rows with a NaN, a +Inf, nothing but -Inf; BSR: those matrix rows and no
    other row of their blocks), a masked entry beside a finite one exactly +0, every other element inside the stated bound."""
    got = np.asarray(got)
    _, _, dead = tight.reference(case)
    if isinstance(case, CsrCase):
        hidden = np.isneginf(tight.csr_operands(case)["s"]) & ~dead
    else:
        hidden = np.isneginf(tight.bsr_z(case)) & ~dead
    ok = bool(np.array_equal(np.isnan(got), dead)) and not got[hidden].any() and not np.signbit(got[hidden]).any()
    inside, worst = stated_bound(got, case)
    return ok and inside, worst


# ---- NEW
def tight_check(got, case):
    return tight.tight(got, case)


def tie_rows(got, case):
    ok, wrong = tight.tie_check(got, case)
    return ok, float(wrong)


def lane_bits(got, case):
    """The backward has no exponential: a kernel that keeps the lane order gives the restatement's bits.  On operands in the
    normal range (narrow and offset rows), where no product can be flushed."""
    want = restated(case)
    got = np.ascontiguousarray(got, dtype=want.dtype)
    bits = np.uint32 if want.dtype == np.float32 else np.uint64
    wrong = int((got.view(bits) != want.view(bits)).sum())
    return wrong == 0, float(wrong)


CHECKS = collections.OrderedDict([("stated_bound", stated_bound), ("row_sums", row_sums), ("anchors", anchors), ("specials", specials),
                                  ("tight", tight_check), ("tie_rows", tie_rows), ("offset_rows", tight_check), ("lane_bits", lane_bits)])
