"""Mutation check of the row-softmax tests (CSR and BSR), on a machine WITHOUT a GPU.  Every fault of tests/_softmax_mutants.py is
put into the lane-order restatement of its kernel (tests/_softmax_lanes.py) and the faulty output is run through the checks the
GPU suites apply to the kernels' output (_softmax_mutants.CHECKS), on the suites' own operands and in the suites' order: first
what tests/test_gpu_softmax.py and tests/test_gpu_softmax_bsr.py held before (OLD: the stated bounds, the row sums, the
exactness anchors, the special values), then tests/_softmax_tight.py (NEW: the derived tight tolerance, the tie rows, the
offset rows, the backward's lane bits).

Held here: the restatements and three honest variants pass every check, at most 1 x the tight tolerance; the tight tolerance
covers every element that is finite by contract and is element by element no looser than the stated bound; every fault but
one fails a check, and CAUGHT_BY records for each the first OLD check (the `before` column: what a checkout of the parent's
tests would have caught) and the first NEW one; STATED_BOUNDS_ALONE_LET_THROUGH are the faults whose `before` is None.

What came out.  (1) A forward that never subtracts the maximum IS caught by an old check that is easy to miss: the equal-scores
anchor of REFERENCE and f64 (exp(0.7) / (L exp(0.7)) is not the correctly rounded 1 / L); in f32 FAST only the one +Inf row of
the special values sees it.  (2) A maximum from the first walk step, a FAST exponent scaled before the difference, an
unfused dot in the FAST and block backward and a z of two roundings pass every old check.  (3) The two-rounding z is the
IDENTITY at the suite's scales 0.125 and 1.0 (the product is exact), which is why it sat at the correct form's ratio there;
at scale 0.3 it is caught by the tight tolerance and, by a factor of hundreds, on the offset rows.  (4) A division by
multiplication with the rounded reciprocal breaks the derivation's `the division u` and is seen by no check
(_softmax_mutants.UNSEEN says why none can)."""
import re

import numpy as np
import pytest

import _softmax_lanes as lanes
import _softmax_mutants as mut
import _softmax_ref as cref
import _softmax_tight as tight

FAMILIES = ("csr_fwd", "csr_bwd", "bsr_fwd", "bsr_bwd")


def first_catch(fault, only=None, keep=lambda case: True):
    """(check, case id) of the first check, in the suite's order, that the faulty restatement fails, and its first case; None:
    it survives."""
    with np.errstate(all="ignore"):
        for name, check in mut.CHECKS.items():
            if only is not None and name not in only:
                continue
            for family in mut.family_of(fault):
                for case in mut.cases_of(name, family):
                    if keep(case) and not check(mut.restated(case, fault), case)[0]:
                        return name, mut.case_id(case)
    return None


def test_the_catalogue_names_the_header_words_every_fault_breaks():
    assert len(mut.FAULTS) >= 31 and len(mut.HONEST) >= 3
    for name, sentence in mut.FAULTS.items():
        assert "`" in sentence and " -- " in sentence, name
    assert set(CAUGHT_BY) == set(mut.FAULTS) and set(mut.EQUIVALENT_WHERE) <= set(mut.FAULTS) and set(mut.UNSEEN) <= set(mut.FAULTS)
    with open(mut.__file__.replace("tests/_softmax_mutants.py", "include/mispmm.h"), encoding="utf-8") as f:
        text = f.read()
    lo, mid, hi = (text.index(mark) for mark in ("Row softmax on a CSR pattern */", "SDDMM on a BSR pattern, bf16 */", "Row softmax on a BSR pattern */"))
    end = text.index("dense helpers */")
    sections = {"csr": text[lo:mid], "bsr": text[hi:end]}
    sections = {k: " ".join(re.sub(r"^ \* ?", "", v, flags=re.M).split()) for k, v in sections.items()}
    for name, sentence in mut.FAULTS.items():
        section = sections[mut.family_of(name)[0][:3]]
        for part in sentence.split("`")[1].split(" ... "):
            assert " ".join(part.split()) in section, f"{name}: the header's section does not say `{part}`"
    csr = cref.matrix("edges")
    with pytest.raises(ValueError, match="unknown fault"):
        lanes.csr_forward(csr.row_ptrs, np.zeros(csr.nnz, np.float32), "f32,fast", 32, fault="no_such_fault")
    with pytest.raises(ValueError, match="unknown fault"):
        lanes.bsr_backward(np.array([0, 1]), 16, np.zeros((1, 16, 16)), np.zeros((1, 16, 16)), 1.0, fault="no_such_fault")


@pytest.mark.parametrize("arith", list(tight.TIE_OFFSET))
def test_tie_rows_the_offset_overflows_and_the_gap_underflows_in_every_arithmetic(arith):
    assert tight.tie_premises(arith)


@pytest.mark.parametrize("name", mut.CSR_NAMES + mut.BSR_NAMES)
def test_tie_rows_meet_every_slot_lane_step_wave_and_the_blocks_around_c(name):
    seen = tight.bsr_tie_coverage(name) if name in mut.BSR_NAMES else tight.csr_tie_coverage(name)
    print(name, seen)
    if name in mut.CSR_NAMES:
        assert seen["group"] == (32 if name == "edges" else int(name.split("-g")[1]))
assert {4, 8, 16, 32, 64} == {32 if n == "edges" else int(n.split("-g")[1]) for n in mut.CSR_NAMES}          # every G


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("variant", [None] + list(mut.HONEST))
def test_the_restatement_and_the_honest_variants_pass_every_check(variant, family):
    worst = {}
    with np.errstate(all="ignore"):
        for name, check in mut.CHECKS.items():
            if name == "lane_bits" and variant is not None:
                continue                # the one check that holds the ORDER of the sums: a variant in another order has other bits
            for case in mut.cases_of(name, family):
                ok, ratio = check(mut.restated(case, variant), case)
                assert ok, f"{variant}: {name} fails on {mut.case_id(case)} ({ratio:.3g})"
                if name in ("tight", "offset_rows"):
                    key = case.arith if isinstance(case, tight.CsrCase) else ("bsr,bf16" if case.out_bf16 else "bsr,f32")
                    worst[key] = max(worst.get(key, 0.0), ratio)
    print(f"{variant} {family}: worst |err| / tight tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert worst and max(worst.values()) <= 1.0


@pytest.mark.parametrize("family", FAMILIES)
def test_the_tight_tolerance_covers_every_finite_element_and_is_no_looser_than_the_stated_bound(family):
    for name in ("tight", "offset_rows"):
        for case in mut.cases_of(name, family):
            exact, tol, dead = tight.reference(case)
            assert tol.shape == exact.shape == dead.shape and np.all(np.isfinite(tol[~dead])) and np.all(tol[~dead] > 0), mut.case_id(case)
            assert np.array_equal(dead, np.isnan(exact)) and (case.kind == "specials") == bool(dead.any()), mut.case_id(case)
            stated = tight.stated_bound(case)
            looser = tol[~dead] > stated[~dead]
            assert not looser.any(), f"{mut.case_id(case)}: {int(looser.sum())} elements have a tight tolerance above the stated bound"


# fault -> (before: the first OLD check that fails and its first case -- what the parent's tests would have caught --,
#           after: the first NEW check that fails and its first case)
CAUGHT_BY = {
    "max_never_subtracted": (("anchors", "fwd,edges,equal,f64,ref"), ("tight", "fwd,edges,wide,f32,fast")),
    "max_from_first_walk_step": (None, ("tie_rows", "fwd,edges,tie1,f32,ref64")),
    "max_from_own_group": (("stated_bound", "fwd,edges,narrow,f32,ref64"), ("tight", "fwd,edges,narrow,f32,ref64")),
    "second_walk_one_step_short": (("stated_bound", "fwd,edges,narrow,f32,ref64"), ("tight", "fwd,edges,narrow,f32,ref64")),
    "last_register_slot_dropped": (("stated_bound", "fwd,edges,narrow,f32,ref64"), ("tight", "fwd,edges,narrow,f32,ref64")),
    "last_entry_dropped": (("stated_bound", "fwd,edges,narrow,f32,ref64"), ("tight", "fwd,edges,narrow,f32,ref64")),
    "dead_slot_counts_one": (("stated_bound", "fwd,edges,narrow,f32,ref64"), ("tight", "fwd,edges,narrow,f32,ref64")),
    "butterfly_skips_widest_step": (("stated_bound", "fwd,edges,narrow,f32,ref64"), ("tight", "fwd,edges,narrow,f32,ref64")),
    "ref_exp_in_fp32": (("stated_bound", "fwd,edges,narrow,f32,ref64"), ("tight", "fwd,edges,narrow,f32,ref64")),
    "ref_sum_rounded_to_fp32": (("stated_bound", "fwd,edges,narrow,f32,ref64"), ("tight", "fwd,edges,narrow,f32,ref64")),
    "f64_sum_in_fp32": (("stated_bound", "fwd,edges,narrow,f64,ref"), ("tight", "fwd,edges,narrow,f64,ref")),
    "fast_log2e_in_bf16": (("stated_bound", "fwd,edges,narrow,f32,fast"), ("tight", "fwd,edges,narrow,f32,fast")),
    "fast_scaled_before_difference": (None, ("tight", "fwd,edges,wide,f32,fast")),
    "division_by_rounded_reciprocal": (None, None),
    "dot_from_first_walk_step": (("stated_bound", "bwd,edges,narrow,f32,ref64"), ("tight", "bwd,edges,narrow,f32,ref64")),
    "dot_misses_last_slot": (("stated_bound", "bwd,edges,narrow,f32,ref64"), ("tight", "bwd,edges,narrow,f32,ref64")),
    "ref_dot_in_fp32": (("stated_bound", "bwd,edges,narrow,f32,ref64"), ("tight", "bwd,edges,narrow,f32,ref64")),
    "single_entry_row_keeps_dp": (("stated_bound", "bwd,edges,narrow,f32,ref64"), ("tight", "bwd,edges,narrow,f32,ref64")),
    "ds_from_p_dp_minus_dot": (("stated_bound", "bwd,edges,narrow,f32,ref64"), ("tight", "bwd,edges,narrow,f32,ref64")),
    "fast_dot_unfused": (None, ("lane_bits", "bwd,edges,narrow,f32,fast")),
    "z_two_roundings": (None, ("tight", "fwd,edges16,wide,0.3,True,False,False")),
    "z_without_mask_on_second_pass": (("stated_bound", "fwd,edges16,narrow,1.0,True,False,False"), ("tight", "fwd,edges16,narrow,1.0,True,False,False")),
    "mask_scaled_with_scores": (("stated_bound", "fwd,edges16,narrow,0.125,True,False,False"), ("tight", "fwd,edges16,narrow,0.125,True,False,False")),
    "max_shared_in_block_row": (("stated_bound", "fwd,edges16,wide,1.0,False,False,False"), ("tight", "fwd,edges16,wide,1.0,False,False,False")),
    "wave3_lost": (("stated_bound", "fwd,edges16,narrow,1.0,False,False,False"), ("tight", "fwd,edges16,narrow,1.0,False,False,False")),
    "block_c_dropped_when_full": (("stated_bound", "fwd,edges16,narrow,1.0,False,False,False"), ("tight", "fwd,edges16,narrow,1.0,False,False,False")),
    "walk_starts_at_w_plus_4": (("stated_bound", "fwd,edges16,narrow,1.0,False,False,False"), ("tight", "fwd,edges16,narrow,1.0,False,False,False")),
    "bf16_out_truncated": (("stated_bound", "fwd,edges16,narrow,1.0,False,False,True"), ("tight", "fwd,edges16,narrow,1.0,False,False,True")),
    "bf16_out_from_bf16_sum": (("stated_bound", "fwd,edges16,narrow,1.0,False,False,True"), ("tight", "fwd,edges16,narrow,1.0,False,False,True")),
    "scale_applied_twice": (("stated_bound", "bwd,edges16,narrow,0.3,False,False,False"), ("tight", "bwd,edges16,narrow,0.3,False,False,False")),
    "scale_dropped": (("stated_bound", "bwd,edges16,narrow,0.3,False,False,False"), ("tight", "bwd,edges16,narrow,0.3,False,False,False")),
    "bf16_p_read_as_high_half": (("stated_bound", "bwd,edges16,narrow,1.0,False,True,False"), ("tight", "bwd,edges16,narrow,1.0,False,True,False")),
    "dot_over_first_c_blocks": (("stated_bound", "bwd,edges16,narrow,1.0,False,False,False"), ("tight", "bwd,edges16,narrow,1.0,False,False,False")),
    "bf16_ds_truncated": (("stated_bound", "bwd,edges16,narrow,1.0,False,False,True"), ("tight", "bwd,edges16,narrow,1.0,False,False,True")),
    "bsr_dot_unfused": (None, ("lane_bits", "bwd,edges16,narrow,1.0,False,False,False")),
}
# The faults that every check of the two GPU suites as they stood lets through, on every case: the finding of this work.
STATED_BOUNDS_ALONE_LET_THROUGH = ("max_from_first_walk_step", "fast_scaled_before_difference", "fast_dot_unfused", "z_two_roundings",
                                   "bsr_dot_unfused")


@pytest.mark.parametrize("fault", list(mut.FAULTS))
def test_every_fault_fails_a_check_and_the_first_to_catch_it_before_and_after_are_the_recorded_ones(fault):
    before, after = first_catch(fault, only=mut.OLD), first_catch(fault, only=mut.NEW)
    print(f"{fault}: before {before}, after {after}")
    assert (before, after) == CAUGHT_BY[fault], (fault, before, after)
    if fault in mut.UNSEEN:
        assert before is None and after is None
    else:
        assert after is not None, f"{fault} survives every new check on every case"      # the new checks stand on their own
    assert (before is None and fault not in mut.UNSEEN) == (fault in STATED_BOUNDS_ALONE_LET_THROUGH)


def test_the_let_through_list_is_not_empty_and_one_fault_alone_is_unseen():
    assert len(STATED_BOUNDS_ALONE_LET_THROUGH) >= 2 and set(mut.UNSEEN) == {"division_by_rounded_reciprocal"}
    assert [f for f, (before, after) in CAUGHT_BY.items() if after is None] == list(mut.UNSEEN)


def test_a_forward_that_never_subtracts_the_maximum_is_caught_before_but_in_fast_by_the_one_inf_row_only():
    """In REFERENCE and f64 the equal-scores anchor sees it (the quotient of exp(0.7) and L exp(0.7) is not the correctly rounded
    1 / L).  In f32 FAST the anchor does not apply, the stated bound passes on narrow and wide scores alike, and only the one
    row of the special values that holds a +Inf tells m = 0 from m = max; the tie rows' offset overflows outright."""
    fast = lambda case: case.arith == "f32,fast"                    # noqa: E731
    assert first_catch("max_never_subtracted", only=("stated_bound", "row_sums", "anchors"), keep=fast) is None
    assert first_catch("max_never_subtracted", only=mut.OLD, keep=fast) == ("specials", "fwd,edges,specials,f32,fast")
    for arith in lanes.ARITH:
        assert first_catch("max_never_subtracted", only=("tie_rows",), keep=lambda case: case.arith == arith) is not None


def test_the_two_rounding_z_is_the_identity_at_a_power_of_two_scale_and_caught_on_the_offset_rows():
    same = []
    for case in mut.cases_of("stated_bound", "bsr_fwd"):
        if case.mask and case.name == "edges16" and not case.out_bf16:
            same.append((case.scale, np.array_equal(mut.restated(case, "z_two_roundings"), mut.restated(case), equal_nan=True)))
    assert {s for s, eq in same if eq} == {1.0, 0.125} and {s for s, eq in same if not eq} == {0.3}, same
    assert first_catch("z_two_roundings", only=mut.OLD) is None
    for name in mut.BSR_NAMES:
        case = tight.BsrCase("fwd", name, "offset", 0.3, True, False, False)             # the mask carries the offset
        z, z2 = tight.bsr_z(case), lanes._z(tight.bsr_operands(case)["s"], tight.bsr_operands(case)["mask"], 0.3, "z_two_roundings")
        moved = int((z != z2).sum())
        ok, worst = tight.tight(mut.restated(case, "z_two_roundings"), case)
        print(f"{name}: {moved} of {z.size} z differ by an ulp; worst |err| / tight tolerance {worst:.3g}")
        assert 0 < moved < z.size // 200 and not ok and worst > 10.0
        assert tight.tight(mut.restated(case), case)[0]
        still = tight.BsrCase("fwd", name, "offset", 0.125, False, False, False)          # no mask: nothing to round twice
        assert np.array_equal(mut.restated(still, "z_two_roundings"), mut.restated(still))


def test_faults_that_are_the_identity_somewhere_are_the_identity_there():
    same = lambda case, fault: np.array_equal(mut.restated(case, fault), mut.restated(case), equal_nan=True)     # noqa: E731
    fwd, bwd = (lambda *a: tight.CsrCase("fwd", *a)), (lambda *a: tight.CsrCase("bwd", *a))
    for case, fault in ((fwd("edges", "narrow", "f32,fast"), "ref_exp_in_fp32"), (fwd("edges", "narrow", "f64,ref"), "ref_sum_rounded_to_fp32"),
                        (fwd("edges", "narrow", "f32,ref64"), "f64_sum_in_fp32"), (fwd("edges", "narrow", "f64,fast"), "fast_log2e_in_bf16"),
                        (fwd("edges-g64", "narrow", "f32,fast"), "max_from_own_group"), (fwd("edges", "tie4", "f32,ref64"), "ref_sum_rounded_to_fp32"),
                        (fwd("edges", "tie4", "f32,fast"), "fast_log2e_in_bf16"), (fwd("edges", "tie2", "f32,fast"), "fast_scaled_before_difference"),
                        (bwd("edges", "tie4", "f32,ref64"), "ref_dot_in_fp32"), (bwd("edges", "tie8", "f64,fast"), "fast_dot_unfused"),
                        (bwd("edges", "narrow", "f64,ref"), "fast_dot_unfused"),
                        (tight.BsrCase("fwd", "edges16", "narrow", 0.3, False, False, False), "mask_scaled_with_scores"),
                        (tight.BsrCase("fwd", "edges16", "narrow", 1.0, True, False, False), "mask_scaled_with_scores"),
                        (tight.BsrCase("fwd", "edges16", "narrow", 0.3, True, False, False), "bf16_out_truncated"),
                        (tight.BsrCase("fwd", "edges16", "tie4", 0.125, True, False, True), "bf16_out_truncated"),
                        (tight.BsrCase("fwd", "edges16", "tie8", 0.125, False, False, True), "bf16_out_from_bf16_sum"),
                        (tight.BsrCase("bwd", "edges16", "narrow", 1.0, False, False, False), "scale_dropped"),
                        (tight.BsrCase("bwd", "edges16", "narrow", 1.0, False, True, False), "scale_applied_twice"),
                        (tight.BsrCase("bwd", "edges16", "narrow", 0.3, False, False, True), "bf16_p_read_as_high_half"),
                        (tight.BsrCase("bwd", "edges32", "tie4", 0.125, False, True, False), "bsr_dot_unfused")):
        assert same(case, fault), (fault, mut.case_id(case))
    # where nothing overflows only roundings tell which maximum was subtracted: inside every stated bound
    for arith in lanes.ARITH:
        for kind in ("narrow", "wide"):
            case = fwd("edges", kind, arith)
            for fault in ("max_never_subtracted", "max_from_first_walk_step"):
                assert mut.stated_bound(mut.restated(case, fault), case)[0], (fault, mut.case_id(case))


# ---- tie rows: exact answers, no tolerance
def test_tie_rows_catch_faults_without_any_tolerance():
    """Not every fault moves an exact answer (EQUIVALENT_WHERE: sums and products that the narrower type holds exactly, t = 0 in
    the exponent, a maximum that every group of lanes holds); the faults of structure do, bit for bit."""
    silent = {"ref_exp_in_fp32", "ref_sum_rounded_to_fp32", "f64_sum_in_fp32", "fast_log2e_in_bf16", "fast_scaled_before_difference",
              "division_by_rounded_reciprocal", "ref_dot_in_fp32", "fast_dot_unfused", "z_two_roundings", "bf16_out_truncated",
              "bf16_out_from_bf16_sum", "bsr_dot_unfused", "mask_scaled_with_scores", "max_shared_in_block_row", "bf16_ds_truncated"}
    for fault in mut.FAULTS:
        caught = first_catch(fault, only=("tie_rows",))
        print(f"tie rows {fault}: {caught if caught else 'not seen'}")
        assert (caught is None) == (fault in silent), fault
