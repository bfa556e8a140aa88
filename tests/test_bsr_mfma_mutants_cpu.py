"""Mutation check of the tests of the bf16 block-sparse MFMA products, on a machine WITHOUT a GPU.  Every fault of
tests/_bsr_mfma_mutants.py is put into the lane-order restatement of its kernel (tests/_bsr_mfma_lanes.py) and the faulty C is run
through the checks the GPU suites apply: first what they held before (OLD: |got - oracle| <= 2e-6 scale (+ 2^-8 |ref|) on the
census's operands and the ragged slots case, the census's integer kind bit for bit, its sentinel), then tests/_bsr_mfma_tight.py
(NEW: the derived bound, the exact family, the special values, the untouched elements).

What came out.  Four faults pass every old check on every old case and are caught by the special values alone: the missing half
of an odd pair, a padding slot (as column 0 or as column K - 1) and an unoccupied column each put a zero coefficient in front
of a B row nobody may read, and 0 * b is +0 for every finite b.  Two faults no check of C can see (_bsr_mfma_mutants.UNSEEN).
The derived tolerance g_n S is NOT below 2e-6 S where an element has more than 16 additions (2e-6 = 16.8 u), so no existing
assertion is replaced by it; for a bf16 C it is far inside the 2^-8 |ref| the old tests add."""
import os
import re

import numpy as np
import pytest

import _bsr_mfma_lanes as lanes
import _bsr_mfma_mutants as mut
import _bsr_mfma_tight as tight


def first_catch(fault, only):
    """(check, case id) of the first check of `only`, in the suite's order, that the faulty restatement fails; None: it survives."""
    for name in only:
        for kernel in mut.family_of(fault):
            for case in mut.cases_of(name, kernel):
                if not mut.CHECKS[name](mut.restated(case, fault), case)[0]:
                    return name, tight.case_id(case)
    return None


def _words(path):
    with open(path, encoding="utf-8") as f:
        return " ".join(re.sub(r"^\s*(//|/?\*+/?) ?", "", f.read(), flags=re.M).split())


def test_the_catalogue_quotes_the_words_every_fault_breaks():
    assert len(mut.FAULTS) >= 25 and len(mut.HONEST) >= 3
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = _words(os.path.join(root, "include", "mispmm.h")) + " " + _words(os.path.join(root, "cuda-optimization-for-spmm_amd", "csrc", "bsr_mfma_tiles.hpp"))
    for name, sentence in mut.FAULTS.items():
        assert sentence.count("`") == 2 and " -- " in sentence and "\n" not in sentence, name
        assert " ".join(sentence.split("`")[1].split()) in text, f"{name}: neither file says `{sentence.split('`')[1]}`"
    assert set(CAUGHT_BY) == set(mut.FAULTS) and set(mut.UNSEEN) <= set(mut.FAULTS)
    case = mut.new_cases("bsr16", "tight")[0]
    bsr = tight.operands(case)["bsr"]
    args = (tight.b_flat(case), bsr.num_cols, case.n, case.ldb, case.ldc, False)
    for fn, head in ((lanes.bsr16, (bsr.block_row_ptrs, bsr.block_col_idxs, bsr.data)), (lanes.bsrc, lanes.compact(bsr))):
        with pytest.raises(ValueError, match="unknown fault"):
            fn(*head, *args, fault="no_such_fault")
    with pytest.raises(ValueError, match="unknown fault"):
        lanes.slots(*lanes.compact_slots(bsr), *args, False, fault="no_such_fault")
    with pytest.raises(ValueError, match="unknown fault"):
        mut.restated(case, "no_such_fault")


@pytest.mark.parametrize("kernel", mut.ALL)
@pytest.mark.parametrize("variant", [None] + list(mut.HONEST))
def test_the_restatement_and_the_honest_variants_pass_every_check(variant, kernel):
    worst = {}
    for name in mut.OLD + mut.NEW:
        for case in mut.cases_of(name, kernel):
            ok, ratio = mut.CHECKS[name](mut.restated(case, variant), case)
            assert ok, f"{variant}: {name} fails on {tight.case_id(case)} ({ratio:.3g})"
            if name in ("tight", "specials"):
                key = "bf16 C" if case.out_bf16 else "fp32 C"
                worst[key] = max(worst.get(key, 0.0), ratio)
    print(f"{variant} {kernel}: worst |err| / tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert worst and max(worst.values()) <= 1.0


@pytest.mark.parametrize("kernel", mut.ALL)
def test_the_cases_meet_their_premises(kernel):
    """The flagged share of every bf16-C case is under the cap; the exact family's premise holds on every case and the family
    holds ties of the bf16 rounding in both parities; the special values reach every place the contract names."""
    for kind in ("tight", "specials"):
        for case in mut.new_cases(kernel, kind):
            exact, tol, dead, _ = tight.reference(case)
            assert np.all(tol[~dead] >= 0) and np.all(np.isfinite(tol)) and (kind == "specials") == bool(dead.any()), tight.case_id(case)
            if case.out_bf16:
                share = tight.flagged(case).sum() / (~dead).sum()
                assert share <= tight.FLAG_CAP, f"{tight.case_id(case)}: {share:.3%} flagged"
            if kind == "specials":
                assert np.isnan(exact).any() and (exact == np.inf).any() and (exact == -np.inf).any() and (~dead).sum() > dead.sum()
                b, planted = tight.operands(case)["b"], tight.operands(case)["planted"]
                assert not np.isfinite(b[0]).all() and not np.isfinite(b[-1]).all() and 0 not in planted["used"]
                assert (len(planted["idle"]) > 0) == (kernel in mut.COMPACT)
    down = up = 0
    for case in mut.new_cases(kernel, "sharp"):
        assert tight.sharp_premise(case), tight.case_id(case)
        d, u = tight.sharp_ties(case)
        down, up = down + d, up + u
    print(f"{kernel}: {down} ties round down to even, {up} round up")
    assert down >= 4 and up >= 4


@pytest.mark.parametrize("kernel", mut.ALL)
def test_the_tight_tolerance_against_the_constant_of_the_old_tests(kernel):
    """fp32 C: g_n S <= 2e-6 S exactly where n <= 16 (2e-6 = 16.8 u), and there are elements on both sides: the derived bound is
    a function of the number of additions, the constant was not, and neither may replace the other.  bf16 C: every interval end
    lies inside the old 2^-8 |ref| + 2e-6 S where n <= 16."""
    small = large = 0
    for case in mut.new_cases(kernel, "tight"):
        exact, tol, dead, scale = tight.reference(case)
        with np.errstate(invalid="ignore", divide="ignore"):
            n = np.where(scale > 0, tol / np.where(scale > 0, scale, 1.0), 0.0)
        n = n / (1.0 + n) / tight.U
        live = scale > 0
        assert np.array_equal((tol <= 2e-6 * scale)[live], (n <= 16.5)[live]), tight.case_id(case)
        small, large = small + int((live & (n <= 16.5)).sum()), large + int((n > 16.5).sum())
        if case.out_bf16:
            lo, hi = tight._ends16(exact, tol)
            old = 2.0 ** -8 * np.abs(exact) + 2e-6 * scale
            ok = (np.abs(lo - exact) <= old) & (np.abs(hi - exact) <= old)
            assert ok[live & (n <= 16.5)].all(), tight.case_id(case)
    assert small > 0 and large > 0


# fault -> (before: the first OLD check that fails and its first case -- what the tests caught as they stood --,
#           after: the first NEW check that fails and its first case)
CAUGHT_BY = {
    "missing_half_reads_block_0": (None, ("specials", "bsr16,p16,specials,4,4,4,False")),
    "missing_half_reads_next_block_row": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "last_odd_block_dropped": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "blocks_past_first_round_dropped": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "wave_partial_lost": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "wave_partial_added_twice": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "reduce_through_bf16": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "regroup_even_odd_swapped": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "regroup_k_rows_swapped": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "a_k_slots_reversed": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "b32_second_half_takes_first_a": (("old_bound", "bsr32,old:bsr_mfma_bf16_b32<T4,c32>,full,4,4,12,False"), ("tight", "bsr32,p32,tight,4,4,4,False")),
    "row_4r_plus_g": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "ncol_without_interleave": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "lane_past_n_not_dropped": (None, None),
    "padding_reads_column_0": (None, ("specials", "bsrc,c16,specials,8,8,8,False")),
    "padding_reads_column_k_minus_1": (None, ("specials", "bsrc,c16,specials,8,8,8,False")),
    "unoccupied_column_kept": (None, ("specials", "bsrc,c16,specials,8,8,8,False")),
    "unused_slot_runs_previous_row": (("old_bound", "slots,old:bsrc_slots_mfma_bf16<c32,nt,share>,full,8,8,16,False"), ("tight", "slots,c16,tight,8,8,8,False")),
    "extra_steps_start_one_late": (("old_bound", "slots,old:bsrc_slots_mfma_bf16<c32,nt>,full,8,8,16,False"), ("tight", "slots,c16,tight,8,8,8,False")),
    "extra_steps_end_one_early": (("old_bound", "slots,old:bsrc_slots_mfma_bf16<c32,nt>,full,8,8,16,False"), ("tight", "slots,c16,tight,8,8,8,False")),
    "extra_ptrs_read_without_extra_steps": (None, None),
    "shared_reduce_rows_of_wrong_wave": (("old_bound", "slots,old:bsrc_slots_mfma_bf16<c32,nt,share>,full,8,8,16,False"), ("tight", "slots,c16s,tight,8,8,8,False")),
    "empty_block_row_unwritten": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "product_rounded_to_bf16": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "b_low_mantissa_bit_cleared": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "a_low_mantissa_bit_cleared": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,4,4,4,False")),
    "bf16_c_truncated": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c16>,full,4,4,12,True"), ("tight", "bsr16,p16,tight,4,4,4,True")),
    "bf16_c_from_bf16_partial": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c16>,full,4,4,12,True"), ("tight", "bsr16,p16,tight,4,4,4,True")),
    "pack_bf2_halves_swapped": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c16>,full,4,4,12,True"), ("tight", "bsr16,p16,tight,4,4,4,True")),
    "ldc_for_ldb": (("old_bound", "bsr16,old:bsr_mfma_bf16<T4,c32>,full,4,4,12,False"), ("tight", "bsr16,p16,tight,72,80,88,False")),
}

# The faults that every check of the GPU suites as they stood lets through, on every case: the finding of this work.
OLD_CHECKS_ALONE_LET_THROUGH = ("missing_half_reads_block_0", "padding_reads_column_0", "padding_reads_column_k_minus_1",
                                "unoccupied_column_kept")


@pytest.mark.parametrize("fault", list(mut.FAULTS))
def test_every_fault_fails_a_check_and_the_first_to_catch_it_before_and_after_are_the_recorded_ones(fault):
    before, after = first_catch(fault, mut.OLD), first_catch(fault, mut.NEW)
    print(f"{fault}: before {before}, after {after}")
    assert (before, after) == CAUGHT_BY[fault], (fault, before, after)
    if fault in mut.UNSEEN:
        assert before is None and after is None
    else:
        assert after is not None, f"{fault} survives every new check on every case"
    assert (before is None and fault not in mut.UNSEEN) == (fault in OLD_CHECKS_ALONE_LET_THROUGH)


def test_the_let_through_list_is_not_empty_and_two_faults_are_unseen():
    assert len(OLD_CHECKS_ALONE_LET_THROUGH) >= 1 and set(mut.UNSEEN) == {"lane_past_n_not_dropped", "extra_ptrs_read_without_extra_steps"}
    assert [f for f, (before, after) in CAUGHT_BY.items() if after is None] == list(mut.UNSEEN)


def test_a_zero_coefficient_in_front_of_a_b_row_nobody_may_read_shows_on_special_values_only():
    """0 * b is +0 for every finite b: the four let-through faults leave every finite case as it was, bit for bit (a kept
    column moves the step boundaries, so there the rounding sums stay inside the tolerance and the exact ones bit for bit)."""
    for fault in OLD_CHECKS_ALONE_LET_THROUGH:
        for kernel in mut.family_of(fault):
            for kind in ("tight", "sharp"):
                for case in mut.new_cases(kernel, kind):
                    if kind == "tight" and fault == "unoccupied_column_kept":
                        assert tight.tight(mut.restated(case, fault), case)[0], (fault, tight.case_id(case))
                        continue
                    assert np.array_equal(mut.restated(case, fault), mut.restated(case)), (fault, tight.case_id(case))
            assert first_catch(fault, ("specials",)) is not None


def test_the_numpy_compaction_is_the_host_helpers():
    """lanes.compact / compact_slots against mispmm_bsr_compact_bf16_host / mispmm_bsr_compact_slots_bf16_host (host code: no GPU)."""
    import ctypes
    from mispmm import capi
    lib = capi.lib()
    for pattern in ("c16", "c8", "c16s"):
        bsr = tight.operands(tight.Case("slots", pattern, "tight", 8, 8, 8, False))["bsr"]
        ptrs, idxs = np.ascontiguousarray(bsr.block_row_ptrs, np.uint32), np.ascontiguousarray(bsr.block_col_idxs, np.uint32)
        data = np.ascontiguousarray(bsr.data, np.float32).reshape(-1)
        mb = bsr.num_rows // 16
        n, used = ctypes.c_uint32(0), ctypes.c_uint32(0)
        head = (mb, 16, bsr.block_col_size, bsr.num_blocks, ptrs.ctypes.data, idxs.ctypes.data, data.ctypes.data, ctypes.byref(n))
        capi.check(lib.mispmm_bsr_compact_bf16_host(*head, None, None, None))
        sp, cl, tl = np.empty(mb + 1, np.uint32), np.empty(n.value * 32, np.uint32), np.empty(n.value * 512, np.uint16)
        capi.check(lib.mispmm_bsr_compact_bf16_host(*head, sp.ctypes.data, cl.ctypes.data, tl.ctypes.data))
        want = lanes.compact(bsr)
        assert np.array_equal(sp, want[0]) and np.array_equal(cl.reshape(-1, 32), want[1] & 0xFFFFFFFF)
        assert np.array_equal((tl.astype(np.uint32) << 16).view(np.float32).reshape(-1, 16, 32), want[2].astype(np.float32))
        capi.check(lib.mispmm_bsr_compact_slots_bf16_host(*head, ctypes.byref(used), None, None, None))
        ep, cl, tl = np.empty(mb + 1, np.uint32), np.empty(n.value * 32, np.uint32), np.empty(n.value * 512, np.uint16)
        capi.check(lib.mispmm_bsr_compact_slots_bf16_host(*head, ctypes.byref(used), ep.ctypes.data, cl.ctypes.data, tl.ctypes.data))
        want = lanes.compact_slots(bsr)
        assert np.array_equal(ep, want[0]) and np.array_equal(cl.reshape(-1, 32), want[1] & 0xFFFFFFFF)
        assert np.array_equal((tl.astype(np.uint32) << 16).view(np.float32).reshape(-1, 16, 32), want[2].astype(np.float32))
