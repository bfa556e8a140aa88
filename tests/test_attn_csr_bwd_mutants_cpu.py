"""Mutation check of the fused CSR attention backward tests, on a machine WITHOUT a GPU.  Every fault of
tests/_attn_csr_bwd_mutants.py is put into the numpy restatement of both passes and the faulty gradients are run through the
check functions the GPU suite applies to the kernel's output (_attn_csr_bwd_mutants.CHECKS: the derived tolerances around
float64, the derived tight check around the forward's own out and lse), on the suite's own operands.

Held here: the restatement and two honest variants pass every check; every fault fails both checks; which check and case
catches each first is the table CAUGHT_BY; a fault that is the identity on some case is the identity there."""
import re

import numpy as np
import pytest

import _attn_csr_bwd_mutants as mut
import _attn_csr_bwd_ref as bref

# the suite's cases at three of its seven widths -- 16-byte lanes either way round and element lanes: every pattern, bias kind and
# head count (tests/test_attn_csr_bwd_cpu.py holds the unmutated restatement on all of them)
HONEST_CASES = tuple(c for c in bref.CASES if (c.d, c.dv) in ((8, 64), (3, 5), (40, 72)))


def first_catch(fault, only=None, cases=HONEST_CASES):
    """(check, case id) of the first check, in the suite's order, that the faulty restatement fails, and its first case; None:
    it survives."""
    with np.errstate(all="ignore"):
        for name, check in mut.CHECKS.items():
            if only is not None and name not in only:
                continue
            for case in cases:
                if not check(mut.restated(case, fault), case)[0]:
                    return name, case.id
    return None


def test_the_catalogue_names_the_header_words_every_fault_breaks():
    assert len(mut.FAULTS) >= 10
    assert set(CAUGHT_BY) == set(mut.FAULTS) and set(mut.EQUIVALENT_WHERE) <= set(mut.FAULTS)
    with open(mut.__file__.replace("tests/_attn_csr_bwd_mutants.py", "include/mispmm_attn_csr_bwd.h"), encoding="utf-8") as f:
        header = " ".join(re.sub(r"^ \* ?", "", f.read(), flags=re.M).split())
    for name, sentence in mut.FAULTS.items():
        assert "`" in sentence and " -- " in sentence, name
        quoted = sentence.split("`")[1]
        assert " ".join(quoted.split()) in header, f"{name}: the header does not say `{quoted}`"
    case = HONEST_CASES[0]
    with pytest.raises(ValueError, match="unknown fault"):
        mut.restated(case, "no_such_fault")


@pytest.mark.parametrize("variant", list(mut.HONEST))
def test_the_honest_variants_pass_every_check(variant):
    assert first_catch(variant) is None
    worst = max(max(mut.CHECKS["tight_backward"](mut.restated(case, variant), case)[1]) for case in HONEST_CASES)
    print(f"{variant}: worst |err| / tight tolerance {worst:.3g}")
    assert worst <= 1.0


# fault -> (the first check, in the suite's order, that fails, its first case)
CAUGHT_BY = {
    "delta_from_the_wrong_row": ("bwd_tolerances", "edges,D8,Dv64,none,H1"),
    "delta_omitted": ("bwd_tolerances", "edges,D8,Dv64,none,H1"),
    "head0_lse_for_every_head": ("bwd_tolerances", "edges,D8,Dv64,none,H3"),
    "bias_not_permuted": ("bwd_tolerances", "edges,D8,Dv64,finite,H1"),
    "head0_bias_for_every_head": ("bwd_tolerances", "edges,D8,Dv64,finite,H3"),
    "last_slot_of_full_batch_dropped": ("bwd_tolerances", "edges,D8,Dv64,none,H1"),
    "dead_slot_counts_one": ("bwd_tolerances", "edges,D8,Dv64,none,H1"),
    "scale_missing_from_ds": ("bwd_tolerances", "edges,D8,Dv64,none,H1"),
    "dk_from_k": ("bwd_tolerances", "edges,D8,Dv64,none,H1"),
    "accumulator_carried_over": ("bwd_tolerances", "edges,D8,Dv64,none,H1"),
}


@pytest.mark.parametrize("fault", list(mut.FAULTS))
def test_every_fault_fails_a_check_and_the_first_to_catch_it_is_the_recorded_one(fault):
    caught = first_catch(fault)
    print(f"{fault}: {caught}")
    assert caught is not None, f"{fault} survives every check on every case"
    assert caught == CAUGHT_BY[fault], (fault, caught)
    # the tight check catches it too, and on the same case: it is no looser than what it stands beside
    assert first_catch(fault, only=("tight_backward",)) == ("tight_backward", CAUGHT_BY[fault][1])


def test_faults_that_are_the_identity_somewhere_are_the_identity_there():
    same = lambda a, b: all(np.array_equal(a[n], b[n], equal_nan=True) for n in ("dq", "dk", "dv"))   # noqa: E731
    for fault, case in (("head0_lse_for_every_head", bref.Case("edges", 8, 64, "masked", 1)), ("bias_not_permuted", bref.Case("edgesT", 8, 64, "none", 3)),
                        ("head0_bias_for_every_head", bref.Case("edges", 8, 64, "masked", 3)), ("head0_bias_for_every_head", bref.Case("ragged", 3, 5, "finite", 1)),
                        ("scale_missing_from_ds", bref.Case("edges", 1, 1, "finite", 1))):
        assert same(mut.restated(case, fault), mut.restated(case)), (fault, case.id)
    # a fault of one pass leaves the other pass's outputs alone
    case = bref.Case("edges", 8, 64, "finite", 1)
    for fault, kept in (("bias_not_permuted", ("dq",)), ("dk_from_k", ("dq", "dv")), ("delta_omitted", ("dv",)), ("scale_missing_from_ds", ("dv",))):
        for n in kept:
            assert np.array_equal(mut.restated(case, fault)[n], mut.restated(case)[n]), (fault, n)
