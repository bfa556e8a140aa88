"""Mutation check of the fused CSR attention tests, on a machine WITHOUT a GPU.  Every fault of tests/_attn_csr_mutants.py is put
into the numpy restatement of the kernel and the faulty output is run through the check functions the GPU suite applies to the
kernel's output (_attn_csr_mutants.CHECKS: the composed out tolerance, the lse bound, the derived tight check; _attn_csr_tight:
the tie rows), on the suite's own operands.

Held here: the restatement and two honest variants pass every check; every fault fails a check; which check and case catches each
first is the table CAUGHT_BY; which faults the composed out tolerance ALONE lets through on every case is OUT_ALONE_LETS_THROUGH;
the tie rows catch, without any tolerance, the faults that move an exact answer."""
import re

import numpy as np
import pytest

import _attn_csr_mutants as mut
import _attn_csr_ref as ref
import _attn_csr_tight as tight

# the suite's cases at three of its seven widths -- 16-byte lanes either way round and element lanes: every pattern, bias kind and head count, and
# every path of the restatement (tests/test_attn_csr_cpu.py holds the unmutated restatement on all of them)
HONEST_CASES = tuple(c for c in ref.CASES if (c.d, c.dv) in ((8, 64), (3, 5), (40, 72)))


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
    assert len(mut.FAULTS) >= 8
    for name, sentence in {**mut.FAULTS, **mut.HONEST}.items():
        assert name in mut.HONEST or ("`" in sentence and " -- " in sentence), name
    assert set(CAUGHT_BY) == set(mut.FAULTS) and set(mut.EQUIVALENT_WHERE) <= set(mut.FAULTS)
    with open(mut.__file__.replace("tests/_attn_csr_mutants.py", "include/mispmm_attn_csr.h"), encoding="utf-8") as f:
        header = " ".join(re.sub(r"^ \* ?", "", f.read(), flags=re.M).split())
    for name, sentence in mut.FAULTS.items():
        quoted = sentence.split("`")[1].split(" ... ")
        assert all(" ".join(part.split()) in header for part in quoted), f"{name}: the header does not say `{sentence.split('`')[1]}`"
    with pytest.raises(ValueError, match="unknown fault"):
        ref.fused_f32(tight.tie_pattern(1)[0], **{k: v for k, v in tight.tie_operands(1, True).items()}, fault="no_such_fault")


@pytest.mark.parametrize("variant", list(mut.HONEST))
def test_the_honest_variants_pass_every_check(variant):
    assert first_catch(variant, cases=HONEST_CASES) is None
    worst = max(mut.tight_forward(mut.restated(case, variant), case)[1] for case in HONEST_CASES)
    print(f"{variant}: worst |err| / tight tolerance {worst:.3g}")
    assert worst <= 1.0


# fault -> (the first check, in the suite's order, that fails, its first case)
CAUGHT_BY = {
    "max_never_updated": ("out_composed", "edges,D8,Dv64,finite,H1"),
    "rescale_skips_divisor": ("out_composed", "edges,D8,Dv64,none,H1"),
    "rescale_skips_o": ("out_composed", "edges,D8,Dv64,none,H1"),
    "last_slot_of_full_batch_dropped": ("out_composed", "edges,D8,Dv64,none,H1"),
    "dead_slot_counts_one": ("out_composed", "edges,D8,Dv64,none,H1"),
    "bias_before_scale": ("out_composed", "edges,D8,Dv64,finite,H1"),
    "head0_bias_for_every_head": ("out_composed", "edges,D8,Dv64,finite,H3"),
    "v_from_previous_keys": ("out_composed", "edges,D8,Dv64,none,H1"),
    "lse_from_max_alone": ("lse_bound", "edges,D8,Dv64,none,H1"),
    "weights_against_old_max": ("out_composed", "edges,D8,Dv64,none,H1"),
}
# The faults the composed out tolerance alone lets through on EVERY case: out does not read lse.  All ten are coarse faults of
# the algorithm's structure; none hides in the slack between the composed tolerance and the tight check, which is held for the
# faults of arithmetic (a truncated weight, a rescale factor of other bits) that tests/_attn_mutants.py met on the block kernel.
OUT_ALONE_LETS_THROUGH = ("lse_from_max_alone",)


@pytest.mark.parametrize("fault", list(mut.FAULTS))
def test_every_fault_fails_a_check_and_the_first_to_catch_it_is_the_recorded_one(fault):
    caught = first_catch(fault)
    print(f"{fault}: {caught}")
    assert caught is not None, f"{fault} survives every check on every case"
    assert caught == CAUGHT_BY[fault], (fault, caught)
    # the tight check catches it too, on that case or a later one: it is no looser than what it stands beside
    assert first_catch(fault, only=("tight_forward",)) is not None
    if fault not in OUT_ALONE_LETS_THROUGH:
        assert CAUGHT_BY[fault][0] == "out_composed"


@pytest.mark.parametrize("fault", OUT_ALONE_LETS_THROUGH)
def test_what_the_composed_out_tolerance_alone_lets_through(fault):
    assert first_catch(fault, only=("out_composed",)) is None
    assert first_catch(fault, only=("lse_bound",)) is not None


def test_faults_that_are_the_identity_somewhere_are_the_identity_there():
    same = lambda a, b: all(np.array_equal(a[n], b[n], equal_nan=True) for n in ("out", "lse"))   # noqa: E731
    for fault, case in (("bias_before_scale", ref.Case("edges", 8, 64, "none", 1)), ("bias_before_scale", ref.Case("edges", 1, 1, "finite", 1)),
                        ("head0_bias_for_every_head", ref.Case("edges", 8, 64, "masked", 3)),
                        ("head0_bias_for_every_head", ref.Case("edges", 8, 64, "finite", 1))):
        assert same(mut.restated(case, fault), mut.restated(case)), (fault, case.id)
    case = ref.Case("edges", 8, 64, "none", 1)
    assert np.array_equal(mut.restated(case, "lse_from_max_alone")["out"], mut.restated(case)["out"])
    assert mut.out_composed(mut.restated(case, "max_never_updated"), case)[0]          # nothing overflows without the +-200 rows


# ---- tie rows: exact answers, no tolerance
@pytest.mark.parametrize("through_bias", [False, True])
@pytest.mark.parametrize("t", tight.TIES)
def test_tie_rows_the_restatement_has_the_exact_answers_bit_for_bit(t, through_bias):
    seen = tight.tie_coverage(t)
    assert seen["slots"] == set(range(8)) and seen["first_batch"] and seen["last_batch"] and seen["partial_last"], seen
    csr = tight.tie_pattern(t)[0]
    op = tight.tie_operands(t, through_bias)
    assert op["bias"] is None or np.isfinite(op["bias"]).all()
    out, lse = ref.fused_f32(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"])
    assert tight.tie_check(dict(out=out, lse=lse), t, through_bias) == (True, 0)


def test_tie_rows_catch_faults_without_any_tolerance():
    """Not every fault moves an exact answer (the bias faults need a bias that differs by head or a scale other than 1; a maximum
    that is never raised subtracts 0, which is these rows' maximum); the others do, bit for bit."""
    silent = {"bias_before_scale", "head0_bias_for_every_head", "max_never_updated"}
    for through_bias in (False, True):
        csr = tight.tie_pattern(4)[0]
        op = tight.tie_operands(4, through_bias)
        for fault in mut.FAULTS:
            with np.errstate(all="ignore"):
                out, lse = ref.fused_f32(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"], fault)
            caught = not tight.tie_check(dict(out=out, lse=lse), 4, through_bias)[0]
            print(f"tie rows t=4 through_bias={through_bias} {fault}: {'caught' if caught else 'not seen'}")
            assert caught or fault in silent, fault
