"""Mutation check of the fused attention tests, on a machine WITHOUT a GPU.  Every fault of tests/_attn_mutants.py is put into the
numpy restatements of the two kernels and the faulty output is run through every numerical check the GPU suite applies to a
kernel's output (tests/_attn_checks.py: the composed tolerances, the lse bound, the constant-V bound, the +0 bits, the
subset-of-outputs equality; tests/_attn_tight.py: the derived tight check and the tie rows) -- the same functions the GPU tests call.

Held here: the restatements keep their bits with fault=None; the unmutated restatement and two honest variants pass every check
on every case; every fault fails a check; which check and case catches each first is the table CAUGHT_BY; the eight faults the
composed tolerances let through (OLD_SURVIVORS) stay inside them on every case, with the worst ratios printed (`-s`), and fall to
the tight check; SURVIVED says which other old check, if any, holds each.
`pytest tests/test_attn_mutants_cpu.py -s -k survive` prints the figures before and after."""
import functools
import itertools
import os

import numpy as np
import pytest

pytest.importorskip("torch")

import _attn_checks as checks  # noqa: E402
import _attn_fused_bwd_ref as bwd_ref  # noqa: E402
import _attn_fused_ref as fwd_ref  # noqa: E402
import _attn_mutants as mutants  # noqa: E402
import _attn_tight as tight  # noqa: E402
from _attn_checks import Case  # noqa: E402
from _softmax_bsr_ref import bf16_round  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_restated_frozen.npz")

# ---- the cases: the suite's own operands, patterns, widths and masks
FWD_WIDTHS = [(8, 64), (40, 72), (128, 128)]
FORWARD_CASES = (
    [Case(n, d, dv, kind) for n, (d, dv), kind in itertools.product(fwd_ref.PATTERNS, FWD_WIDTHS, fwd_ref.MASKS)]
    + [Case(n, 40, 72, kind, out_bf16=True) for n, kind in itertools.product(fwd_ref.PATTERNS, fwd_ref.MASKS)]
    + [Case(n, 64, 64, "causal", const_v=value) for n, value in itertools.product(("edges16", "edges32"), (1.0, -0.34765625))]
    # scores spread far past the overflow of exp: |z| up to several hundred
    + [Case("ragged16", 64, 64, "none", wide=16, scale=1.0), Case("edges32", 64, 64, "leading", wide=16, scale=1.0)])
BWD_WIDTHS = [(8, 64), (40, 72)]
BACKWARD_CASES = (
    [Case(n, d, dv, kind, src="bwd") for n, (d, dv), kind in itertools.product(bwd_ref.PATTERNS, BWD_WIDTHS, bwd_ref.MASKS)]
    + [Case(n, 40, 72, "causal", src="bwd", out_bf16=True, grads_bf16=True) for n in bwd_ref.PATTERNS]
    + [Case(n, 40, 72, "causal", src="bwd", grads_bf16=True, g32=True) for n in ("edges16", "edgesT32")]
    + [Case(n, 40, 72, "blankcols", src="bwd") for n in ("ragged16", "edgesT32")])

FORWARD_CHECKS = {**checks.OLD_FORWARD, "tight_forward": tight.tight_forward}
BACKWARD_CHECKS = {**checks.OLD_BACKWARD, "tight_backward": tight.tight_backward}


@functools.lru_cache(maxsize=None)
def forward_got(case, fault):
    q, k, v, _ = case.arrays
    out, lse = bwd_ref.forward_f32(case.name, q, k, v, case.mask, case.scale_value, fault)
    return dict(out=bf16_round(out) if case.out_bf16 else out, lse=lse)


@functools.lru_cache(maxsize=None)
def backward_got(case, fault):
    """The backward restated on the UNMUTATED restated forward's out and lse."""
    q, k, v, g = case.arrays
    fwd = forward_got(Case(case.name, case.d, case.dv, case.kind, src="bwd", out_bf16=case.out_bf16), None)
    dq, dk, dv = bwd_ref.backward_f32(case.name, q, k, v, g, fwd["out"], fwd["lse"], case.mask, case.scale_value, case.grads_bf16, fault)
    got = dict(out=fwd["out"], lse=fwd["lse"], dq=dq, dk=dk, dv=dv)
    # the restatement has no `need`: a subset is the same pass run alone, so its bits are those of the call for all three
    got["subsets"] = {need: tuple(x if n else None for x, n in zip((dq, dk, dv), need)) for need in itertools.product((False, True), repeat=3)}
    return got


def sides(fault):
    if fault in mutants.FORWARD:
        return ((FORWARD_CASES, FORWARD_CHECKS, forward_got),)
    if fault in mutants.BACKWARD:
        return ((BACKWARD_CASES, BACKWARD_CHECKS, backward_got),)
    return ((FORWARD_CASES, FORWARD_CHECKS, forward_got), (BACKWARD_CASES, BACKWARD_CHECKS, backward_got))


def first_catch(fault, only=None, wide=True):
    """(check, case id) of the first check, in the suite's order, that the faulty restatement fails, and its first case; None: it
    survives.  only: the names of the checks to run."""
    with np.errstate(all="ignore"):
        for cases, table, got_of in sides(fault):
            for name, check in table.items():
                if only is not None and name not in only:
                    continue
                for case in cases:
                    if case.wide != 1 and not wide:
                        continue
                    res = check(got_of(case, fault), case)
                    if res is not None and not res[0]:
                        return name, case.id
    return None


def worst_ratios(fault, names, wide=True):
    """{check: the worst figure over all cases} for the named checks."""
    worst = {}
    with np.errstate(all="ignore"):
        for cases, table, got_of in sides(fault):
            for name in names:
                for case in cases if name in table else ():
                    if case.wide != 1 and not wide:
                        continue
                    res = table[name](got_of(case, fault), case)
                    if res is not None:
                        figure = np.max(res[1]) if name != "tight_forward" and name != "tight_backward" else np.max(res[1][:-1 if name == "tight_forward" else -2])
                        worst[name] = max(worst.get(name, 0.0), float(figure))
    return worst


# ---- fault=None keeps today's bits
@pytest.mark.parametrize("name", ["ragged16", "ragged32"])
def test_without_a_fault_the_restatements_keep_their_bits(name):
    """Against outputs frozen before the hooks went in (tests/golden/attn_restated_frozen.npz): D = 40, Dv = 72, the causal mask."""
    frozen = np.load(GOLDEN)
    # the restatements call np.exp2 and np.log in float32: their last bit is the C library's and numpy's build's, not this project's
    x, y = np.linspace(-60.0, 0.0, 8192).astype(np.float32), np.linspace(0.5, 3000.0, 8192).astype(np.float32)
    if not (np.array_equal(np.exp2(x), frozen["probe_exp2"]) and np.array_equal(np.log(y), frozen["probe_log"])):
        pytest.skip("np.exp2 / np.log in float32 differ here from where the outputs were frozen: their bits cannot be compared")
    d, dv = 40, 72
    q, k, v, g = (x[0] for x in bwd_ref.operands(name, d, dv))
    mask, scale = bwd_ref.mask_of(name, "causal"), d ** -0.5
    out, lse = fwd_ref.fused_f32(name, q, k, v, mask, scale)
    again = bwd_ref.forward_f32(name, q, k, v, mask, scale, fault=None)
    delta = bwd_ref.delta_f32(g, out)
    dq, dk, dvv = bwd_ref.backward_f32(name, q, k, v, g, out, lse, mask, scale, False)
    for what, x in (("out", out), ("lse", lse), ("delta", delta), ("dq", dq), ("dk", dk), ("dv", dvv)):
        assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), frozen[f"{name}_{what}"].view(np.uint32)), what
    assert np.array_equal(again[0].view(np.uint32), out.view(np.uint32)) and np.array_equal(again[1].view(np.uint32), lse.view(np.uint32))
    with pytest.raises(ValueError, match="unknown fault"):
        fwd_ref.fused_f32(name, q, k, v, mask, scale, fault="no_such_fault")
    with pytest.raises(ValueError, match="unknown fault"):
        bwd_ref.backward_f32(name, q, k, v, g, out, lse, mask, scale, False, fault="w_truncated")     # a forward fault


def test_the_catalogue_names_the_header_words_every_fault_breaks():
    assert len(mutants.FORWARD) >= 9 and len(mutants.BACKWARD) >= 11 and not set(mutants.FORWARD) & set(mutants.BACKWARD)
    for name, sentence in mutants.ALL.items():
        assert sentence.startswith(("H ", "B ")) and "`" in sentence and " -- " in sentence, name
    assert set(mutants.OLD_SURVIVORS) <= set(mutants.ALL) and set(mutants.EQUIVALENT_WHERE) <= set(mutants.ALL)
    assert set(CAUGHT_BY) == set(mutants.ALL)


# ---- the unmutated restatement and the honest variants pass everything
@pytest.mark.parametrize("variant", [None] + list(mutants.HONEST))
def test_the_restatement_and_its_honest_variants_pass_every_check_on_every_case(variant):
    assert first_catch(variant) is None
    tightest = worst_ratios(variant, ("tight_forward", "tight_backward"))
    print(f"{variant or 'the restatement'}: worst |err| / tight tolerance: forward {tightest['tight_forward']:.3g}, backward {tightest['tight_backward']:.3g}")
    assert tightest["tight_forward"] <= 1.0 and tightest["tight_backward"] <= 1.0


def test_every_case_has_exact_products_and_few_flagged_elements():
    worst = 0.0
    for case in FORWARD_CASES:
        res = tight.tight_forward(forward_got(case, None), case)
        assert (res is None) == bool(case.const_v or case.wide != 1), case.id
        if res is not None:
            assert tight.exact_products(case)
            worst = max(worst, res[1][2])
    for case in BACKWARD_CASES:
        res = tight.tight_backward(backward_got(case, None), case)
        if res is not None:
            assert tight.exact_products(case)
            worst = max(worst, res[1][3], res[1][4])
    print(f"worst flagged share of the live elements: {worst:.3%}")
    assert 0.0 < worst <= tight.FLAGGED_CAP
    assert not tight.exact_products(FORWARD_CASES[-1])                 # the wide-score case: S rounds, the tight check stands aside


# ---- every fault is caught; by what, first
# fault -> (the first check, in the suite's order -- the old ones before the tight one -- that fails, its first case).  An entry
# that names tight_forward / tight_backward is a fault NO old check catches on any case.
CAUGHT_BY = {
    "w_truncated": ("tight_forward", "fwd:ragged16,D8,Dv64,none"),
    "divisor_unrounded": ("constant_v", "fwd:edges16,D64,Dv64,causal,v=1.0"),
    "scale_bf16": ("lse_bound", "fwd:ragged16,D8,Dv64,none"),
    "stale_max": ("out_composed", "fwd:ragged16,D64,Dv64,none,wide16,scale=1.0"),
    "s_bf16": ("out_composed", "fwd:ragged16,D8,Dv64,none"),
    "acc_bf16": ("out_composed", "fwd:ragged16,D8,Dv64,none"),
    "last_key_dropped": ("out_composed", "fwd:ragged16,D8,Dv64,none"),
    "lse_from_rounded": ("lse_bound", "fwd:ragged16,D8,Dv64,none"),
    "rescale_skips_divisor": ("out_composed", "fwd:ragged16,D8,Dv64,none"),
    "ds_truncated": ("tight_backward", "bwd:ragged16,D8,Dv64,none"),
    "delta_scaled": ("tight_backward", "bwd:ragged16,D8,Dv64,none"),
    "p_bf16_before_ds": ("tight_backward", "bwd:ragged16,D8,Dv64,none"),
    "delta_from_bf16_out": ("tight_backward", "bwd:ragged16,D8,Dv64,none"),
    "p_truncated": ("bwd_composed", "bwd:ragged16,D8,Dv64,none"),
    "lse_shifted": ("bwd_composed", "bwd:ragged16,D8,Dv64,leading"),
    "bwd_scale_bf16": ("bwd_composed", "bwd:ragged16,D40,Dv72,causal"),
    "mask_transposed_cols": ("bwd_composed", "bwd:ragged16,D8,Dv64,causal"),
    "last_query_dropped": ("bwd_composed", "bwd:ragged16,D8,Dv64,none"),
    "grad_out_unrounded": ("tight_backward", "bwd:edges16,D40,Dv72,causal,gbf16,g32"),
    "dq_acc_carried": ("bwd_composed", "bwd:ragged16,D8,Dv64,none"),
}
# The composed tolerance each of the eight survivors was measured against, and the OTHER old check that does catch it, if one does:
# the constant-V bound holds the divisor, the lse bound a rounded scale, and only the wide-score cases added with this file a stale
# maximum.  The other five fall to the tight check alone.
SURVIVED = {"w_truncated": ("out_composed", None), "divisor_unrounded": ("out_composed", "constant_v"), "scale_bf16": ("out_composed", "lse_bound"),
            "stale_max": ("out_composed", "out_composed"), "ds_truncated": ("bwd_composed", None), "delta_scaled": ("bwd_composed", None),
            "p_bf16_before_ds": ("bwd_composed", None), "delta_from_bf16_out": ("bwd_composed", None)}


@pytest.mark.parametrize("fault", list(mutants.ALL))
def test_every_fault_fails_a_check_and_the_first_to_catch_it_is_the_recorded_one(fault):
    caught = first_catch(fault)
    print(f"{fault}: {caught}")
    assert caught is not None, f"{fault} survives every check on every case"
    assert caught == CAUGHT_BY[fault], (fault, caught)


@pytest.mark.parametrize("fault", mutants.OLD_SURVIVORS)
def test_the_old_tolerance_lets_it_survive_and_the_tight_check_catches_it(fault):
    """What was gained: worst |err| / tolerance over the suite's cases (the wide-score ones, new with this file, aside) under the
    composed tolerance (below 1: a survivor) and under the tight check (above 1: caught)."""
    bound, other = SURVIVED[fault]
    old = worst_ratios(fault, (bound,), wide=False)[bound]
    new = max(worst_ratios(fault, ("tight_forward", "tight_backward"), wide=False).values())
    print(f"{fault}: worst |err| / tolerance: {bound} {old:.3g} (survives), tight {new:.3g} (caught); other old check that catches it: {other}")
    assert first_catch(fault, only=(bound,), wide=False) is None and old < 1.0
    assert first_catch(fault, only=("tight_forward", "tight_backward")) is not None and new > 1.0
    assert (CAUGHT_BY[fault][0] if not CAUGHT_BY[fault][0].startswith("tight") else None) == other


def test_a_stale_maximum_is_caught_by_a_wide_score_case_under_the_old_checks_too():
    """Equivalent in real arithmetic where nothing overflows (mutants.EQUIVALENT_WHERE); with |z| in the hundreds the weights
    against a stale maximum overflow and out is not even finite."""
    wide = [c for c in FORWARD_CASES if c.wide != 1]
    assert wide
    for case in wide:
        clean, faulty = forward_got(case, None), forward_got(case, "stale_max")
        assert np.isfinite(clean["out"]).all() and checks.out_composed(clean, case)[0] and checks.lse_bound(clean, case)[0]
    assert any(not checks.out_composed(forward_got(case, "stale_max"), case)[0] for case in wide)


def test_faults_that_are_the_identity_somewhere_are_the_identity_there():
    """mutants.EQUIVALENT_WHERE, case by case: the same bits as the unmutated restatement."""
    same = lambda a, b, names: all(np.array_equal(a[n], b[n], equal_nan=True) for n in names)   # noqa: E731
    grads = ("dq", "dk", "dv")
    bf = next(c for c in BACKWARD_CASES if c.out_bf16)
    assert same(backward_got(bf, "delta_from_bf16_out"), backward_got(bf, None), grads)
    plain = next(c for c in BACKWARD_CASES if not c.g32)
    assert same(backward_got(plain, "grad_out_unrounded"), backward_got(plain, None), grads)
    for kind in ("none", "leading"):
        c = Case("ragged16", 40, 72, kind, src="bwd")
        assert same(backward_got(c, "mask_transposed_cols"), backward_got(c, None), grads)
    c = Case("ragged16", 40, 72, "none")
    rows = slice(2 * 16, 3 * 16)                                       # block row 2: one block, one half step
    assert same({"o": forward_got(c, "rescale_skips_divisor")["out"][rows]}, {"o": forward_got(c, None)["out"][rows]}, ("o",))
    c = Case("ragged16", 40, 72, "none", src="bwd")
    assert np.array_equal(backward_got(c, "dq_acc_carried")["dq"][:16], backward_got(c, None)["dq"][:16])


# ---- tie rows: exact answers, no tolerance
@pytest.mark.parametrize("through_mask", [False, True])
@pytest.mark.parametrize("t", tight.TIES)
def test_tie_rows_the_restatement_has_the_exact_answers_bit_for_bit(t, through_mask):
    seen = tight.tie_coverage(bwd_ref.PATTERNS, t, through_mask)
    assert seen["positions"] == set(range(32)) and all(seen[n] for n in ("first_step", "last_step", "half_step", "first_query", "last_query")), seen
    for name in bwd_ref.PATTERNS:
        op = tight.tie_operands(name, t, through_mask)
        assert op["mask"] is None or np.isfinite(op["mask"]).all()
        out, lse = bwd_ref.forward_f32(name, op["q"], op["k"], op["v"], op["mask"], op["scale"])
        for out_bf16 in (False, True):
            stored = bf16_round(out) if out_bf16 else out
            assert tight.tie_forward(dict(out=stored, lse=lse), name, t, through_mask, out_bf16) == (True, 0), (name, out_bf16)
            for grads_bf16 in (False, True):
                dq, dk, dv = bwd_ref.backward_f32(name, op["q"], op["k"], op["v"], op["g"], stored, lse, op["mask"], op["scale"], grads_bf16)
                assert tight.tie_backward(dict(dq=dq, dk=dk, dv=dv), name, t, through_mask, grads_bf16) == (True, 0), (name, out_bf16, grads_bf16)


def test_tie_rows_catch_faults_without_any_tolerance():
    """Not every fault moves an exact answer (a truncation of a weight that is exactly 1 does nothing); these do."""
    name, t = "ragged16", 4
    for through_mask in (False, True):
        op = tight.tie_operands(name, t, through_mask)
        args = (name, op["q"], op["k"], op["v"], op["mask"], op["scale"])
        out, lse = bwd_ref.forward_f32(*args)
        for fault in ("last_key_dropped", "rescale_skips_divisor", "acc_bf16"):
            o, l = bwd_ref.forward_f32(*args, fault)
            caught = not tight.tie_forward(dict(out=o, lse=l), name, t, through_mask)[0]
            assert caught or fault == "acc_bf16", fault                # small integers survive a rounding to bf16
        for fault in ("last_query_dropped", "dq_acc_carried", "delta_scaled", "mask_transposed_cols"):
            dq, dk, dv = bwd_ref.backward_f32(name, op["q"], op["k"], op["v"], op["g"], out, lse, op["mask"], op["scale"], False, fault)
            caught = not tight.tie_backward(dict(dq=dq, dk=dk, dv=dv), name, t, through_mask)[0]
            assert caught or (fault == "mask_transposed_cols" and not through_mask), fault
