"""Deliberate faults for the numpy restatement of the fused CSR attention kernel (tests/_attn_csr_ref.py::fused_f32) and the
numerical checks the GPU suite applies to the kernel's output, as functions of (got, case) -- tests/test_gpu_attn_csr.py and the
CPU harness tests/test_attn_csr_mutants_cpu.py call the same code.  A fault is a name handed to fused_f32 as `fault=`; every name
carries one sentence that cites the words of include/mispmm_attn_csr.h it breaks: a kernel that made the same mistake would
break the contract in the same way.  HONEST: two variants that keep the words and differ only where the header leaves room."""
import functools

import numpy as np

import _attn_csr_ref as ref
import _attn_csr_tight as tight
from _softmax_ref import matrix

FAULTS = {
    "max_never_updated": "ALGORITHM maximum: `m = max(m, mb)` -- m stays -Inf, so mu stays 0 and nothing is ever subtracted.",
    "rescale_skips_divisor": "ALGORITHM divisor: `l = fl(fl(l * alpha) + t)` -- l = fl(l + t): the rescale reaches O but not l.",
    "rescale_skips_o": "ALGORITHM product: `O = fl(alpha * O)` -- the rescale reaches l but not O.",
    "last_slot_of_full_batch_dropped": "out: `sum_e` over every stored entry -- the eighth entry of every full batch gets the weight 0.",
    "dead_slot_counts_one": "ALGORITHM divisor: `a slot past the row end: +0` -- it counts exp(0) = 1 in t.",
    "bias_before_scale": "z: `fma(scale, s[e], bias_h[e])` -- z = scale * (s + bias).",
    "head0_bias_for_every_head": "OPERANDS: `bias: [H][nnz] ... with head stride bias_head_stride` -- every head reads head 0's bias.",
    "v_from_previous_keys": "product: `O = fma(w_i, V[c_i], O)` with the batch's own columns -- V is gathered with the previous batch's keys.",
    "lse_from_max_alone": "lse: `mu + logf(l)` -- mu alone.",
    "weights_against_old_max": "ALGORITHM weights: `with the batch's NEW mu` -- w = exp(z - mu_old).",
}
HONEST = {
    "exp_float64": "the exponentials taken in float64 and rounded once to fp32 (v_exp_f32 and np.exp2 are both within the header's "
                   "(3 t + 2) u of this one).",
    "sums_in_another_order": "the 8 weights of a batch summed one after the other from the last, and the 8 fmas into O taken from the last: "
                             "orders of fp32 sums, which the tight check allows as g_n.",
}
assert set(FAULTS) == set(ref.FAULTS) and set(HONEST) == set(ref.HONEST)

# Faults no output of SOME case can expose, and why; each is still caught on another case.
EQUIVALENT_WHERE = {
    "max_never_updated": "where no score reaches the overflow of exp every mu gives the same softmax in real arithmetic; the rows whose bias "
                         "carries +200 overflow outright.",
    "bias_before_scale": "without a bias, or with scale = 1 (D = 1), the two forms are the same number.",
    "head0_bias_for_every_head": "with one head, no bias or a shared bias there is no other bias to read.",
    "lse_from_max_alone": "out does not read lse: only the lse bound and the tight check see it.",
}


@functools.lru_cache(maxsize=None)
def expected(case):
    """(out, lse, out tolerance, lse tolerance) of a case in float64; read-only."""
    op, csr = ref.operands(case), matrix(case.name)
    out, lse = ref.attention_f64(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"])
    return (out, lse, ref.out_tolerance(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"]),
            ref.lse_tolerance(csr, op["q"], op["k"], op["scale"], op["bias"]))


def out_composed(got, case):
    """out against float64 inside the composed tolerance of the four-launch chain: (ok, worst |err| / tolerance)."""
    want, _, tol, _ = expected(case)
    with np.errstate(invalid="ignore"):
        err = np.abs(got["out"].astype(np.float64) - want)
        return bool(np.all(err <= tol)), float(np.max(np.where(np.isnan(err), np.inf, err / tol)))


def lse_bound(got, case):
    """lse against float64 inside the header's bound; -Inf exactly on the rows without entries."""
    _, want, _, tol = expected(case)
    stored = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got["lse"][stored].astype(np.float64) - want[stored])
        ok = bool(np.all(err <= tol[stored])) and bool(np.array_equal(np.isneginf(got["lse"]), ~stored))
        return ok, float(np.max(np.where(np.isnan(err), np.inf, err / tol[stored]), initial=0.0))


def tight_forward(got, case):
    ok, worst = tight.tight_forward(got, case)
    return ok, max(worst)


CHECKS = {"out_composed": out_composed, "lse_bound": lse_bound, "tight_forward": tight_forward}


@functools.lru_cache(maxsize=8)
def restated(case, fault=None):
    op, csr = ref.operands(case), matrix(case.name)
    out, lse = ref.fused_f32(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"], fault)
    return dict(out=out, lse=lse)
