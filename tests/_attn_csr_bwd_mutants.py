"""Deliberate faults for the numpy restatement of the fused CSR attention backward (tests/_attn_csr_bwd_ref.py::backward_f32) and
the numerical checks the GPU suite applies to the kernel's output, as functions of (got, case) -- tests/test_gpu_attn_csr_bwd.py
and the CPU harness tests/test_attn_csr_bwd_mutants_cpu.py call the same code, after tests/_attn_csr_mutants.py.  A fault is a
name handed to backward_f32 as `fault=`; every name carries one sentence that cites the words of include/mispmm_attn_csr_bwd.h
it breaks.  HONEST: two variants that keep the words and differ only where the header leaves room."""
import functools

import _attn_csr_bwd_ref as bref
import _attn_csr_bwd_tight as btight
import _attn_csr_ref as ref
import _attn_csr_tight as tight

FAULTS = {
    "delta_from_the_wrong_row": "`dS[e] = scale * P[e] * (dP[e] - delta_h[r])` -- the next row's delta is read.",
    "delta_omitted": "dS: `fl(fl(P * fl(dP - delta)) * scale)` -- dS = fl(fl(P * dP) * scale).",
    "head0_lse_for_every_head": "OPERANDS: `lse [H][M] and delta [H][M] contiguous` -- every head reads head 0's lse.",
    "bias_not_permuted": "COLUMN PASS: `bias[perm[t]]` -- bias[t], A^T's entry number used in A's order.",
    "head0_bias_for_every_head": "OPERANDS: `a shared bias (bias_head_stride 0)` is the only one shared -- every head reads head 0's bias.",
    "last_slot_of_full_batch_dropped": "`for i = 0 .. 7 in order` -- the eighth entry of every full batch contributes nothing.",
    "dead_slot_counts_one": "`A slot past the end of a row or a column and a lane past D or Dv read nothing` -- the slot re-reads the first "
                            "entry's rows and counts with P = 1.",
    "scale_missing_from_ds": "dS: `fl(fl(P * fl(dP - delta)) * scale)` -- the last product is left out.",
    "dk_from_k": "COLUMN PASS: `dK = fma(dS_i, Q[r_i], dK)` -- the key's own row of K is accumulated.",
    "accumulator_carried_over": "`every accumulator starts from +0` -- a row starts from the result of the row before it.",
}
HONEST = {
    "exp_float64": "the exponentials taken in float64 and rounded once to fp32 (inside the header's (3 |t| + 2) u of v_exp_f32).",
    "sums_in_another_order": "the entries of a row or column accumulated from the last to the first: an order of fp32 sums, g_L.",
}
assert set(FAULTS) == set(bref.FAULTS) and set(HONEST) == set(bref.HONEST)

# Faults no output of SOME case can expose, and why; each is still caught on another case.
EQUIVALENT_WHERE = {
    "head0_lse_for_every_head": "with one head there is no other lse to read.",
    "bias_not_permuted": "without a bias nothing is read through perm.",
    "head0_bias_for_every_head": "with one head, no bias or a shared bias there is no other bias to read.",
    "scale_missing_from_ds": "with scale = 1 (D = 1) the product changes nothing.",
}


@functools.lru_cache(maxsize=None)
def expected(case):
    """((dq, dk, dv), (tolerances)) of a case in float64; read-only."""
    op, csr = bref.operands(case), bref.matrix(case.name)
    args = (csr, op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"])
    return bref.backward_f64(*args), bref.bwd_tolerances(*args)


def bwd_composed(got, case):
    """dq, dk, dv against float64 inside bwd_tolerances: (ok, worst |err| / tolerance per output)."""
    want, tols = expected(case)
    res = [tight._worst(got[n], w, t) for n, w, t in zip(("dq", "dk", "dv"), want, tols)]
    return all(ok for ok, _ in res), tuple(worst for _, worst in res)


CHECKS = {"bwd_tolerances": bwd_composed, "tight_backward": btight.tight_backward}


@functools.lru_cache(maxsize=None)
def forward_restated(case):
    op, csr = bref.operands(case), bref.matrix(case.name)
    return ref.fused_f32(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"])


@functools.lru_cache(maxsize=8)
def restated(case, fault=None):
    """The restated backward on the restated forward's out and lse: dict(out, lse, dq, dk, dv)."""
    op, csr = bref.operands(case), bref.matrix(case.name)
    out, lse = forward_restated(case)
    dq, dk, dv = bref.backward_f32(csr, op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"], out, lse, fault)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)
