"""Deliberate faults for the numpy restatements of the two fused attention kernels (tests/_attn_fused_ref.py::fused_f32,
tests/_attn_fused_bwd_ref.py::forward_f32 / delta_f32 / _weights / backward_f32).  A fault is a name handed to those functions as
`fault=`; with fault=None they keep their bits.  Every name carries one sentence that cites the words of include/mispmm_attn.h
(H) or include/mispmm_attn_bwd.h (B) it breaks: a kernel that made the same mistake would break the contract in the same way, and
tests/test_attn_mutants_cpu.py shows which check of the GPU suite would notice.

HONEST lists two variants that keep the contract and differ from the restatement only where the contract leaves room; the
tight check of tests/_attn_tight.py has to hold both."""

FORWARD = {
    "w_truncated": "H ALGORITHM: `the weights enter the second MFMA as bf16, rounded once to nearest even` -- truncated towards zero instead.",
    "divisor_unrounded": "H ALGORITHM: `the divisor l is the sum of the ROUNDED weights` -- l is summed from the fp32 weights.",
    "scale_bf16": "H z: `fl32(scale * s + mask)` with the fp32 scale -- scale is rounded to bf16 before use.",
    "stale_max": "H ALGORITHM: `a running maximum m, the weights w = exp(z - mu) with mu = m` -- m keeps the first step's value.",
    "s_bf16": "H s: `fp32 accumulation: the bits of mispmm_sddmm_bsr_bf16` -- S is rounded to bf16 before it is scaled.",
    "acc_bf16": "H ALGORITHM: `online softmax in fp32 ... the accumulator O` -- O is rounded to bf16 after every step.",
    "last_key_dropped": "H out: `sum_e sum_j` over every stored key -- the last live key of a row's last step gets the weight 0.",
    "lse_from_rounded": "H ALGORITHM: `lse comes from a second fp32 sum lx of the UNROUNDED weights` -- lse is taken from l.",
    "rescale_skips_divisor": "H ALGORITHM: `running sums and the accumulator O multiplied by exp(mu_old - mu_new) after every step` "
                             "-- on the second step l is not.",
}

BACKWARD = {
    "ds_truncated": "B dS: `then rounded ONCE to bf16 (nearest even)` -- truncated towards zero instead.",
    "delta_scaled": "B delta: `sum_c dO[r,c] * O[r,c]` -- multiplied by 1 + 2^-9.",
    "p_bf16_before_ds": "B dS: `fl(fl(P * fl(dP - delta[r])) * scale)` with the fp32 P -- P is rounded to bf16 before it enters dS.",
    "delta_from_bf16_out": "B delta: `O = the forward's out as stored (fp32 or bf16 bits)` -- an fp32 out is rounded to bf16 first.",
    "p_truncated": "B dV: `bf16(P[r,key])`, nearest even as everywhere -- truncated towards zero instead.",
    "lse_shifted": "B P: `exp(z[r,key] - lse[r])` -- lse is read 2^-9 too large.",
    "bwd_scale_bf16": "B dS and z: the fp32 `scale`, `exactly as mispmm_attn.h defines it` -- scale is rounded to bf16 before use.",
    "mask_transposed_cols": "B PATTERNS: `block t of A^T is block perm[t] of A` in A's element order -- the column pass reads the mask block "
                            "transposed.",
    "last_query_dropped": "B dK, dV: `sum over the rows that store key` -- the last query of a block column's last step contributes nothing.",
    "grad_out_unrounded": "B OPERANDS: `dO ... raw bf16 bits` -- a float32 grad_out enters the passes with all its 24 bits.",
    "dq_acc_carried": "B ALGORITHM: `dQ^T += K^T dS^T by MFMA, fp32 accumulators from +0` -- a block row starts from the one before it.",
}

HONEST = {
    "exp_float64": "the exponentials taken in float64 and rounded once to fp32 (v_exp_f32 and np.exp2 are both within the header's "
                   "(3 t + 2) u of this one).",
    "mfma_fp32_sequential": "the sums inside the second products' MFMAs taken in fp32, term after term (the header fixes no order inside "
                            "the instruction).",
}

# the eight the old checks let through, as measured on the CPU before the tight check existed
OLD_SURVIVORS = ("w_truncated", "divisor_unrounded", "scale_bf16", "stale_max",
                 "ds_truncated", "delta_scaled", "p_bf16_before_ds", "delta_from_bf16_out")

# Faults no output of SOME case can expose, and why; each is still caught on another case.
EQUIVALENT_WHERE = {
    "stale_max": "where no score spread reaches the overflow of exp every mu gives the same softmax in real arithmetic; only the "
                 "roundings of the weights move, and the wide-score case overflows outright.",
    "delta_from_bf16_out": "with a bf16 out the stored out is already rounded: the fault is the identity there.",
    "grad_out_unrounded": "a grad_out that holds bf16 numbers is its own rounding: only a float32 grad_out with low bits shows it.",
    "mask_transposed_cols": "without a mask, or with one whose blocks are symmetric (`leading`: whole blocks), nothing is read differently.",
    "rescale_skips_divisor": "a row of one step, or one whose maximum sits in its first step, has a factor of exactly 1 there.",
    "dq_acc_carried": "the first non-empty block row has nothing before it.",
}

ALL = {**FORWARD, **BACKWARD}


def check(fault, allowed):
    if fault is not None and fault not in allowed and fault not in HONEST:
        raise ValueError(f"unknown fault {fault!r}")
    return fault
