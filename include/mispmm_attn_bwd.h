/* mispmm_attn_bwd.h -- C ABI of libmispmm_attn_bwd.so: the backward of the fused block-sparse attention forward
 * (mispmm_attn.h) in bf16 for AMD CDNA4 (gfx950).
 *
 * A third library beside libmispmm.so (mispmm.h), which it links exactly as libmispmm_attn.so does: status codes,
 * mispmm_stream_t, mispmm_last_error() and mispmm_last_kernel() are that library's, and a call here leaves its message and
 * its kernel tag there.  Conventions as in mispmm.h: device pointers, row-major dense operands, a call only enqueues on
 * `stream`, and every argument is validated before any device work.
 */
#ifndef MISPMM_ATTN_BWD_H
#define MISPMM_ATTN_BWD_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Fused attention backward on a BSR pattern, bf16 */
/* dQ, dK and dV of mispmm_attn_bsr_bf16 for H heads in at most TWO launches, whatever H: neither the scores S, the weights
 * P, dP nor dS is written to memory anywhere.  For head h, matrix row r and a key the pattern stores in r's block row, with
 * z exactly as mispmm_attn.h defines it (the bits of mispmm_sddmm_bsr_bf16, then one fp32 fma with the mask, or the fp32
 * product scale * s without one):
 *   delta[r]   = sum_c dO[r,c] * O[r,c]                   fp32; O = the forward's out as stored (fp32 or bf16 bits)
 *   P[r,key]   = exp(z[r,key] - lse[r])                   fp32, v_exp_f32 of fl(t * log2 e) as the forward; z = -Inf: +0
 *   dP[r,key]  = <dO[r,:Dv], V[key,:Dv]>                  v_mfma_f32_16x16x32_bf16, columns ascending, fp32 accumulation
 *   dS[r,key]  = fl(fl(P * fl(dP - delta[r])) * scale)    three fp32 operations, then rounded ONCE to bf16 (nearest even)
 *   dQ[r,:]    = sum over the stored keys of r    bf16(dS[r,key]) * K[key,:]
 *   dK[key,:]  = sum over the rows that store key bf16(dS[r,key]) * Q[r,:]
 *   dV[key,:]  = sum over the rows that store key bf16(P[r,key])  * dO[r,:]
 * PATTERNS.  A as in mispmm_attn_bsr_bf16: numBlockRows block rows of bS x bS blocks, M = numBlockRows * bS rows, K columns,
 * blockRowPtrs[numBlockRows + 1], blockColIdxs[numBlocks].  A^T: tBlockRowPtrs[K / bS + 1], tBlockColIdxs[numBlocks], a block
 * row of A^T listing the block rows of A that store that block column (mispmm_csr_transpose_host on the block arrays).  perm
 * (uint32 [numBlocks]): block t of A^T is block perm[t] of A; read only with a mask, may be NULL without one.  Both patterns
 * are shared by all heads; a pattern that repeats a block is summed as often as it is stored.
 * OPERANDS.  Q [H][M][D], Kmat [H][K][D], V [H][K][Dv], dO [H][M][Dv]: raw bf16 bits, row strides ldq / ldk / ldv / ldg and
 * head strides in elements, as in the forward.  out [H][M][Dv]: what the forward wrote, fp32 or bf16 bits by out_bf16, strides
 * ldo / o_head.  lse: fp32 [H][M] contiguous, the forward's.  delta: fp32 [H][M] contiguous WORKSPACE the call writes (all of
 * it) and then reads; required whenever dQ or dK is asked for.  mask and scale as in the forward.  dQ [H][M][D], dK [H][K][D],
 * dV [H][K][Dv]: fp32, or bf16 bits with grads_bf16 (the fp32 sum rounded once, to nearest even; a NaN stays a NaN), each with
 * its own row and head stride.  EACH MAY BE NULL: its work is skipped and the other outputs keep their bits; all three NULL is
 * a no-op.  Only columns 0 .. D - 1 (Dv - 1) of a row are written.  out, tBlockRowPtrs / tBlockColIdxs and perm are looked at
 * only by the passes that need them: out and delta with dQ or dK, the transposed pattern with dK or dV.  No output may overlap
 * an input or another output.
 * LIMITS, as in the forward.  bS 16 or 32 and D, Dv multiples of 8 from 8 to 128, else MISPMM_ERR_UNSUPPORTED.  scale finite
 * and > 0, K a multiple of bS, every leading dimension >= its width, no required pointer null, else MISPMM_ERR_INVALID_ARG.
 * Every pointer that is used 16-byte aligned, bf16 row and head strides multiples of 8, fp32 ones multiples of 4, and every
 * operand of one head spanning less than 2 GiB, else MISPMM_ERR_UNSUPPORTED.  Every refusal precedes any device work and
 * leaves a message that names attn_bsr_bwd_bf16 in mispmm_last_error().  H == 0, numBlockRows == 0 or all of dQ, dK, dV
 * NULL: a no-op (after the checks of bS, scale, D, Dv and K).  A block column of A at or past K / bS reads zeros for K and V
 * (as the forward) and a block row named by tBlockColIdxs at or past numBlockRows contributes nothing.
 * ZERO ROWS.  An empty block row of A writes +0 to its bS rows of dQ; an empty block row of A^T writes +0 to its bS rows of dK
 * and dV.
 * ALGORITHM.  THE ROW PASS (with dQ or dK): one wave owns 16 query rows of one head, holds their Q and dO fragments, forms
 * delta -- a lane sums its 8 columns of each 32-column step of Dv ascending by fma, the four lanes of a row meet as
 * (g0 + g1) + (g2 + g3) -- writes it, and, with dQ, walks the block row 32 keys at a step in storage order (two blocks at
 * bS = 16, the odd last one alone; one block at bS = 32): S^T and dP^T by MFMA with K resp. V rows as the A operand, P and dS
 * in the lane that holds lse and delta of the element's row, dQ^T += K^T dS^T by MFMA, fp32 accumulators from +0, step after
 * step.  THE COLUMN PASS (with dK or dV; after the row pass on the same stream): one wave owns 16 keys, holds their K and V
 * fragments and walks its block row of A^T 32 queries at a step in storage order, the same products with Q resp. dO rows as
 * the A operand; dK^T += Q^T dS, dV^T += dO^T P.  With dV alone the row pass, dP and dS are skipped.  No atomics, no LDS;
 * every sum has a fixed order: run to run identical, and the result of a head does not depend on H, on the strides, or on
 * which other outputs are asked for.  Nothing is allocated: capturable (one stream, no parallel branches).
 * SPECIAL VALUES.  A masked element (z = -Inf) beside a finite lse has P = +0 and dS = +-0 and contributes exactly +0 to every
 * sum.  A matrix row whose lse is not finite (the forward's NaN rows: all keys masked, a NaN, a +Inf) gives NaN in its row of
 * dQ and in the dK / dV rows of every key it stores, as torch and the three-launch chain do.
 * NUMERICS.  u = 2^-24, r8 = 2^-8 (one rounding to bf16), g_n = n 2^-23 / (1 - n 2^-23) the any-order fp32 dot product of n
 * terms; `exact` on real arithmetic from the bf16 inputs; first order, every propagated factor taken at (value + its own error),
 * 1.01 on the whole.  L: the keys a row stores; T = max |z - m| over the row's finite z.
 *   E_z      scale E_s + u |scale s| + u |z|        E_s the SDDMM bound of mispmm.h over D terms; the rounded scale; the fma
 *   E_lse    max_row E_z + (L + 8 T + 16) u + 2 u (|lse| + ln L + 1)                                   (mispmm_attn.h)
 *   P        |P^ - P| <= P (exp(E_a) - 1) + (3 t + 2) u P exp(E_a) + 2^-126 =: E_P,  E_a = E_z + E_lse, t = |z - lse| + E_a:
 *            the argument's error through exp; the difference, the product with log2 e and v_exp_f32, counted as
 *            mispmm_softmax_bsr_f32 counts them, on the perturbed P; a flushed subnormal.  Where P enters dV: + r8 (P + E_P)
 *   dP       |dP^ - dP| <= the SDDMM bound over Dv terms + <E_g, |V|> =: E_dP;  E_g = r8 |dO| where the caller rounded a float32
 *            grad_out to bf16 before the call (the `exact` then being on the unrounded one), 0 for a grad_out given in bf16
 *   delta    |delta^ - delta| <= g_Dv sum (|dO| + E_g)(|O| + E_out) + sum (|dO| + E_g) E_out + sum E_g |O| =: E_delta,
 *            E_out the forward's tolerance on out for the out type in use (a bf16 out: 2^-8 |out| is part of it)
 *   dS       |dS^ - dS| <= scale (E_P X + P (E_dP + E_delta)) + (4 u + r8) scale (P + E_P) X + 2^-126 =: E_dS,
 *            X = |dP - delta| + E_dP + E_delta: four fp32 roundings (the difference, two products, the fp32 scale), one to bf16
 *   dQ       |dQ^ - dQ| <= sum E_dS |K| + g_L sum (|dS| + E_dS) |K|;  dK the same over the n rows that store the key, with
 *            |Q| and g_n;  dV: sum (E_P + r8 (P + E_P)) (|dO| + E_g) + g_n sum (P + that) (|dO| + E_g) + sum P E_g.
 *            A bf16 gradient adds r8 (|exact| + the bound).
 * tests/_attn_fused_bwd_ref.py::bwd_tolerances evaluates exactly these in float64 and the tests hold the kernels to them.
 * One wave per unit, 4 waves to a workgroup, the grid over (head, unit) in XCD order.  No LDS, no scratch.
 * mispmm_last_kernel() = attn_bsr_bwd_rows<b16|b32,mask|nomask,D2|D4,V2|V4> + attn_bsr_bwd_cols<...>, the tags of the launches
 * made joined by " + " (dV alone: the cols tag; dQ alone: the rows tag): D<n> / V<n> 32-column steps of D / Dv held in
 * registers (2: up to 64 columns, 4: up to 128).  The types of out and of the gradients are run-time branches outside the
 * loops and not part of a tag. */
int mispmm_attn_bsr_bwd_bf16(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                             const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint32_t *tBlockRowPtrs,
                             const uint32_t *tBlockColIdxs, const uint32_t *perm, const uint16_t *Q, uint32_t ldq, uint64_t q_head,
                             const uint16_t *Kmat, uint32_t ldk, uint64_t k_head, const uint16_t *V, uint32_t ldv, uint64_t v_head,
                             const uint16_t *dO, uint32_t ldg, uint64_t g_head, const void *out, uint32_t ldo, uint64_t o_head, int out_bf16,
                             const float *lse, float *delta, uint32_t D, uint32_t Dv, const float *mask, float scale, void *dQ, uint32_t lddq,
                             uint64_t dq_head, void *dK, uint32_t lddk, uint64_t dk_head, void *dV, uint32_t lddv, uint64_t dv_head,
                             int grads_bf16);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_BWD_H */
