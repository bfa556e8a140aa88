/* mispmm_attn_csr_bwd.h -- C ABI of libmispmm_attn_csr_bwd.so: the backward of fused attention on a CSR pattern in fp32 for AMD
 * CDNA4 (gfx950).
 *
 * A sixth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag there.  Conventions as in
 * mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every argument is validated
 * before any device work.
 */
#ifndef MISPMM_ATTN_CSR_BWD_H
#define MISPMM_ATTN_CSR_BWD_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Backward of fused attention on a CSR pattern, fp32 */
/* The gradients of mispmm_attn_csr_f32 (mispmm_attn_csr.h) with respect to Q, Kmat and V for H heads in AT MOST TWO launches,
 * whatever H: the scores, the weights and their gradients are written nowhere.  A, rowPtrs, colIdxs, Q, Kmat, V, scale and
 * bias are the forward's; out and lse are what the forward wrote; grad_out is the gradient of out.  For head h, entry e of
 * row r with c = colIdxs[e]:
 *   z[e]      = fma(scale, <Q_h[r, :D], K_h[c, :D]>, bias_h[e])        as in the forward
 *   P[e]      = exp(z[e] - lse_h[r])
 *   dP[e]     = <grad_out_h[r, :Dv], V_h[c, :Dv]>
 *   delta_h[r]= <grad_out_h[r, :Dv], out_h[r, :Dv]>
 *   dS[e]     = scale * P[e] * (dP[e] - delta_h[r])
 *   dQ_h[r]   = sum over the entries of row r of dS[e] K_h[c]
 *   dK_h[c]   = sum over the entries of column c of dS[e] Q_h[r]
 *   dV_h[c]   = sum over the entries of column c of P[e] grad_out_h[r]
 * The bias gets no gradient.
 * OPERANDS, all fp32.  Q [H][M][D], Kmat [H][K][D], V [H][K][Dv], out and grad_out [H][M][Dv], dQ [H][M][D], dK [H][K][D],
 * dV [H][K][Dv]: each with a row stride (ld*) and a head stride of its own, in elements, any values; a head stride of 0 is
 * allowed on Kmat, V and a shared bias (bias_head_stride 0).  dK and dV are ALWAYS per head: a caller that shares Kmat or V
 * over the heads sums the heads' gradients itself.  lse [H][M] and delta [H][M] contiguous; delta is a workspace the call
 * writes (delta_h[r] above) and may be read afterwards.  tRowPtrs[K + 1], tColIdxs[nnz]: the CSR pattern of A^T (row c lists
 * the rows r of A that store column c); perm[nnz], uint32: entry t of A^T is entry perm[t] of A.  perm is read only to index
 * the bias.  Only columns 0 .. width - 1 of a row of an output are written.
 * NULL OUTPUTS.  dQ, dK or dV may be NULL: that gradient is not computed and its work is skipped at run time.  dQ alone:
 * the row pass only.  dV alone: the column pass only, which then takes no dP, dS or delta.  dK (with or without dV) and no
 * dQ: the row pass stops after delta, then the column pass.  Neither dK nor dV: no column pass.  An output has the same
 * bits whatever else is asked for (given the same lane width, below).
 * WIDTHS.  Every D and Dv from 1 to 256.  G = 8, 16, 32 or 64 lanes own one output row, G the smallest with
 * G * V >= max(D, Dv), in both passes.  V4, 16-byte lanes: D, Dv, every leading dimension and head stride of Q, Kmat, V, out,
 * grad_out and of the outputs asked for multiples of 4, their bases 16-byte aligned.  V1: everything else; there a wave
 * holds 1, 2 or 4 chunks of 64 columns.
 * REFUSALS, before any device work, each with its message in mispmm_last_error().  MISPMM_ERR_UNSUPPORTED: D or Dv outside
 * 1 .. 256.  MISPMM_ERR_INVALID_ARG: a scale that is not finite.  Then H == 0, M == 0 or all three outputs NULL: a no-op.
 * MISPMM_ERR_INVALID_ARG: rowPtrs, Q, Kmat or V null, colIdxs null with nnz > 0; out, lse or grad_out null, delta null where
 * dQ or dK is asked for; tRowPtrs null, or tColIdxs null with nnz > 0, where dK or dV is asked for; perm null with a bias
 * where dK or dV is asked for; a leading dimension smaller than its width.  MISPMM_ERR_UNSUPPORTED: the rows of one head of
 * Q, Kmat, V, out or grad_out, or nnz elements of bias, span 2 GiB or more; more than 2^31 - 1 workgroups.
 * MISPMM_ERR_INVALID_ARG: dQ, dK, dV or delta overlapping an input or one another.
 * ALGORITHM: two passes, fp32 throughout, each the lane group of mispmm_attn_csr_f32.  Entries are taken in storage order in
 * batches of 8 (the last one partial); every accumulator starts from +0 and adds in storage order.
 *   s, dP    every lane sums the products of its columns by one fma chain from +0, columns ascending; the lanes' sums meet
 *            in the forward's fixed tree: lanes 1, 2, 4, 8, 16, 32 apart.  s has the same bits in both passes and the
 *            forward's.
 *   z        one fma(scale, s, bias).
 *   P        v_exp_f32(fl(fl(z - lse) * fl(log2 e))); NaN where lse is not finite.
 *   dS       fl(fl(P * fl(dP - delta)) * scale).
 *   ROW PASS     one lane group per (head, row r) on A's pattern.  delta[r]: each lane one fma chain over its columns of
 *                grad_out[r] and out[r], ascending, from +0; the lanes summed in the same tree; written to `delta`.
 *                dQ = fma(dS_i, K[c_i], dQ) for i = 0 .. 7 in order, batch after batch.
 *   COLUMN PASS  one lane group per (head, key c) on A^T's pattern, after the row pass on the same stream: it reads
 *                lse[r], delta[r] and bias[perm[t]] per entry.  dV = fma(P_i, grad_out[r_i], dV) and
 *                dK = fma(dS_i, Q[r_i], dK) for i = 0 .. 7 in order.
 * No atomics, no LDS, nothing allocated, no synchronisation: capturable.  Run to run identical; the result of a head does
 * not depend on H.
 * SPECIAL VALUES.  A -Inf bias beside a finite lse: P = exp2(-Inf) = +0 and dS = 0, the entry contributes exactly +0 to
 * every sum.  An empty row: a +0 row of dQ (and delta = <grad_out, out>, +0 on the forward's +0 row).  An empty column: +0
 * rows of dK and dV.  A row whose lse is not finite (a NaN or +Inf score, or nothing but -Inf): NaN in its dQ row and in
 * the dK and dV rows of every key it names, as torch and the four-launch chain give.  A slot past the end of a row or a
 * column and a lane past D or Dv read nothing: a NaN in a row of Q, Kmat, V or grad_out that no entry names -- row 0
 * included -- reaches no output.
 * NUMERICS.  u = 2^-24; g_n = n u / (1 - n u); L the number of entries summed; t = z - lse (<= 0 up to the errors below).
 *   z      |z - exact| <= E_z = g_(D+1) (|scale| sum |q||k| + |bias|)           the forward's
 *   P      |P - exact| <= P (E_z + E_lse + (3 |t| + 3) u) + 2^-126: the errors of z and of the STORED lse (the forward's
 *          bound), one rounding of the difference, (3 |t| + 2) u for the product with the rounded log2 e and v_exp_f32, and
 *          a flushed subnormal.
 *   dP     |dP - exact| <= g_Dv sum |g||v|
 *   delta  |delta - exact| <= g_Dv sum |g||o| + sum |g| E_out, E_out the error of the stored out
 *   dS     three roundings on top: |dS - exact| <= |scale| (E_P |dP - delta| + P (E_dP + E_delta) + 3 u P |dP - delta|)
 *   dQ, dK, dV   sum of the entries' errors times |K|, |Q|, |grad_out| plus g_L sum |terms|.
 * The gradients are NOT the bits of the four-launch chain, which normalises P by its own row sum and takes <P, dP>.
 * One row or one column is walked by ONE lane group: the longest of either decides the tail of its launch.
 * mispmm_last_kernel() = attn_csr_bwd_row<f32,G..,V..,C..> or attn_csr_bwd_col<f32,G..,V..,C..> of the LAST launch
 * (G8|G16|G32|G64, V4|V1, C1|C2|C4; C2 and C4 only with G64,V1). */
int mispmm_attn_csr_bwd_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                            const uint32_t *colIdxs, const uint32_t *tRowPtrs, const uint32_t *tColIdxs, const uint32_t *perm,
                            const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat, uint64_t k_head_stride,
                            uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv, uint32_t Dv, float scale,
                            const float *bias, uint64_t bias_head_stride, const float *out, uint64_t out_head_stride, uint32_t ldo,
                            const float *lse, const float *grad_out, uint64_t g_head_stride, uint32_t ldg, float *delta, float *dQ,
                            uint64_t dq_head_stride, uint32_t lddq, float *dK, uint64_t dk_head_stride, uint32_t lddk, float *dV,
                            uint64_t dv_head_stride, uint32_t lddv);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_CSR_BWD_H */
