/* mispmm_attn_csr_bf16_bwd.h -- C ABI of libmispmm_attn_csr_bf16_bwd.so: the backward of fused attention on a CSR pattern with Q,
 * K, V and grad_out in bf16 for AMD CDNA4 (gfx950).
 *
 * An eighth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag there.  Conventions as in
 * mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every argument is validated
 * before any device work.
 */
#ifndef MISPMM_ATTN_CSR_BF16_BWD_H
#define MISPMM_ATTN_CSR_BF16_BWD_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Backward of fused attention on a CSR pattern, bf16 operands */
/* The gradients of mispmm_attn_csr_bf16 (mispmm_attn_csr_bf16.h) with respect to Q, Kmat and V for H heads in AT MOST TWO
 * launches, whatever H, reading bf16: what up to four mispmm_bf16_to_f32 launches, mispmm_attn_csr_bwd_f32
 * (mispmm_attn_csr_bwd.h) and three mispmm_f32_to_bf16 launches compute, with no fp32 copy of any operand.  The scores, the
 * weights and their gradients are written nowhere.  A, rowPtrs, colIdxs, Q, Kmat, V, scale and bias are the forward's; out and
 * lse are the FP32 out and lse the forward wrote; grad_out is the gradient of out, in bf16.  A bf16 value widens to fp32
 * EXACTLY (its 16 bits become the upper half of the fp32, nothing flushed, nothing quieted); with q, k, v, g the widened Q,
 * Kmat, V and grad_out, for head h, entry e of row r with c = colIdxs[e]:
 *   z[e]      = fma(scale, <q_h[r, :D], k_h[c, :D]>, bias_h[e])        as in the forward
 *   P[e]      = exp(z[e] - lse_h[r])
 *   dP[e]     = <g_h[r, :Dv], v_h[c, :Dv]>
 *   delta_h[r]= <g_h[r, :Dv], out_h[r, :Dv]>
 *   dS[e]     = scale * P[e] * (dP[e] - delta_h[r])
 *   dQ_h[r]   = sum over the entries of row r of dS[e] k_h[c]
 *   dK_h[c]   = sum over the entries of column c of dS[e] q_h[r]
 *   dV_h[c]   = sum over the entries of column c of P[e] g_h[r]
 * The bias gets no gradient.
 * OPERANDS.  Q [H][M][D], Kmat [H][K][D], V [H][K][Dv] and grad_out [H][M][Dv]: bf16 bit patterns (uint16_t).  out [H][M][Dv],
 * lse [H][M], bias and delta [H][M]: fp32.  dQ [H][M][D], dK [H][K][D], dV [H][K][Dv]: fp32 (grads_bf16 == 0), or bf16 bit
 * patterns (grads_bf16 != 0): the SAME fp32 accumulators rounded once to nearest even by v_cvt_pk_bf16_f32, a NaN stays a NaN;
 * one flag for all three.  Each of Q, Kmat, V, out, grad_out, dQ, dK, dV has a row stride (ld*) and a head stride of its
 * own, in ELEMENTS of its own type, any values; a head stride of 0 is allowed on Kmat, V and a shared bias
 * (bias_head_stride 0).  dK and dV are ALWAYS per head: a caller that shares Kmat or V over the heads sums the heads'
 * gradients itself.  lse [H][M] and delta [H][M] contiguous; delta is a workspace the call writes (delta_h[r] above) and may be
 * read afterwards.  tRowPtrs[K + 1], tColIdxs[nnz]: the CSR pattern of A^T (row c lists the rows r of A that store column c);
 * perm[nnz], uint32: entry t of A^T is entry perm[t] of A.  perm is read only to index the bias.  Only columns
 * 0 .. width - 1 of a row of an output are written.
 * NOT BUILT: an fp32 grad_out.  A holder of one rounds it to bf16 first (mispmm_f32_to_bf16) or widens Q, Kmat and V and calls
 * mispmm_attn_csr_bwd_f32.
 * NULL OUTPUTS.  dQ, dK or dV may be NULL: that gradient is not computed and its work is skipped at run time.  dQ alone:
 * the row pass only.  dV alone: the column pass only, which then takes no dP, dS or delta.  dK (with or without dV) and no
 * dQ: the row pass stops after delta, then the column pass.  Neither dK nor dV: no column pass.  An output has the same
 * bits whatever else is asked for (given the same lane width, below).
 * WIDTHS.  Every D and Dv from 1 to 256.  G = 8, 16, 32 or 64 lanes own one output row, G the smallest with
 * G * V >= max(D, Dv), in both passes.  V8, 16-byte lanes, G = 8, 16 or 32: D, Dv and every leading dimension and head stride
 * of Q, Kmat, V and grad_out multiples of 8; the leading dimension and head stride of out multiples of 4; the bases of Q,
 * Kmat, V, grad_out and out 16-byte aligned; and of every output asked for the leading dimension and head stride multiples
 * of 4 (fp32) or 8 (bf16) and the base 16-byte aligned.  V1, element lanes (buffer_load_ushort; a 2-byte store for a bf16
 * gradient): everything else; there a wave holds 1, 2 or 4 chunks of 64 columns.  The lane width is decided once per call:
 * both passes carry the same tag suffix.
 * REFUSALS, before any device work, each with its message in mispmm_last_error().  MISPMM_ERR_UNSUPPORTED: D or Dv outside
 * 1 .. 256.  MISPMM_ERR_INVALID_ARG: a scale that is not finite.  Then H == 0, M == 0 or all three outputs NULL: a no-op.
 * MISPMM_ERR_INVALID_ARG: rowPtrs, Q, Kmat or V null, colIdxs null with nnz > 0; out, lse or grad_out null, delta null where
 * dQ or dK is asked for; tRowPtrs null, or tColIdxs null with nnz > 0, where dK or dV is asked for; perm null with a bias
 * where dK or dV is asked for; a leading dimension smaller than its width.  MISPMM_ERR_UNSUPPORTED: the rows of one head of
 * Q, Kmat, V, out or grad_out, or nnz elements of bias, span 2 GiB or more, counted in BYTES of the operand's own element type
 * (2 for Q, Kmat, V and grad_out, 4 for out and bias: buffer descriptors); more than 2^31 - 1 workgroups.
 * MISPMM_ERR_INVALID_ARG: a base of Q, Kmat, V, grad_out or of a bf16 gradient that is not 2-byte aligned; dQ, dK, dV or delta
 * overlapping an input or one another, on extents in bytes of each operand's own type.
 * ALGORITHM: that of mispmm_attn_csr_bwd_f32, word for word, on the widened operands: two passes, fp32 throughout, each the
 * lane group of mispmm_attn_csr_bf16.  Entries are taken in storage order in batches of 8 (the last one partial); every
 * accumulator starts from +0 and adds in storage order.
 *   s, dP    every lane sums the products of its columns by one fma chain from +0, columns ascending (V8: 8 consecutive
 *            columns), each factor a widened bf16 -- no packed dot instruction; the lanes' sums meet in the forward's fixed
 *            tree: lanes 1, 2, 4, 8, 16, 32 apart.  s has the same bits in both passes and the forward's.
 *   z        one fma(scale, s, bias).
 *   P        v_exp_f32(fl(fl(z - lse) * fl(log2 e))); NaN where lse is not finite.
 *   dS       fl(fl(P * fl(dP - delta)) * scale).
 *   ROW PASS     one lane group per (head, row r) on A's pattern.  delta[r]: each lane one fma chain over its columns of
 *                g[r] and out[r], ascending, from +0; the lanes summed in the same tree; written to `delta`.
 *                dQ = fma(dS_i, k[c_i], dQ) for i = 0 .. 7 in order, batch after batch.
 *   COLUMN PASS  one lane group per (head, key c) on A^T's pattern, after the row pass on the same stream: it reads
 *                lse[r], delta[r] and bias[perm[t]] per entry.  dV = fma(P_i, g[r_i], dV) and
 *                dK = fma(dS_i, q[r_i], dK) for i = 0 .. 7 in order.
 *   store        the fp32 accumulators, or each rounded once to bf16.
 * On V1 a lane's chains are those of mispmm_attn_csr_bwd_f32's V1 instance of the same G and C: dQ, dK, dV and delta are then
 * BIT FOR BIT that call's on the widened operands.  On V8 a lane's chain covers 8 consecutive columns here and 4 there: s, dP
 * and delta may differ inside their bounds, and are the same bits where every sum is exact in any order.
 * No atomics, no LDS, nothing allocated, no synchronisation: capturable.  Run to run identical; the result of a head does
 * not depend on H.
 * SPECIAL VALUES, as mispmm_attn_csr_bwd_f32.  A -Inf bias beside a finite lse: P = exp2(-Inf) = +0 and dS = 0, the entry
 * contributes exactly +0 to every sum.  An empty row: a +0 row of dQ (and delta = <g, out>, +0 on the forward's +0 row).  An
 * empty column: +0 rows of dK and dV.  A row whose lse is not finite (a NaN or +Inf score, or nothing but -Inf): NaN in its
 * dQ row and in the dK and dV rows of every key it names.  A slot past the end of a row or a column and a lane past D or Dv
 * read nothing: a NaN in a row of Q, Kmat, V or grad_out that no entry names -- row 0 included -- reaches no output.
 * NUMERICS.  The bounds of mispmm_attn_csr_bwd_f32 (z, P, dP, delta, dS, dQ, dK, dV) on the widened operands, u = 2^-24, with
 * E_lse and E_out the bf16 forward's; a bf16 gradient adds one rounding, 2^-8 relative (2^-9 to nearest; subnormal results to
 * the bf16 grid).
 * One row or one column is walked by ONE lane group: the longest of either decides the tail of its launch.
 * mispmm_last_kernel() = attn_csr_bf16_bwd_row<G..,V..,C..> or attn_csr_bf16_bwd_col<G..,V..,C..> of the LAST launch
 * (G8|G16|G32|G64, V8|V1, C1|C2|C4; G64, C2 and C4 only with V1). */
int mispmm_attn_csr_bf16_bwd(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                             const uint32_t *colIdxs, const uint32_t *tRowPtrs, const uint32_t *tColIdxs, const uint32_t *perm,
                             const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat, uint64_t k_head_stride,
                             uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv, uint32_t Dv, float scale,
                             const float *bias, uint64_t bias_head_stride, const float *out, uint64_t out_head_stride, uint32_t ldo,
                             const float *lse, const uint16_t *grad_out, uint64_t g_head_stride, uint32_t ldg, float *delta,
                             int grads_bf16, void *dQ, uint64_t dq_head_stride, uint32_t lddq, void *dK, uint64_t dk_head_stride,
                             uint32_t lddk, void *dV, uint64_t dv_head_stride, uint32_t lddv);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_CSR_BF16_BWD_H */
