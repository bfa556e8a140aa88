/* mispmm_attn_csr_dbias.h -- C ABI of libmispmm_attn_csr_dbias.so: the bias gradient of fused attention on a CSR pattern, for
 * fp32 operands and for bf16 ones, for AMD CDNA4 (gfx950).
 *
 * A tenth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag there.  Conventions as in
 * mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every argument is validated
 * before any device work.
 */
#ifndef MISPMM_ATTN_CSR_DBIAS_H
#define MISPMM_ATTN_CSR_DBIAS_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Bias gradient of fused attention on a CSR pattern, fp32 and bf16 */
/* The gradient of mispmm_attn_csr_f32 (mispmm_attn_csr.h) and of mispmm_attn_csr_bf16 (mispmm_attn_csr_bf16.h) with respect to
 * the bias, the additive term over A's entries, for H heads in ONE launch: the scores and the weights are written nowhere.  A,
 * rowPtrs, colIdxs, Q, Kmat, V, scale and bias are the forward's; out and lse are what the forward wrote; grad_out is the
 * gradient of out.  Every symbol as in mispmm_attn_csr_bwd.h; for head h, entry e of row r with c = colIdxs[e]:
 *   z[e]      = fma(scale, <Q_h[r, :D], K_h[c, :D]>, bias_h[e])        as in the forward
 *   P[e]      = exp(z[e] - lse_h[r])
 *   dP[e]     = <grad_out_h[r, :Dv], V_h[c, :Dv]>
 *   delta_h[r]= <grad_out_h[r, :Dv], out_h[r, :Dv]>
 *   dBias_h[e]= P[e] * (dP[e] - delta_h[r])                            no scale: dz / dbias = 1
 * It is the gradient with respect to the scores' additive term whether or not a bias was given: with a NULL bias the term is
 * +0 and dBias is the gradient with respect to z.
 * OPERANDS.  _f32: Q [H][M][D], Kmat [H][K][D], V [H][K][Dv], out and grad_out [H][M][Dv] in fp32.  _bf16: Q, Kmat, V and
 * grad_out are bf16 bits, widened exactly; out stays fp32, as the bf16 forward wrote it.  Each with a row stride (ld*) and a
 * head stride of its own, in elements, any values; a head stride of 0 is allowed on Kmat, V and a shared bias
 * (bias_head_stride 0).  lse [H][M] fp32, contiguous.  bias [nnz] or [H][nnz] fp32 in A's entry order.  dBias [H][nnz] fp32 with
 * its own head stride >= nnz: it is ALWAYS per head, as dK and dV of the backward are -- a caller that shares the bias over the
 * heads sums the heads' gradients itself.  Exactly the H * nnz entries are written, nothing between the heads.
 * NULLS.  bias may be NULL (above).  Nothing else may.  The `delta` workspace of the backward is neither read nor written:
 * the call runs alone and in any order relative to mispmm_attn_csr_bwd_f32 / mispmm_attn_csr_bf16_bwd.
 * WIDTHS.  Every D and Dv from 1 to 256.  G = 8, 16, 32 or 64 lanes own one row, G the smallest with G * V >= max(D, Dv).
 * 16-byte lanes (_f32: V4, _bf16: V8): D, Dv, every leading dimension and head stride of Q, Kmat, V and grad_out multiples of
 * the lane width, those of out multiples of 4, their bases 16-byte aligned.  V1: everything else; there a wave holds 1, 2 or 4
 * chunks of 64 columns.  dBias has no say.  This is the backward's rule on the operands read here: on the same operands (and,
 * there, gradients that allow its wide lanes) both land on the same (G, V, C).
 * REFUSALS, before any device work, each with its message in mispmm_last_error().  MISPMM_ERR_UNSUPPORTED: D or Dv outside
 * 1 .. 256.  MISPMM_ERR_INVALID_ARG: a scale that is not finite.  Then H == 0, M == 0 or nnz == 0: a no-op.
 * MISPMM_ERR_INVALID_ARG: rowPtrs, colIdxs, Q, Kmat or V null; out, lse, grad_out or dBias null; a leading dimension smaller
 * than its width; dbias_head_stride < nnz with H > 1.  MISPMM_ERR_UNSUPPORTED: the rows of one head of Q, Kmat, V, out or
 * grad_out, or nnz elements of bias, span 2 GiB or more; more than 2^31 - 1 workgroups.  MISPMM_ERR_INVALID_ARG: (_bf16) Q,
 * Kmat, V or grad_out not 2-byte aligned; dBias overlapping an input (the index arrays and lse among them).
 * ALGORITHM: one pass, fp32 throughout: the ROW PASS of the backward (mispmm_attn_csr_bwd.h) without its dQ, one lane group
 * per (head, row r) on A's pattern.  Entries are taken in storage order in batches of 8 (the last one partial).
 *   s, dP    every lane sums the products of its columns by one fma chain from +0, columns ascending; the lanes' sums meet
 *            in the forward's fixed tree: lanes 1, 2, 4, 8, 16, 32 apart.  The same bits as in the backward's passes.
 *   delta    each lane one fma chain over its columns of grad_out[r] and out[r], ascending, from +0; the lanes summed in the
 *            same tree; kept in a register.  The same bits as the backward's workspace.
 *   z        one fma(scale, s, bias).
 *   P        v_exp_f32(fl(fl(z - lse) * fl(log2 e))); NaN where lse is not finite.
 *   dBias    fl(P * fl(dP - delta)): the backward's dS before its last multiply, so fl(dBias * scale) is that dS bit for bit.
 * One lane stores one entry, live slots only; an empty row stores nothing.  No atomics, no LDS, nothing allocated, no
 * synchronisation: capturable.  Run to run identical; the result of a head does not depend on H.
 * SPECIAL VALUES.  A -Inf bias beside a finite lse: P = exp2(-Inf) = +0 and dBias is a zero of either sign.  A row whose lse
 * is not finite (a NaN or +Inf score, or nothing but -Inf): NaN in that row's entries and nowhere else.  A slot past the end of
 * a row and a lane past D or Dv read nothing: a NaN in a row of Q, Kmat, V or grad_out that no entry names -- row 0 included --
 * reaches no output.
 * NUMERICS.  u = 2^-24; g_n = n u / (1 - n u); E_z, E_P, E_dP, E_delta as in mispmm_attn_csr_bwd.h; x = dP - delta,
 * E_x = E_dP + E_delta.  Two roundings on top: |dBias - exact| <= E_P (|x| + E_x) + P E_x + 2 u P |x| -- the backward's dS
 * bound with one rounding fewer and no scale.
 * COST.  s and dP are computed a third time beside the backward's two passes, and one row is walked by ONE lane group: the
 * longest row decides the tail of the launch.
 * mispmm_last_kernel() = attn_csr_dbias<f32,G..,V..,C..> or attn_csr_dbias<bf16,G..,V..,C..> (G8|G16|G32|G64, V4|V8|V1,
 * C1|C2|C4; C2 and C4 only with G64,V1; bf16 V8 has no G64). */
int mispmm_attn_csr_dbias_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                              const uint32_t *colIdxs, const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat,
                              uint64_t k_head_stride, uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv,
                              uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, const float *out,
                              uint64_t out_head_stride, uint32_t ldo, const float *lse, const float *grad_out, uint64_t g_head_stride,
                              uint32_t ldg, float *dBias, uint64_t dbias_head_stride);

int mispmm_attn_csr_dbias_bf16(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                               const uint32_t *colIdxs, const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat,
                               uint64_t k_head_stride, uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv,
                               uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, const float *out,
                               uint64_t out_head_stride, uint32_t ldo, const float *lse, const uint16_t *grad_out,
                               uint64_t g_head_stride, uint32_t ldg, float *dBias, uint64_t dbias_head_stride);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_CSR_DBIAS_H */
