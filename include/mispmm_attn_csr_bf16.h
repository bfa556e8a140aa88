/* mispmm_attn_csr_bf16.h -- C ABI of libmispmm_attn_csr_bf16.so: fused attention on a CSR pattern with Q, K and V in bf16 for
 * AMD CDNA4 (gfx950).
 *
 * A seventh library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag there.  Conventions as in
 * mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every argument is validated
 * before any device work.
 */
#ifndef MISPMM_ATTN_CSR_BF16_H
#define MISPMM_ATTN_CSR_BF16_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Fused attention on a CSR pattern, bf16 operands */
/* mispmm_attn_csr_f32 (mispmm_attn_csr.h) for a holder of bf16 Q, K and V: what three mispmm_bf16_to_f32 launches, that call
 * and a mispmm_f32_to_bf16 compute, in ONE launch for H heads, with no fp32 copy of any operand.  A is M x K with
 * rowPtrs[M + 1] and colIdxs[nnz]; its values are not read and the pattern is shared by all heads.  Columns need not be
 * sorted, and a (row, column) pair stored twice counts twice.  A bf16 value widens to fp32 EXACTLY (its 16 bits become the
 * upper half of the fp32, nothing flushed, a NaN's payload kept); with q, k, v the widened operands, for head h and row r,
 * over the stored entries e of row r, c = colIdxs[e]:
 *   s[e]      = <q_h[r, :D], k_h[c, :D]>
 *   z[e]      = fma(scale, s[e], bias_h[e])               one fp32 fma; bias == NULL: the term is +0
 *   out_h[r]  = sum_e softmax_e(z) * v_h[c, :Dv]
 *   lse_h[r]  = log sum_e exp z[e]                        natural logarithm
 * OPERANDS.  Q [H][M][D], Kmat [H][K][D], V [H][K][Dv]: bf16 bit patterns (uint16_t).  out [H][M][Dv]: fp32 (out_bf16 == 0)
 * or bf16 bit patterns (out_bf16 != 0): the SAME fp32 result rounded once to nearest even by v_cvt_pk_bf16_f32, a NaN stays a
 * NaN -- the rounding of mispmm_f32_to_bf16 and of mispmm_rows_bf16's bf16 C.  Row strides ldq / ldk / ldv / ldo and head
 * strides in ELEMENTS of the operand's own type, any values: [H, M, D] storage, a [M, H, D] tensor viewed as [H, M, D], and a
 * head stride of 0 on Kmat and V (multi-query attention: one K and V for all heads).  bias: fp32, [H][nnz] in A's entry order
 * with head stride bias_head_stride (0: one bias shared by all heads), added to the scaled scores, -Inf = masked; NULL:
 * none.  lse: fp32, [H][M] contiguous, or NULL.  out and lse must not overlap an input.  Only columns 0 .. Dv - 1 of a row of
 * out are written.
 * WIDTHS.  Every D and Dv from 1 to 256; 0 or above 256: MISPMM_ERR_UNSUPPORTED.  G lanes own one (head, row), G the smallest
 * with G * V >= max(D, Dv).  V8, 16-byte lanes, G = 8, 16 or 32, one chunk: D, Dv, the four leading dimensions and the head
 * strides of Q, Kmat, V and out multiples of 8, and the bases of Q, Kmat, V and out 16-byte aligned (also a bf16 out: a lane
 * stores 16 bytes of it).  V1, element lanes (buffer_load_ushort; a 2-byte store for a bf16 out), G = 8, 16, 32 or 64:
 * everything else; there a wave holds 1, 2 or 4 chunks of 64 columns.  There is no 8-byte lane form: the head widths in use
 * are multiples of 8.
 * REFUSALS, before any device work, each with its message in mispmm_last_error().  MISPMM_ERR_UNSUPPORTED: D or Dv outside
 * 1 .. 256.  MISPMM_ERR_INVALID_ARG: a scale that is not finite.  Then H == 0 or M == 0: a no-op.  MISPMM_ERR_INVALID_ARG:
 * rowPtrs, Q, Kmat, V or out null, colIdxs null with nnz > 0; ldq < D, ldk < D, ldv < Dv, ldo < Dv.
 * MISPMM_ERR_UNSUPPORTED: the rows of one head of Q, Kmat, V or out, or nnz elements of bias, span 2 GiB or more, counted in
 * BYTES of the operand's own element type (2 for Q, Kmat, V and a bf16 out, 4 for an fp32 out and bias: buffer descriptors);
 * more than 2^31 - 1 workgroups.  MISPMM_ERR_INVALID_ARG: a base of Q, Kmat, V or of a bf16 out that is not 2-byte aligned.
 * ALGORITHM: that of mispmm_attn_csr_f32, word for word, on the widened operands: ONLINE, one pass, fp32 throughout.  The
 * row's entries are taken in storage order in batches of 8 (the last one partial).
 *   S        every lane sums the products of its columns by one fma chain from +0, columns ascending (V8: 8 consecutive
 *            columns per chunk), each factor a widened bf16 -- no packed dot instruction; the lanes' sums meet in a fixed
 *            tree: lanes 1, 2, 4, 8, 16, 32 apart, in that order.
 *   z        one fma(scale, s, bias).
 *   maximum  mb = the largest z of the batch (a NaN is skipped); m = max(m, mb), m = -Inf before the first batch;
 *            mu = m, or 0 while m is infinite.
 *   weights  w = v_exp_f32(fl(fl(z - mu) * fl(log2 e))) with the batch's NEW mu.
 *   rescale  alpha = v_exp_f32(fl(fl(mu_old - mu_new) * fl(log2 e))), and exactly 1 while m_old is -Inf.
 *   divisor  t = ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)) over the batch (a slot past the row end: +0);
 *            l = fl(fl(l * alpha) + t).
 *   product  O = fl(alpha * O), then O = fma(w_i, v[c_i], O) for i = 0 .. 7 in order, O in fp32.
 *   out      O / l, an IEEE division per element; for a bf16 out then one rounding to nearest even.
 *   lse      mu + logf(l), from that same sum.
 * Where every score is exact in fp32 in any order of summation, z, every maximum, weight, rescale factor and the divisor are
 * determined by these words, and O is summed per column in one order: the fp32 out and lse are then BIT FOR BIT those of
 * mispmm_attn_csr_f32 on the widened operands.  Where scores round the two kernels may differ in S inside its bound: a
 * lane's chain covers 8 consecutive columns here and 4 there.
 * No atomics, no LDS; run to run identical; the result of a head does not depend on H or on any stride.
 * SPECIAL VALUES, as mispmm_attn_csr_f32: a -Inf bias is a masked entry and contributes exactly +0 where the row has a finite
 * score; a row holding a NaN or a +Inf score, or nothing but -Inf, is NaN in every element of out of that row and of no
 * other, and its lse is NaN, +Inf or -Inf respectively.  An EMPTY row writes +0 to its Dv columns and -Inf to lse.  A row of
 * one finite entry has w = 1, l = 1: out is that row of v (a -0 comes back as +0: O starts from +0).  A slot past the end
 * of a row and a lane past D or Dv read nothing: NaN bits in a row of Kmat or V that no entry of the row names -- row 0
 * included -- reach no output.
 * NUMERICS.  The bounds of mispmm_attn_csr_f32 (z, lse, out) on the widened operands, u = 2^-24; a bf16 out adds one rounding,
 * 2^-8 relative (2^-9 to nearest; subnormal results to the bf16 grid).
 * One launch, no allocation, no synchronisation: capturable.  The (head, row block) items go over the XCDs in order, heads
 * slowest, so one head's K and V stay in an XCD's L2 while its rows are walked; a row is walked by ONE lane group, so the
 * longest row decides the tail of the launch.
 * mispmm_last_kernel() = attn_csr_bf16<G8|G16|G32|G64,V8|V1,C1|C2|C4>  (C: chunks of G * V columns held in registers; G64, C2
 * and C4 only with V1). */
int mispmm_attn_csr_bf16(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                         const uint32_t *colIdxs, const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat,
                         uint64_t k_head_stride, uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv,
                         uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, void *out, uint64_t out_head_stride,
                         uint32_t ldo, int out_bf16, float *lse);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_CSR_BF16_H */
