/* mispmm_attn_csr.h -- C ABI of libmispmm_attn_csr.so: fused attention on a CSR pattern in fp32 for AMD CDNA4 (gfx950).
 *
 * A fifth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag there.  Conventions as in
 * mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every argument is validated
 * before any device work.
 */
#ifndef MISPMM_ATTN_CSR_H
#define MISPMM_ATTN_CSR_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Fused attention on a CSR pattern, fp32 */
/* What a multiply by the scale, mispmm_sddmm_csr_f32, mispmm_softmax_csr_f32 and mispmm_csr_f32 compute in four launches per
 * head, in ONE launch for H heads: neither the scores nor the weights are written.  A is M x K with rowPtrs[M + 1] and
 * colIdxs[nnz]; its values are not read and the pattern is shared by all heads.  Columns need not be sorted, and a
 * (row, column) pair stored twice counts twice.  For head h and row r, over the stored entries e of row r, c = colIdxs[e]:
 *   s[e]      = <Q_h[r, :D], K_h[c, :D]>
 *   z[e]      = fma(scale, s[e], bias_h[e])               one fp32 fma; bias == NULL: the term is +0
 *   out_h[r]  = sum_e softmax_e(z) * V_h[c, :Dv]
 *   lse_h[r]  = log sum_e exp z[e]                        natural logarithm
 * OPERANDS, all fp32.  Q [H][M][D], Kmat [H][K][D], V [H][K][Dv], out [H][M][Dv]: row strides ldq / ldk / ldv / ldo and head
 * strides in elements, any values: [H, M, D] storage, a [M, H, D] tensor viewed as [H, M, D], and a head stride of 0 on
 * Kmat and V (multi-query attention: one K and V for all heads).  bias: [H][nnz] in A's entry order with head stride
 * bias_head_stride (0: one bias shared by all heads), added to the scaled scores, -Inf = masked; NULL: none.  lse: [H][M]
 * contiguous, or NULL.  out and lse must not overlap an input.  Only columns 0 .. Dv - 1 of a row of out are written.
 * WIDTHS.  Every D and Dv from 1 to 256; 0 or above 256: MISPMM_ERR_UNSUPPORTED.  G = 8, 16, 32 or 64 lanes own one
 * (head, row), G the smallest with G * V >= max(D, Dv).  V4, 16-byte lanes: D, Dv, the four leading dimensions and the
 * head strides of Q, Kmat, V and out multiples of 4, their bases 16-byte aligned.  V1, element lanes: everything else; there
 * a wave holds 1, 2 or 4 chunks of 64 columns.
 * REFUSALS, before any device work, each with its message in mispmm_last_error().  MISPMM_ERR_UNSUPPORTED: D or Dv outside
 * 1 .. 256.  MISPMM_ERR_INVALID_ARG: a scale that is not finite.  Then H == 0 or M == 0: a no-op.  MISPMM_ERR_INVALID_ARG:
 * rowPtrs, Q, Kmat, V or out null, colIdxs null with nnz > 0; ldq < D, ldk < D, ldv < Dv, ldo < Dv.
 * MISPMM_ERR_UNSUPPORTED: the rows of one head of Q, Kmat, V or out, or nnz elements of bias, span 2 GiB or more (buffer
 * descriptors, as mispmm_sddmm_csr_f32); more than 2^31 - 1 workgroups.
 * ALGORITHM: ONLINE, one pass, fp32 throughout -- the FAST arithmetic of the three CSR kernels; there is no other.  The
 * row's entries are taken in storage order in batches of 8 (the last one partial).
 *   S        every lane sums the products of its columns by one fma chain from +0, columns ascending (V4: 4 consecutive
 *            columns per chunk); the lanes' sums meet in a fixed tree: lanes 1, 2, 4, 8, 16, 32 apart, in that order.
 *   z        one fma(scale, s, bias).
 *   maximum  mb = the largest z of the batch (a NaN is skipped); m = max(m, mb), m = -Inf before the first batch;
 *            mu = m, or 0 while m is infinite.
 *   weights  w = v_exp_f32(fl(fl(z - mu) * fl(log2 e))) with the batch's NEW mu.
 *   rescale  alpha = v_exp_f32(fl(fl(mu_old - mu_new) * fl(log2 e))), and exactly 1 while m_old is -Inf.
 *   divisor  t = ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)) over the batch (a slot past the row end: +0);
 *            l = fl(fl(l * alpha) + t).
 *   product  O = fl(alpha * O), then O = fma(w_i, V[c_i], O) for i = 0 .. 7 in order.  O and l are multiplied by the SAME
 *            bits of alpha, so alpha's own error cancels in the quotient except between earlier and later batches.
 *   out      O / l, an IEEE division per element: the divisor is the sum of the very weights that multiply V.  With V
 *            constant over a row's entries out returns that constant to within (L + 2 L / 8 + 3) 2^-24 relative.
 *   lse      mu + logf(l), from that same sum.
 * No atomics, no LDS; run to run identical; the result of a head does not depend on H or on any stride.
 * SPECIAL VALUES, as torch.softmax / torch.logsumexp on the L values z of a row: a -Inf bias is a masked entry and
 * contributes exactly +0 where the row has a finite score, also where all entries of the row's leading batches are masked;
 * a row holding a NaN or a +Inf score, or nothing but -Inf, is NaN in every element of out of that row and of no other, and
 * its lse is NaN, +Inf or -Inf respectively.  An EMPTY row writes +0 to its Dv columns and -Inf to lse.  A row of one finite
 * entry has w = 1, l = 1: out is that row of V, bit for bit (a -0 comes back as +0: O starts from +0).  A slot past the
 * end of a row and a lane past D or Dv read nothing: a NaN in a row of K or V that no entry of the row names -- row 0
 * included -- reaches no output.
 * NUMERICS.  u = 2^-24; L the row's length; T = max |z - m| over the row's finite z; `exact` in real arithmetic on the
 * fp32 operands.
 *   z     |z - exact| <= g_(D+1) (|scale| sum |q||k| + |bias|),  g_n = n u / (1 - n u)
 *   lse   |lse - exact| <= E_z + (L + 8 T + 16) u + 2 u (|lse| + ln L + 1),  E_z the largest z error of the row: l is off
 *         by less than (L + 8 T + 16) u relative (a term passes at most L / 8 + 4 additions and rescalings, its
 *         exponential costs (3 T + 2) u, the chain of rescale factors (3 T + 2 L / 8) u since the maximum only rises),
 *         then logf to an ulp and one addition.
 *   out   held to the tolerance the four-launch chain in FAST arithmetic is held to (the bounds of mispmm_sddmm_csr_f32,
 *         mispmm_softmax_csr_f32 and the product, composed); the scale is applied to S, not to Q, so the two roundings of
 *         q' = fl(q * scale) of the chain are here the one rounding of the fma.
 * One launch, no allocation, no synchronisation: capturable.  The (head, row block) items go over the XCDs in order, heads
 * slowest, so one head's K and V stay in an XCD's L2 while its rows are walked; a row is walked by ONE lane group, so the
 * longest row decides the tail of the launch.
 * mispmm_last_kernel() = attn_csr<f32,G8|G16|G32|G64,V4|V1,C1|C2|C4>  (C: chunks of G * V columns held in registers; C2 and
 * C4 only with G64,V1). */
int mispmm_attn_csr_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                        const uint32_t *colIdxs, const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat,
                        uint64_t k_head_stride, uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv,
                        uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, float *out, uint64_t out_head_stride,
                        uint32_t ldo, float *lse);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_CSR_H */
