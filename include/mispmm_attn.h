/* mispmm_attn.h -- C ABI of libmispmm_attn.so: fused block-sparse attention forward in bf16 for AMD CDNA4 (gfx950).
 *
 * A second library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag there.  Conventions as in
 * mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every argument is validated
 * before any device work.
 */
#ifndef MISPMM_ATTN_H
#define MISPMM_ATTN_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Fused attention on a BSR pattern, bf16 */
/* What mispmm_sddmm_bsr_bf16 (fp32 scores), mispmm_softmax_bsr_f32 (bf16 P) and mispmm_bsr_bf16 compute in three launches
 * per head, in ONE launch for H heads: the scores and P are never written, and per matrix row only a log-sum-exp is kept.
 * A is numBlockRows block rows of square bS x bS blocks, bS 16 or 32, M = numBlockRows * bS rows and K columns (a multiple
 * of bS); blockRowPtrs[numBlockRows + 1], blockColIdxs[numBlocks] as in mispmm_bsr_bf16; A's values are not read and the
 * pattern is shared by all heads.  For head h and matrix row r = R * bS + i of block row R, over the stored blocks e of R
 * with c = blockColIdxs[e]:
 *   s[e][i][j] = <Q_h[r, :D], K_h[c * bS + j, :D]>        v_mfma_f32_16x16x32_bf16, columns ascending, fp32 accumulation: the
 *                                                         bits of mispmm_sddmm_bsr_bf16
 *   z[e][i][j] = fl32(scale * s + mask[e][i][j])          one fp32 fma; mask == NULL: the fp32 product scale * s: the z of
 *                                                         mispmm_softmax_bsr_f32
 *   out_h[r,:] = sum_e sum_j softmax_row(z)[e][j] * V_h[c * bS + j, :Dv]
 *   lse_h[r]   = log sum_e sum_j exp(z[e][i][j])          natural logarithm, fp32
 * OPERANDS.  Q [H][M][D], Kmat [H][K][D], V [H][K][Dv]: raw bf16 bits, row-major, row strides ldq / ldk / ldv and head
 * strides q_head / k_head / v_head in elements (any layout whose last dimension is contiguous: [H, M, D], [M, H, D], one
 * head with a stride of 0).  mask: fp32 [numBlocks][bS][bS] in A's block order, shared by all heads, added to the scaled
 * scores, -Inf = masked; NULL: none.  out [H][M][Dv], row stride ldo, head stride o_head: fp32, or raw bf16 bits with
 * out_bf16 (the fp32 result rounded once, to nearest even, as mispmm_f32_to_bf16; a NaN stays a NaN).  lse: fp32 [H][M]
 * contiguous, or NULL.  scale is applied here and not to Q, which would round Q a second time.
 * LIMITS.  bS 16 or 32 and D, Dv multiples of 8 from 8 to 128, else MISPMM_ERR_UNSUPPORTED.  scale finite and > 0, K a
 * multiple of bS, ldq >= D, ldk >= D, ldv >= Dv, ldo >= Dv, no null pointer but mask and lse (blockColIdxs may be null when
 * numBlocks == 0), else MISPMM_ERR_INVALID_ARG.  Every lane moves 16-byte vectors: Q, Kmat, V, mask and out 16-byte
 * aligned, ldq, ldk, ldv and the three head strides multiples of 8, ldo and o_head multiples of 4 (bf16 out: 8), else
 * MISPMM_ERR_UNSUPPORTED.  The rows of one head of Q, Kmat or V span less than 2 GiB (buffer descriptors), else
 * MISPMM_ERR_UNSUPPORTED.  Each refusal leaves its message in mispmm_last_error().  H == 0 or numBlockRows == 0: a no-op
 * (after the checks of bS, scale, D, Dv and K).  A block column at or past K / bS reads zeros for K and V.  out and lse
 * must not overlap any input.
 * An EMPTY block row writes +0 to its bS rows of out (all Dv columns) and -Inf to lse.  Only columns 0 .. Dv - 1 of a row
 * of out are written.
 * ALGORITHM.  Online softmax in fp32, one pass over the block row, 32 keys at a step (two blocks at bS = 16, the odd last
 * one alone; one block at bS = 32) in storage order: a running maximum m, the weights w = exp(z - mu) with mu = m (0 while
 * m is infinite) by v_exp_f32 of fl(t * log2 e), running sums and the accumulator O multiplied by exp(mu_old - mu_new)
 * after every step (by 1 while everything so far is masked).  The weights enter the second MFMA as bf16, rounded once to
 * nearest even, and the divisor l is the sum of the ROUNDED weights -- the numbers the product multiplies by -- so
 *   out = (sum w^ v) / (sum w^),   w^ = bf16(w):
 * a convex combination of V's rows up to fp32 rounding: where a column of V is constant over the row's keys, out returns
 * it to within (L + 16) 2^-24 relative, L = bS * (blocks of the block row), not to 2^-9.  out = O * fl(1 / l).  lse comes
 * from a second fp32 sum lx of the UNROUNDED weights: lse = mu + logf(lx).  Order of every sum: a lane sums keys
 * 4g .. 4g + 3 of each 16-key tile of each step, ascending, step by step; the four lanes g of a row meet once, as
 * (g0 + g1) + (g2 + g3).  No atomics; run-to-run identical; the result of a head does not depend on H or on the strides.
 * SPECIAL VALUES, as torch.softmax / torch.logsumexp on the L values z of a matrix row: -Inf beside a finite z contributes
 * exactly +0, also when every key of the row's first steps is masked; a row that holds a NaN or a +Inf or nothing but
 * -Inf is NaN in every element of out of that matrix row and of no other row; lse is NaN, +Inf, -Inf for the three (NaN
 * where a NaN and a +Inf meet).
 * NUMERICS.  u = 2^-24; T = max |z - m| over the row's finite z; `exact` on the fp32 z as defined above.
 *   lse   |lse - exact| <= (L + 8 T + 16) u + 2 u (|lse| + ln L + 1)
 *         lx is off by less than (L + 8 T + 16) u relative: a term passes at most L / 16 + 11 additions and rescalings,
 *         its exponential costs (3 T + 2) u as in mispmm_softmax_bsr_f32, and the chain of rescale factors (3 T + L / 16) u
 *         since the maximum only rises; then logf to an ulp and one addition.
 *   out   held to the bound the three-launch chain is held to: with P' = w / sum w the real softmax of z,
 *         |out - P' V| <= sum |dP||V| + g_L sum P^|V|,  |dP| <= 2^-8 P' + (1 + 2^-8)((L + 8 T + 16) u P' + 2^-126) + 2^-126,
 *         g_n = n 2^-23 / (1 - n 2^-23).  Rounding w to bf16 is off by 2^-9 relative and so, at worst, is the divisor: the
 *         two halves of the 2^-8.  The rescalings add 2 u per step to numerator and divisor alike; they are inside g_L.
 * One wave owns 16 matrix rows of one head; 4 waves to a workgroup; the grid runs over (head, unit) in XCD order, so a
 * head's K and V stay in one XCD's L2.  The longest block row decides the tail of the launch.  No LDS, no scratch.
 * mispmm_last_kernel() = attn_bsr<b16|b32,f32|bf16,mask|nomask,D2|D4,T4|T8>: D<n> 32-column steps of D held in registers
 * (D2: D <= 64), T<n> accumulator tiles of 16 columns of Dv (T4: Dv <= 64).  One launch, no allocation: capturable. */
int mispmm_attn_bsr_bf16(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                         const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint16_t *Q, uint32_t ldq, uint64_t q_head,
                         const uint16_t *Kmat, uint32_t ldk, uint64_t k_head, const uint16_t *V, uint32_t ldv, uint64_t v_head, uint32_t D,
                         uint32_t Dv, const float *mask, float scale, void *out, uint32_t ldo, uint64_t o_head, int out_bf16, float *lse);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_H */
