/* mispmm_attn_fp8.h -- C ABI of libmispmm_attn_fp8.so: fused block-sparse attention forward with Q, K and V in fp8 (OCP
 * e4m3, the bytes of torch.float8_e4m3fn) on v_mfma_f32_16x16x32_fp8_fp8, for AMD CDNA4 (gfx950).
 *
 * A fifteenth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag there.  Conventions as in
 * mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every argument is validated
 * before any device work.
 */
#ifndef MISPMM_ATTN_FP8_H
#define MISPMM_ATTN_FP8_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Fused attention on a BSR pattern, Q, K and V in e4m3 */
/* mispmm_attn_bsr_bf16 (mispmm_attn.h) for operands that are already e4m3 -- an fp8 KV cache, an fp8 model -- without
 * widening them first: ONE launch for H heads, the scores and the weights never written.  A is numBlockRows block rows of
 * square bS x bS blocks, bS 16 or 32, M = numBlockRows * bS rows and K columns (a multiple of bS); blockRowPtrs, blockColIdxs
 * as in mispmm_attn_bsr_bf16; A's values are not read and the pattern is shared by all heads.  For head h and matrix row
 * r = R * bS + i of block row R, over the stored blocks e of R with c = blockColIdxs[e], q^ k^ v^ the e4m3 numbers:
 *   s[e][i][j] = <q^_h[r, :D], k^_h[c * bS + j, :D]>      v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulation
 *   z[e][i][j] = fl32(c_h * s + mask[e][i][j])            ONE fp32 fma; mask == NULL: the fp32 product c_h * s
 *   c_h        = fl(fl(scale * q_scale[h]) * k_scale[h])  formed once per wave; a NULL scale is no multiply
 *   out_h[r,:] = v_scale[h] * sum_e sum_j softmax_row(z)[e][j] * v^_h[c * bS + j, :Dv]
 *   lse_h[r]   = log sum_e sum_j exp(z[e][i][j])          natural logarithm, fp32
 * OPERANDS.  Q [H][M][D], Kmat [H][K][D], V [H][K][Dv]: e4m3 bytes, row-major, row strides ldq / ldk / ldv and head strides
 * q_head / k_head / v_head in elements (= bytes), any layout whose last dimension is contiguous, as in mispmm_attn_bsr_bf16.
 * q_scale, k_scale, v_scale: fp32 [H] DEVICE arrays, each nullable: the per-head scales of a quantised Q, K and V (x = x^ *
 * scale).  They are device arrays so that a caller that quantises on the device needs no synchronisation and the call stays
 * capturable; the kernel reads them by scalar loads.  NULL means 1 and no multiply.  Each given scale must be finite and
 * > 0: that cannot be checked without reading the device, so it is the CALLER'S CONTRACT and the call does not check it.
 * A violation is computed through as written above: a q_scale or k_scale that is 0, negative, Inf or NaN gives the z of that
 * c_h (0: every kept key weighs the same; negative: the softmax of the negated scores; Inf or NaN: NaN rows), a v_scale
 * that is not finite and > 0 multiplies out by it (0 * NaN and Inf * 0 are NaN); nothing is read or written out of bounds.
 * mask: fp32 [numBlocks][bS][bS] in A's block order, shared by all heads, added to the scaled scores, -Inf = masked; NULL:
 * none.  out [H][M][Dv], row stride ldo, head stride o_head: fp32, or raw bf16 bits with out_bf16 (the fp32 result rounded
 * once, to nearest even; a NaN stays a NaN).  lse: fp32 [H][M] contiguous, or NULL.
 * LIMITS.  bS 16 or 32, else MISPMM_ERR_UNSUPPORTED.  D a multiple of 16 from 16 to 128 (a lane reads 16 consecutive bytes of
 * a row of Q or K: wholly inside D or wholly dropped) and Dv a multiple of 8 from 8 to 128, else MISPMM_ERR_UNSUPPORTED.
 * scale finite and > 0, K a multiple of bS, ldq >= D, ldk >= D, ldv >= Dv, ldo >= Dv, no null pointer but mask, lse and the
 * scales (blockColIdxs may be null when numBlocks == 0), else MISPMM_ERR_INVALID_ARG.  Q, Kmat, mask and out 16-byte aligned
 * with ldq, ldk, q_head and k_head multiples of 16; V 8-byte aligned with ldv and v_head multiples of 8; ldo and o_head
 * multiples of 4 (bf16 out: 8); the scales 4-byte aligned; else MISPMM_ERR_UNSUPPORTED.  The rows of one head of Q, Kmat or V
 * span less than 2 GiB (buffer descriptors), else MISPMM_ERR_UNSUPPORTED.
 * REFUSALS, before any device work, in this order, each with its message in mispmm_last_error(): bS; scale; D or Dv not a
 * multiple of 8 in 8 .. 128; K not a multiple of bS; D not a multiple of 16 -- then H == 0 or numBlockRows == 0 is a no-op --
 * a null pointer; a leading dimension below its width; alignment of operands and strides; alignment of the scales; a head
 * that spans 2 GiB or more; more work units than one launch takes.
 * A block column at or past K / bS reads zeros for K and V.  out and lse must not overlap any input.  An EMPTY block row
 * writes +0 to its bS rows of out (all Dv columns, whatever v_scale holds) and -Inf to lse.  Only columns 0 .. Dv - 1 of a
 * row of out are written.
 * ALGORITHM.  The work split and the online softmax in fp32 are those of mispmm_attn_bsr_bf16: one pass over the block row,
 * 32 keys at a step (two blocks at bS = 16, the odd last one alone; one block at bS = 32) in storage order, a running
 * maximum m, the weights w = exp(z - mu) with mu = m (0 while m is infinite) by v_exp_f32 of fl(t * log2 e), running sums
 * and the accumulator O multiplied by exp(mu_old - mu_new) after every step (by 1 while everything so far is masked).
 * A score sums its D products inside the matrix instruction, 32 at a time: columns 64 s + 16 g + (0 .. 7), g = 0 .. 3, then
 * columns 64 s + 16 g + (8 .. 15), for s = 0, 1 -- a lane reads 16 consecutive bytes of a row and feeds the halves to
 * consecutive instructions.  The weights enter the second MFMA as e4m3 of fl(2^8 w), rounded once to nearest even by
 * v_cvt_pk_fp8_f32: w in (0, 1] lands in (0, 256] inside e4m3's range, 256 itself exact, and a weight flushes to zero only
 * below 2^-18 (unscaled it would below 2^-10: most of a long row).  The divisor l is the sum of the ROUNDED scaled weights --
 * the numbers the product multiplies by -- so
 *   out = fl(fl(O * fl(1 / l)) * v_scale[h]),   O / l = (sum w^ v^) / (sum w^),   w^ = e4m3(2^8 w):
 * a convex combination of V's rows up to fp32 rounding, the 2^8 cancelling without a multiply: where a column of V is
 * constant over the row's keys, out returns it to within (L + 16) 2^-24 relative, L = bS * (blocks of the block row), not
 * to 2^-4.  The two multiplies of out are separate.  lse comes from a second fp32 sum lx of the UNROUNDED, unscaled weights:
 * lse = mu + logf(lx).  Order of every sum: a lane sums keys 4g .. 4g + 3 of each 16-key tile of each step, ascending, step by
 * step; the four lanes g of a row meet once, as (g0 + g1) + (g2 + g3).  No atomics; run-to-run identical; the result of a
 * head does not depend on H or on the strides.
 * SPECIAL VALUES are exactly those of mispmm_attn_bsr_bf16, on the L values z of a matrix row: -Inf beside a finite z
 * contributes exactly +0, also when every key of the row's first steps is masked; a row that holds a NaN or a +Inf or
 * nothing but -Inf is NaN in every element of out of that matrix row and of no other row; lse is NaN, +Inf, -Inf for the
 * three.  e4m3 has no Inf and one NaN (0x7F / 0xFF): a NaN byte in Q or K makes the scores it meets NaN and so the rows
 * they belong to (a NaN in K: every row whose block row stores that key's block; in Q: that row); a NaN byte in V makes
 * the column it stands in NaN in every row whose block row stores its key's block -- also where the key is masked, 0 * NaN
 * -- and no other column.
 * NUMERICS.  u = 2^-24; `exact` with z_x = c_h * s_x + mask in real numbers on the e4m3 values (c_h the fp32 number above),
 * P_x = softmax_row(z_x); T = max |z - m| over the row's finite z.
 *   z     |z - z_x| <= E = g_n(U) * c_h * sum |q^||k^| + 2 u |z_x|,  g_n(U) = n U / (1 - n U),  U = 2^-14,
 *         n = (the score's products that are not zero) + (matrix instructions of its chain: D / 32, rounded up to even).
 *         U is the MEASURED per-addition unit of this instruction (mispmm_bsr_fp8.h, NUMERICS: it aligns the 32 products of
 *         a step to the largest and drops what falls below its internal width); the fma adds one fp32 rounding.
 *   lse   |lse - exact| <= E_r + (L + 8 T + 16) u + 2 u (|lse| + ln L + 1),  E_r = max E over the row's finite z: the bound
 *         of mispmm_attn_bsr_bf16 and the shift a score error can cause.
 *   out   with P' the real softmax of the kernel's z: P' <= exp(2 E_r) P_x, and before v_scale
 *         |out - P_x V| <= sum (|dP| + (exp(2 E_r) - 1) P_x) |v^| + g_nv(U) sum P^ |v^|,
 *         |dP| <= (2^-3 P' + (17 / 16) 2^-18 (1 + L P')) / (1 - L 2^-17) + (1 + 2^-3)((L + 8 T + 16) u P' + 2^-126) + 2^-126,
 *         P^ <= P' + |dP|,  nv = L + 2 (steps of the block row) + 2.
 *         This is the bound of mispmm_attn_bsr_bf16 with its 2^-8 become 2^-3: e4m3 rounds to nearest with 3 fraction bits,
 *         off by at most 1 / 17 relative (half an ulp, 2^-4, of a number at least 1 + 2^-4 ulps up its binade), and the
 *         divisor by as much the other way: (2 / 17) / (1 - 1 / 17) = 2^-3 to all orders.  Below 2^-6 (scaled) e4m3 is
 *         subnormal with spacing 2^-9: an absolute 2^-10, unscaled 2^-18, per weight, in the numerator once and in the
 *         divisor L times; the divisor is at least 2^8, the row's largest weight.  The second product runs on the same
 *         8-bit instruction: its sum is held to g_nv(U), not to the g_L(2^-23) of the bf16 one.  v_scale and the bf16
 *         rounding add their own roundings: |out_h - v_scale (..)| grows by 2 u |out| (bf16: 2^-9 |out|).
 *         tests/test_gpu_attn_fp8.py prints the worst observed share of each bound on finite e4m3 bytes of every exponent.
 * One wave owns 16 matrix rows of one head; 4 waves to a workgroup; the grid runs over (head, unit) in XCD order.  The longest
 * block row decides the tail of the launch.  No LDS, no scratch.
 * mispmm_last_kernel() = attn_bsr_fp8<b16|b32,f32|bf16,mask|nomask,D1|D2,T4|T8>: D<n> 64-column steps of D held in registers
 * (D1: D <= 64), T<n> accumulator tiles of 16 columns of Dv (T4: Dv <= 64).  One launch, no allocation: capturable. */
int mispmm_attn_bsr_fp8(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                        const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint8_t *Q, uint32_t ldq, uint64_t q_head,
                        const uint8_t *Kmat, uint32_t ldk, uint64_t k_head, const uint8_t *V, uint32_t ldv, uint64_t v_head, uint32_t D,
                        uint32_t Dv, const float *mask, float scale, const float *q_scale, const float *k_scale, const float *v_scale,
                        void *out, uint32_t ldo, uint64_t o_head, int out_bf16, float *lse);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_FP8_H */
