/* mispmm_bsr_fp8.h -- C ABI of libmispmm_bsr_fp8.so: the block-sparse product C = A @ B with A's blocks and B in fp8 (OCP
 * e4m3, the bytes of torch.float8_e4m3fn) on v_mfma_f32_16x16x32_fp8_fp8, for AMD CDNA4 (gfx950).
 *
 * A thirteenth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag there.  Conventions as in
 * mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every argument is validated
 * before any device work.
 */
#ifndef MISPMM_BSR_FP8_H
#define MISPMM_BSR_FP8_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ C = diag(rowScale) (A @ B) diag(colScale), A and B e4m3 */
/* A is (numBlockRows * bS) x K in BSR with square blocks, bS = 16 or 32: blockRowPtrs[numBlockRows + 1],
 * blockColIdxs[numBlocks], and `blocks`: numBlocks * bS * bS e4m3 bytes in A's block order, row-major inside a block, as
 * mispmm_bsr_bf16 takes its bf16 blocks.  B: [K][N] e4m3 bytes, row stride ldb bytes, unit column stride; the gap columns
 * N .. ldb - 1 are never read.  C: [numBlockRows * bS][N], row stride ldc elements, fp32, or with c_bf16 raw bf16 bits.
 * rowScale: numBlockRows * bS floats or NULL; colScale: N floats or NULL -- the per-row scale of a quantised A and the
 * per-column scale of a quantised B factor out of every sum exactly, so the kernel applies them in its epilogue.
 * THE CONTRACT.   C[i][j] = fl(fl(acc * rowScale[i]) * colScale[j])
 * with acc the fp32 accumulator after the fixed-order cross-wave sum (below), fl the fp32 rounding to nearest even, the two
 * multiplies separate and in this order.  A NULL scale skips its multiply: it is not a multiply by 1 (the bits of a NaN's
 * payload and the sign of a zero are acc's).  A bf16 C is that fp32 value rounded once, to nearest even, by
 * v_cvt_pk_bf16_f32 (a NaN stays a NaN).  An empty block row is written as +0, whatever the scales hold.  With ldc > N the
 * elements between N and ldc are not written.  C must not overlap an input.
 * ALGORITHM.  One workgroup of 4 waves per (block row, super-tile of 128 output columns; of 256 where N >= 256 and N and ldb
 * are multiples of 16 and B is 16-byte aligned).  A K step is 32 k slots: a pair of 16 x 16 blocks in storage order (the
 * missing half of an odd pair is zeros and reads nothing of B), or one 32 x 32 block.  Step s of a block row runs on wave
 * s % 4; a wave adds its steps, ascending, into one fp32 accumulator per element inside the matrix instruction, and the four
 * partial sums are then added as ((w0 + w1) + w2) + w3 in fp32.  No atomics: the bits are the same run to run.
 * NUMERICS, with `exact` the real-number sum of an element's stored terms and S = sum |a||b| over them, before the scales:
 *   every e4m3 number is widened exactly -- the format has subnormals down to 2^-9, a NaN at 0x7F / 0xFF and no Inf -- and the
 *   product of two of them has at most 8 significant bits and an exponent of -18 .. 17: exact in fp32, never flushed.
 *   |acc - exact| <= g_n S,  g_n = n u / (1 - n u),  u = 2^-14 per addition,
 *   n = (the element's products that are not zero) + (steps its wave runs for the block row: ceil(ceil(blocks / 2) / 4) at
 *   16 x 16, ceil(blocks / 4) at 32 x 32) + 3 (the partial sums of the other waves): the form mispmm.h states for
 *   mispmm_bsr_bf16, with a MEASURED u.  The bf16 instruction keeps to u = 2^-23; the 8-bit one does not.  On an MI355X,
 *   against a float64 product of the widened operands, finite e4m3 values of every exponent (subnormals included) give a
 *   worst |acc - exact| / (g_n S at u = 2^-23) of 134.0 (16 x 16, N = 272; 55.6 at N = 24) and 52.4 (32 x 32, N = 272) in
 *   tests/test_gpu_bsr_fp8.py, and 74.7 over operands drawn by exponent spread at N = 24; the error is exactly zero while the
 *   operands span at most three binades and grows with the spread to 2^-12.1 S: the instruction aligns the 32 products of a
 *   step to the largest and drops what falls below its internal width.  u is the next power of two above 2 x 134.0 x 2^-23
 *   = 2^-14.9; the factor 2 covers inputs the runs did not draw.  Nothing here was widened by hand, and nothing was read off a manual.
 *   Each scale adds one rounding of its own: |C - exact r c| <= (g_n S + 2^-24 (2 + 2^-24) |acc|) |r c| barring underflow.
 *   Where every partial sum in every order is an fp32 number (integers in [-8, 8]: |sum| < 2^24) acc is exact.
 *   NaN: C[i][j] is NaN exactly where the sum of its terms is or a scale it meets is.  The kernel multiplies every stored
 *   element of a block: an explicit zero of A against a NaN of B is NaN.  It reads no B row for the missing half of an odd
 *   pair or past a block row's end.
 * REFUSALS, before any device work, in this order, each with its message in mispmm_last_error().
 *   MISPMM_ERR_INVALID_ARG   blockRowPtrs, B or C null; blockColIdxs or blocks null with numBlocks > 0
 *   MISPMM_ERR_UNSUPPORTED   bS other than 16 or 32
 *   MISPMM_ERR_UNSUPPORTED   N, ldb or ldc not a multiple of 8
 *   MISPMM_ERR_INVALID_ARG   ldb < N or ldc < N
 *   MISPMM_ERR_UNSUPPORTED   blocks or B not 8-byte aligned, C not 16-byte aligned, a scale not 4-byte aligned
 *   MISPMM_ERR_UNSUPPORTED   K * ldb reaches 2 GiB (B is read through one buffer descriptor)
 *   MISPMM_ERR_UNSUPPORTED   numBlockRows * super-tiles beyond 2^31 - 1 workgroups
 * numBlockRows == 0 or N == 0 is a no-op once the shape checks have passed (the grid aside).
 * One launch, no allocation, no synchronisation: capturable.  24 or 48 KiB of LDS, no scratch.  mispmm_last_kernel() =
 * bsr_mfma_fp8<b16|b32,T8|T16,c16|c32,scales|plain>; `scales` = at least one scale is given. */
int mispmm_bsr_fp8(mispmm_stream_t stream, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                   const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint8_t *blocks, const uint8_t *B, uint32_t N,
                   uint32_t ldb, const float *rowScale, const float *colScale, void *C, uint32_t ldc, int c_bf16);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_BSR_FP8_H */
