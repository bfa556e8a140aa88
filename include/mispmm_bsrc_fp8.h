/* mispmm_bsrc_fp8.h -- C ABI of libmispmm_bsrc_fp8.so: the block-sparse product C = A @ B with A column-compacted in 16-row
 * strips and fixed step slots, A's values and B in fp8 (OCP e4m3, the bytes of torch.float8_e4m3fn), on
 * v_mfma_f32_16x16x32_fp8_fp8, for AMD CDNA4 (gfx950).  The fp8 twin of mispmm_bsrc_slots_bf16 (mispmm.h).
 *
 * A fourteenth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag there.  Conventions as in
 * mispmm.h: device pointers (the host helper aside), row-major dense operands, a call only enqueues on `stream`, and every
 * argument is validated before any device work.
 */
#ifndef MISPMM_BSRC_FP8_H
#define MISPMM_BSRC_FP8_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ HOST: BSR blocks in e4m3 -> strips in step slots */
/* A is (numBlockRows * bS) x K in BSR with square blocks, bS = 16 or 32, `blocks_host`: numBlocks * bS * bS e4m3 bytes the
 * caller has quantised, in A's block order, row-major inside a block.  The matrix is cut into STRIPS of 16 rows, numBlockRows *
 * bS / 16 of them: a 32 x 32 block row is two independent strips.  Per strip the helper lists the columns in which any of the
 * 16 rows holds a byte x with (x & 0x7F) != 0 -- a NaN byte (0x7F, 0xFF) counts as occupied, +0 and -0 do not -- in ascending
 * order (a block column stored twice gives its columns twice, in storage order), pads the list with 0xFFFFFFFF to a multiple
 * of 32, and gathers the strip's bytes into one tile [16 rows][32 k] per step of 32 columns, 512 bytes, zeros where a row
 * holds nothing and under padding.  Placement as mispmm_bsr_compact_slots_bf16_host: the first 4 steps of strip R are steps
 * 4 R + w, w = 0 .. 3, a slot past the strip's step count being an all-padding column list with a zero tile; steps past the
 * fourth follow as step 4 * strips + extraPtrs[R] .. extraPtrs[R + 1].
 * Outputs NULL (all three) = size query: *nSteps_out = 4 * strips + extra steps, *nUsedSteps_out (may be NULL) = the steps
 * that hold values.  Then extraPtrs_out_host[strips + 1], cols_out_host[nSteps * 32], tiles_out_host[nSteps * 512].
 * REFUSALS, in this order: nSteps_out null; bS other than 16 or 32 (MISPMM_ERR_UNSUPPORTED); some but not all of the three
 * outputs; numBlockRows * bS beyond 2^32 - 1 (MISPMM_ERR_UNSUPPORTED); then whatever mispmm_bsr_check_host says of the
 * structure (M = numBlockRows * bS, the arrays as long as the counts claim), with its message; blocks_host null with
 * numBlocks > 0; 4 * strips + extra steps above 2^26 - 1 (MISPMM_ERR_UNSUPPORTED). */
int mispmm_bsr_compact_slots_fp8_host(uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                                      const uint32_t *blockRowPtrs_host, const uint32_t *blockColIdxs_host, const uint8_t *blocks_host,
                                      uint32_t *nSteps_out, uint32_t *nUsedSteps_out, uint32_t *extraPtrs_out_host,
                                      uint32_t *cols_out_host, uint8_t *tiles_out_host);

/* ---------------------------------------------------------- C = diag(rowScale) (A @ B) diag(colScale), A and B e4m3, strips */
/* A: numStrips strips of 16 rows as the helper above lays them out: extraPtrs[numStrips + 1], cols[nSteps * 32],
 * tiles[nSteps * 512] bytes.  B: [K][N] e4m3 bytes, row stride ldb bytes, unit column stride; the gap columns N .. ldb - 1
 * are never read.  C: [numStrips * 16][N], row stride ldc elements, fp32, or with c_bf16 raw bf16 bits.  rowScale:
 * numStrips * 16 floats or NULL; colScale: N floats or NULL.
 * THE CONTRACT is mispmm_bsr_fp8's (mispmm_bsr_fp8.h):   C[i][j] = fl(fl(acc * rowScale[i]) * colScale[j])
 * with acc the fp32 accumulator after the fixed-order sums below, fl the fp32 rounding to nearest even, the two multiplies
 * separate and in this order.  A NULL scale skips its multiply: it is not a multiply by 1.  A bf16 C is that fp32 value
 * rounded once, to nearest even, by v_cvt_pk_bf16_f32 (a NaN stays a NaN).  An empty strip -- one without an occupied column --
 * is written as +0, whatever the scales hold.  With ldc > N the elements between N and ldc are not written.  C must not
 * overlap an input.  nSteps is the extent of cols / tiles: nSteps == 4 * numStrips says there are NO extra steps, extraPtrs
 * must then be all zeros and is not read; with extra steps every extraPtrs[R + 1] <= nSteps - 4 * numStrips.  A live column
 * index must be below K: B is read through a buffer descriptor of its exact size, and an index past it reads zeros, never
 * memory.
 * ALGORITHM.  One workgroup of 4 waves per (strip, super-tile of 128 output columns).  Wave w multiplies the step in slot
 * 4 R + w: one v_mfma_f32_16x16x32_fp8_fp8 per 16 output columns, 8 per step, each into a fresh fp32 accumulator that sums the
 * step's 32 products inside the instruction.  Extra step i of a strip runs on wave 1 + i % 3, which adds its tile to the
 * wave's own in fp32, ascending.  The four partial tiles are then added as ((w0 + w1) + w2) + w3 in fp32 through LDS.  No
 * atomics: the bits are the same run to run.  Where C is fp32 and nSteps == 4 * numStrips wave q adds and stores rows
 * 4q .. 4q+3 of the strip (`share`), else wave 0 adds and stores all 16 (`w0`): the same bits either way.
 * NUMERICS, with `exact` the real-number sum of an element's stored terms and S = sum |a||b| over them, before the scales:
 *   every e4m3 number is widened exactly and the product of two of them is exact in fp32 (mispmm_bsr_fp8.h).
 *   |acc - exact| <= g_n S,  g_n = n u / (1 - n u),  u = 2^-14 per addition -- the u mispmm_bsr_fp8.h MEASURED for this
 *   instruction, which aligns the 32 products of a step to the largest and drops what falls below its internal width --
 *   n = (the element's products that are not zero) + (steps its wave runs for the strip: at most 1 + ceil(extra / 3)) + 3
 *   (the partial sums of the other waves).  tests/test_gpu_bsrc_fp8.py prints the worst |acc - exact| / (g_n S) at u = 2^-23
 *   and at u = 2^-14 for rows gathered from all over K (DESIGN.md section 9 item 33 keeps the figures).
 *   Each scale adds one rounding of its own: |C - exact r c| <= (g_n S + 2^-24 (2 + 2^-24) |acc|) |r c| barring underflow.
 *   Where every partial sum in every order is an fp32 number (integers in [-8, 8]: |sum| < 2^24) acc is exact.
 *   NaN, as the bf16 compacted products (mispmm.h): a column no row of the strip occupies is never multiplied and its B row
 *   is never read; an occupied column multiplies all 16 rows of the strip, stored zeros included, so a NaN in its B row makes
 *   the 16 rows NaN in that output column.  No B row is read for a padding column.
 * REFUSALS, before any device work, in this order, each with its message in mispmm_last_error().
 *   MISPMM_ERR_INVALID_ARG   extraPtrs, cols, tiles, B or C null
 *   MISPMM_ERR_UNSUPPORTED   N, ldb or ldc not a multiple of 8
 *   MISPMM_ERR_INVALID_ARG   ldb < N or ldc < N
 *   MISPMM_ERR_UNSUPPORTED   tiles or B not 8-byte aligned, C not 16-byte aligned, extraPtrs, cols or a scale not 4-byte aligned
 *   MISPMM_ERR_UNSUPPORTED   K * ldb reaches 2 GiB (B is read through one buffer descriptor)
 *   MISPMM_ERR_UNSUPPORTED   numStrips * 16 rows beyond 2^32 - 1, or numStrips * super-tiles beyond 2^31 - 1 workgroups
 *   MISPMM_ERR_INVALID_ARG   nSteps < 4 * numStrips
 * numStrips == 0 or N == 0 is a no-op once these checks have passed.
 * One launch, no allocation, no synchronisation: capturable.  24 KiB of LDS, no scratch.  mispmm_last_kernel() =
 * bsrc_slots_mfma_fp8<T8,c16|c32,scales|plain,share|w0>; T8 = 8 output tiles per lane (128-column super-tiles, the one form
 * built); `scales` = at least one scale is given. */
int mispmm_bsrc_slots_fp8(mispmm_stream_t stream, uint32_t numStrips, uint32_t K, uint32_t nSteps, const uint32_t *extraPtrs,
                          const uint32_t *cols, const uint8_t *tiles, const uint8_t *B, uint32_t N, uint32_t ldb, const float *rowScale,
                          const float *colScale, void *C, uint32_t ldc, int c_bf16);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_BSRC_FP8_H */
