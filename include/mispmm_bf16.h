/* mispmm_bf16.h -- C ABI of libmispmm_bf16.so: the sparse product over a row list with B in bf16, for AMD CDNA4 (gfx950).
 *
 * A fourth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, enum mispmm_acc_mode,
 * mispmm_last_error() and mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag
 * there.  Conventions as in mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every
 * argument is validated before any device work.
 */
#ifndef MISPMM_BF16_H
#define MISPMM_BF16_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ C = A @ B over a row list, A's values fp32, B bf16 */
/* A is M x K, given as the row list mispmm_csr_f64 documents: rowPtrs[M + 1], colIdxs[nnz], vals[nnz].  A CSR is such a
 * list as it is; a COO is one once it is stable-sorted by row (rowPtrs = mispmm_coo_row_bounds); an ELL and the non-zero
 * list of a BSR (mispmm_bsr_nonzeros_host) are too.  rowPtrs == NULL: every row holds exactly rowNnz entries, row r at
 * [r * rowNnz, (r + 1) * rowNnz) -- a CSR of uniform rows and a row-major padded ELL of that width alike; M * rowNnz must
 * be nnz.  rowNnz is not read where rowPtrs is given.  In either form a column index of 0xFFFFFFFF marks a PADDING slot: it
 * is never a column, its B row is not read and its coefficient is not used, whatever it holds (an Inf, a NaN).
 * OPERANDS.  vals: fp32.  B: [K][N] raw bf16 bits, row stride ldb elements.  C: [M][N] fp32, row stride ldc; with out_bf16
 * raw bf16 bits: the fp32 result rounded once, to nearest even, by v_cvt_pk_bf16_f32 as mispmm_f32_to_bf16 does (a NaN
 * stays a NaN).  C must not overlap an input.
 * NUMERICS, exact contracts.  b = B's element widened to fp32 exactly (bits << 16: subnormals, -0 and NaN payloads as
 * they are, nothing flushed).  Every element of C is one chain that starts at acc = +0 and takes the row's entries e in
 * LIST order, a = vals[e], b = B[colIdxs[e]][j]:
 *   MISPMM_ACC_FAST                      acc = fmaf(a, b, acc)                                one rounding per entry
 *   MISPMM_ACC_REFERENCE, sum_f32 == 0   p = fl32(a * b);  acc (a double) += p;  C = fl32(acc)  the rule of the CSR reference
 *   MISPMM_ACC_REFERENCE, sum_f32 != 0   p = fl32(a * b);  acc = fl32(acc + p)                  the rule of COO / ELL / BSR
 * sum_f32 is ignored in FAST.  A padding slot contributes 0 * 0 = +0, and so does the end of every row: the stored value
 * is chain + (+0), which differs from the chain only where a sum has underflowed to -0 (stored as +0).  An empty row
 * writes +0 to its N columns.  Columns N .. ldc - 1 of C are never written.  No atomics: results are identical from run
 * to run and do not depend on the lane widths below.
 * LANE WIDTHS.  G = 8, 16, 32 or 64 lanes own one row of C (the smallest G with G * V >= N, 64 beyond), a lane V
 * consecutive columns:
 *   V8   one 16-byte read per B row: N and ldb multiples of 8, B and C 16-byte aligned, ldc a multiple of 4 (fp32 C: two
 *        16-byte stores per lane) or of 8 (bf16 C: one)
 *   V4   one 8-byte read: N and ldb multiples of 4, B and C 8-byte aligned, ldc a multiple of 2 (fp32 C: two 8-byte
 *        stores) or of 4 (bf16 C: one)
 *   V1   one 2-byte read: everything else -- any N, ldb >= N, ldc >= N, B 2-byte aligned, C 4-byte (bf16 C: 2-byte) aligned
 * The widest form the operands allow is taken.
 * REFUSALS, before any device work, each with its message in mispmm_last_error().  MISPMM_ERR_INVALID_ARG: an unknown
 * acc_mode; ldb < N or ldc < N; rowPtrs == NULL with M * rowNnz != nnz; colIdxs or vals null with nnz > 0; B or C null;
 * B not 2-byte aligned, C not 4-byte (bf16 C: 2-byte) aligned.  MISPMM_ERR_UNSUPPORTED: K * ldb * 2 bytes of B or
 * M * ldc * 4 (bf16 C: 2) bytes of C reach 2 GiB (buffer descriptors; there is no wide body).  M == 0 or N == 0: a no-op,
 * after the checks that look at no pointer (acc_mode, leading dimensions, M * rowNnz).
 * One launch, no allocation, no synchronisation: capturable.  mispmm_last_kernel() =
 * rows_bf16<G8|G16|G32|G64,V8|V4|V1,fast|ref64|ref32> f32|bf16 xcd 8x1  (xcd 1x1: fewer than 16 workgroups of rows, kept
 * in dispatch order). */
int mispmm_rows_bf16(mispmm_stream_t stream, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs, uint32_t rowNnz,
                     const uint32_t *colIdxs, const float *vals, const uint16_t *B, uint32_t N, uint32_t ldb, void *C, uint32_t ldc,
                     int out_bf16, int acc_mode, int sum_f32);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_BF16_H */
