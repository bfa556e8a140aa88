/* mispmm_sddmm_bf16.h -- C ABI of libmispmm_sddmm_bf16.so: SDDMM on a CSR pattern with both dense operands in bf16, for AMD
 * CDNA4 (gfx950).
 *
 * A ninth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, enum mispmm_acc_mode,
 * mispmm_last_error() and mispmm_last_kernel() are that library's, and a call here leaves its message and its kernel tag
 * there.  Conventions as in mispmm.h: device pointers, row-major dense operands, a call only enqueues on `stream`, and every
 * argument is validated before any device work.
 */
#ifndef MISPMM_SDDMM_BF16_H
#define MISPMM_SDDMM_BF16_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ out[e] = <X[row(e), :], Y[col(e), :]> on a CSR pattern, X and Y bf16 */
/* A is M x K, given by its pattern alone: rowPtrs[M + 1], colIdxs[nnz]; A's values are not read.  For every stored entry e
 * of row r,  out[e] = sum over j < N of x[r][j] * y[colIdxs[e]][j].  Rows may be ragged, empty or long and may hold unsorted
 * or repeated columns.  The backward of C = A @ B with respect to A's values is this product with X = dC, Y = B.
 * OPERANDS.  X: [M][N], Y: [K][N] raw bf16 bits, row stride ldx / ldy elements (>= N); the gap columns N .. ld - 1 of a
 * strided operand are never read.  out: nnz elements in A's storage order, fp32; with out_bf16 raw bf16 bits: the same fp32
 * result rounded once, to nearest even, by v_cvt_pk_bf16_f32 as mispmm_f32_to_bf16 does (a NaN stays a NaN).  The out type
 * is a wave-uniform branch at the store: it costs no kernel instances.  out must not overlap an input.
 * NUMERICS, exact contracts.  x, y = the elements widened to fp32 exactly (bits << 16: subnormals, -0 and NaN payloads as
 * they are, nothing flushed).  ALGORITHM: G lanes own a row of A; lane l owns the V consecutive columns
 * c * G * V + l * V .. + V - 1 of every chunk c of G * V columns.  Every lane runs ONE chain that starts at acc = +0 and
 * takes its columns in ascending order (chunks ascending, the V elements of a chunk ascending):
 *   MISPMM_ACC_FAST        acc = fmaf(x, y, acc) in fp32                          one rounding per column
 *   MISPMM_ACC_REFERENCE   acc = fma((double)x, (double)y, acc) in fp64           the product is exact: one rounding, at the add
 * A lane all of whose columns lie past N contributes +0.  The G lane sums are then added as a butterfly adds them: every
 * lane l takes s = s + (the s of lane l ^ 1), then of l ^ 2, l ^ 4, ... up to l ^ (G / 2), in the chain's type; REFERENCE
 * rounds to fp32 once at the end.  No packed dot instruction is used (v_dot2_f32_bf16 does not state its rounding), no
 * atomics: results are identical from run to run.  Consequences:
 *   (a) on V1 the order is that of mispmm_sddmm_csr_f32 on its element lanes: at a width where that kernel takes element
 *       lanes too (N not a multiple of 4), out equals its result on the widened operands bit for bit, in both modes;
 *   (b) in REFERENCE, whenever the exact sum fits 53 bits -- 16 product bits + the spread of the products' exponents +
 *       ceil(log2 N) <= 53 -- every partial sum is exact and out is the correctly rounded fp32 value of the real-number sum,
 *       whatever the lane width;
 *   (c) in FAST, |out - exact| <= g * S with g = N * 2^-24 / (1 - N * 2^-24), S = sum |x||y|: the bound mispmm.h states for
 *       mispmm_sddmm_csr_f32;
 *   (d) out[e] is NaN or +-Inf exactly where the sum of its products is; other entries are unaffected;
 *   (e) a product of two bf16 numbers has 16 significant bits: it is exact in fp32 unless it underflows or overflows fp32,
 *       the only inexact products.
 * LANE WIDTHS.  G = 8, 16, 32 or 64 (the smallest G with G * V >= N, 64 beyond); with G = 64 the group's slice of X's row
 * is held in registers for 1, 2 or 4 chunks (C1, C2, C4) or re-read per batch of 8 entries (C0: more than 4 chunks).
 *   V8   one 16-byte read per operand row and chunk: N, ldx and ldy multiples of 8, X and Y 16-byte aligned
 *   V1   one 2-byte read per column: everything else -- any N, any ld >= N, X and Y 2-byte aligned
 * The widest form the operands allow is taken; there is no V4.
 * SPECIAL CASES.  N == 0 writes +0 to every out[e] by one memset (tag sddmm_csr_bf16<zero>).  M == 0 or nnz == 0: a no-op,
 * after the checks that look at no pointer (acc_mode, leading dimensions).
 * REFUSALS, before any device work, each with its message in mispmm_last_error().  MISPMM_ERR_INVALID_ARG: an unknown
 * acc_mode; ldx < N or ldy < N; rowPtrs, colIdxs or out null with work to do; X or Y null with N > 0; X or Y not 2-byte
 * aligned; out not 4-byte (bf16 out: 2-byte) aligned.  MISPMM_ERR_UNSUPPORTED: M * ldx * 2 or K * ldy * 2 bytes reach
 * 2 GiB (buffer descriptors; there is no wide body).
 * One launch, no allocation, no synchronisation: capturable.  No LDS, no scratch.  mispmm_last_kernel() =
 * sddmm_csr_bf16<ref64|fast,G8|G16|G32|G64,V8|V1,C1|C2|C4|C0> f32|bf16 */
int mispmm_sddmm_csr_bf16(mispmm_stream_t stream, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs, const uint32_t *colIdxs,
                          const uint16_t *X, uint32_t ldx, const uint16_t *Y, uint32_t ldy, uint32_t N, void *out, int out_bf16,
                          int acc_mode);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_SDDMM_BF16_H */
