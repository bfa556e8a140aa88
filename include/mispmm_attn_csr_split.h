/* mispmm_attn_csr_split.h -- C ABI of libmispmm_attn_csr_split.so: the fused attention forward on a CSR pattern with every
 * long row SPLIT over several lane groups, fp32 and bf16 operands, for AMD CDNA4 (gfx950).
 *
 * A library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's.  Conventions as in mispmm.h: device pointers, row-major dense operands, a call only
 * enqueues on `stream`, and every argument is validated before any device work.
 */
#ifndef MISPMM_ATTN_CSR_SPLIT_H
#define MISPMM_ATTN_CSR_SPLIT_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Fused attention on a CSR pattern, rows split over lane groups */
/* What mispmm_attn_csr_f32 (mispmm_attn_csr.h) and mispmm_attn_csr_bf16 (mispmm_attn_csr_bf16.h) compute -- the same operands,
 * limits (D and Dv from 1 to 256, free head and row strides), lane-width rule (16-byte lanes where widths, strides and bases
 * allow, element lanes otherwise), special values and layout of out and lse; read those headers for them -- for the shapes
 * where one lane group per row leaves the card idle: few rows against very many keys (decoding, chunked prefill against a long
 * context), or a pattern whose longest row decides the tail of the launch.  TWO launches on `stream`: a partial kernel in which
 * (head, row, segment) is one lane group, and a combine kernel.
 * SEGMENTS, worked out in the kernels from rowPtrs; the host never reads the pattern.  A row of len entries has
 * n = ceil(len / 8) batches and S' = min(splits, max(1, floor(n / min_batches))) segments: every segment holds at least
 * min_batches batches and a short row (n < 2 min_batches) has S' = 1.  Segment s < S' walks batches floor(s n / S') ..
 * floor((s + 1) n / S') - 1 in storage order, floor(s n / S') formed as s floor(n / S') + floor(s (n mod S') / S').  No segment
 * below S' is empty, and only the row's true last segment can end in a partial batch.
 * WORK ITEM: (head, row, s) for s < splits, one lane group; the items of a head are numbered row * splits + s, so a workgroup
 * holds consecutive segments of one row (disjoint K and V rows, Q[r] shared through L1).  A group with s >= S' returns at once.
 * Inside its segment a group does exactly what the one-launch kernel does (the ALGORITHM of mispmm_attn_csr.h, for bf16 on the
 * exactly widened operands): the same z = fma(scale, <q, k>, bias) from one fma chain per lane, the same per-batch online
 * softmax, the same K-before-V issue order with the column and bias fetch one batch ahead.  Its ending:
 *   S' = 1   the group stores out and lse itself, the one-launch kernel's ending (O / l, mu + logf(l), one rounding to bf16
 *            where asked).  The workspace is not touched.
 *   S' > 1   the group stores its unnormalised state (m_s, l_s, O_s) to the workspace.
 * THE MERGE, per (head, row) with S' > 1, s ascending, in fp32, no contraction of its products and sums:
 *   1. M = fmax over the m_s (a NaN is dropped, as in the loop: no m_s is one).
 *   2. mu = 0 where |M| = Inf, else M; mu_s likewise from m_s.
 *   3. w_s = 1 where m_s = -Inf, else v_exp_f32(fl(fl(mu_s - mu) * fl(log2 e))): the loop's own exponential.
 *   4. l = sum w_s l_s and O = sum w_s O_s: fp32 products and sums, each sum STARTING FROM ITS FIRST TERM and not from zero.
 *   5. out = O / l, an IEEE division per element as in the one-launch kernel, rounded once (to nearest even) where bf16;
 *      lse = mu + logf(l).
 * Consequences.  splits = 1 gives the bits of the one-launch kernel for every row.  For any splits, every row with
 * n < 2 min_batches has those bits too: it has S' = 1.  A wholly masked segment has m_s = -Inf, l_s = 0, O_s = +0 and
 * contributes nothing (w_s = 1 times zeros).  The NaN, +Inf and all -Inf rules of a row are the one-launch kernel's and stay in
 * their row: a NaN weight or a +Inf score in any segment makes l NaN and so every element of that row, lse NaN or +Inf; a row
 * of nothing but -Inf has l = 0, out NaN and lse = -Inf.  There are no atomics, and results are run to run identical for the
 * same (splits, min_batches), independent of H and of the strides.
 * NUMERICS.  The bounds NUMERICS of mispmm_attn_csr.h states for out and lse hold for a split row as they stand, and they are
 * what is tested.  A split row is NOT the one-launch kernel's result plus one term: its running maximum restarts in every
 * segment, so the rounded differences fl(z - mu) and fl(mu_old - mu_new) fall at other maxima, and the merge adds one more
 * rescale factor w_s and an S'-term sum.  Each of these is of the kind those bounds already count per entry and per batch; no
 * tighter bound is stated for split rows.
 * WORKSPACE.  fp32, 16-byte aligned, caller-sized: mispmm_attn_csr_split_workspace() bytes = 4 * H * M * splits * (Dvp + 2),
 * Dvp = Dv rounded up to a multiple of 4.  With slot = (h * M + row) * splits + s: first O as [slots][Dvp], then the states as
 * [slots][2] = (m, l).  Contents are scratch: nothing is kept between calls and nothing need be cleared.  Slots of s >= S',
 * and every slot of a row with S' = 1, are never written or read.  The call makes two launches, allocates nothing and does
 * not synchronise: it can be captured into a graph.
 * REFUSALS, before any device work, each with its message in mispmm_last_error(), in this order.  MISPMM_ERR_UNSUPPORTED: D
 * or Dv outside 1 .. 256.  MISPMM_ERR_INVALID_ARG: a scale that is not finite; splits 0 or above 256 (256 and not the 64 of
 * mispmm_attn_split.h: a lane group is a quarter to a sixteenth of a wave); min_batches 0.  Then H == 0 or M == 0: a no-op.
 * MISPMM_ERR_INVALID_ARG: rowPtrs, Q, Kmat, V or out null, colIdxs null with nnz > 0; ldq < D, ldk < D, ldv < Dv, ldo < Dv.
 * MISPMM_ERR_UNSUPPORTED: the rows of one head of Q, Kmat, V or out, or nnz elements of bias, span 2 GiB or more;
 * M * splits >= 2^32; more than 2^31 - 1 workgroups for the M * splits items of each of H heads (or for the combine launch's
 * M / 4 per head).  MISPMM_ERR_INVALID_ARG: a base of bf16 Q, Kmat, V or of a bf16 out that is not 2-byte aligned; a null,
 * misaligned or too small workspace -- the message names the bytes needed.
 * Work split: 256-thread workgroups of 256 / G lane groups, G as in the one-launch kernel; no LDS, no barrier, no scratch.  The
 * combine kernel: one wave per (head, row), four rows to a 256-thread workgroup; the wave reads rowPtrs and returns where
 * S' = 1; otherwise every lane forms M, the weights and l from the S' state pairs (same-address loads, no LDS), and streams
 * its 4 columns of the O_s as 16-byte loads, s ascending; 64 lanes x 4 columns cover Dv <= 256.  It stores a lane's 4 columns
 * at once where the partial kernel ran 16-byte lanes, element by element otherwise.
 * mispmm_last_kernel(): the partial launch notes attn_csr_split<f32|bf16,G8|G16|G32|G64,V4|V8|V1,C1|C2|C4,S<splits>> (G, V, C
 * as in the one-launch kernels), then the combine launch notes attn_csr_combine<f32|bf16,S<splits>> (the type of out), which
 * is what is read after the call.  mispmm_attn_csr_split_last_partial() returns the partial launch's note of the calling
 * thread's last call that launched ("" before the first): what names the instance that ran. */
uint64_t mispmm_attn_csr_split_workspace(uint32_t H, uint32_t M, uint32_t Dv, uint32_t splits);

const char *mispmm_attn_csr_split_last_partial(void);

int mispmm_attn_csr_split_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                              const uint32_t *colIdxs, const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat,
                              uint64_t k_head_stride, uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv,
                              uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, float *out,
                              uint64_t out_head_stride, uint32_t ldo, float *lse, uint32_t splits, uint32_t min_batches, void *workspace,
                              uint64_t workspace_bytes);

int mispmm_attn_csr_split_bf16(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                               const uint32_t *colIdxs, const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat,
                               uint64_t k_head_stride, uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv,
                               uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, void *out,
                               uint64_t out_head_stride, uint32_t ldo, int out_bf16, float *lse, uint32_t splits, uint32_t min_batches,
                               void *workspace, uint64_t workspace_bytes);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_CSR_SPLIT_H */
