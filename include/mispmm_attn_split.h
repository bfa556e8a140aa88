/* mispmm_attn_split.h -- C ABI of libmispmm_attn_split.so: the fused block-sparse attention forward in bf16 with every block
 * row SPLIT over several waves, for AMD CDNA4 (gfx950).
 *
 * A library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's.  Conventions as in mispmm.h: device pointers, row-major dense operands, a call only
 * enqueues on `stream`, and every argument is validated before any device work.
 */
#ifndef MISPMM_ATTN_SPLIT_H
#define MISPMM_ATTN_SPLIT_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Fused attention on a BSR pattern, bf16, block rows split over waves */
/* What mispmm_attn_bsr_bf16 (mispmm_attn.h) computes -- the same operands, limits, special values and layout of out and lse;
 * read that header for them -- for the shapes where one wave per 16 rows leaves the card idle: few rows and very many keys
 * (decoding, chunked prefill against a long context), or one head of a ragged pattern whose longest row decides the tail.
 * TWO launches on `stream`: a partial kernel in which (head, 16-row unit, segment) is one wave, and a combine kernel.
 * SEGMENTS.  A block row of n steps, n = ceil(blocks / E), E = 2 blocks at bS = 16 and 1 at bS = 32 (a step is 32 keys), is
 * cut at whole steps: segment s of S = `splits` walks steps floor(s n / S) .. floor((s + 1) n / S) - 1 in storage order.  The
 * kernels compute this from blockRowPtrs; the host does not read the pattern.  A segment without steps (n < S) does no work,
 * writes nothing, and its workspace is never read.  Inside its steps a wave does exactly what the one-wave kernel does (the
 * ALGORITHM of mispmm_attn.h: the same z, the same bf16 rounding of the weights, l from the rounded and lx from the unrounded
 * weights, the four lanes of a row meeting as (g0 + g1) + (g2 + g3)) and stores its state unnormalised: per row the running
 * maximum m_s, l_s, lx_s and the fp32 accumulator O_s.
 * THE MERGE, per matrix row, over the row's non-empty segments with s ascending:
 *   1. M = fmax over the m_s (a NaN is dropped, as in the loop: no m_s is one).
 *   2. mu = 0 if |M| = Inf, else M; mu_s likewise from m_s.
 *   3. w_s = 1 if m_s = -Inf, else exp(mu_s - mu) by v_exp_f32 of fl(t * log2 e), as every exponential of the loop.
 *   4. l = sum w_s l_s, lx = sum w_s lx_s, O = sum w_s O_s: fp32 products and sums, s ascending, each sum STARTING FROM ITS
 *      FIRST TERM and not from zero, so a -0 survives.
 *   5. out = O * fl(1 / l), rounded once (to nearest even) if bf16; lse = mu + logf(lx).
 *   6. A block row with no blocks: +0 in its rows of out and lse = -Inf.
 * Consequences.  splits = 1 gives the bits of mispmm_attn_bsr_bf16: the merge of one term is the identity (w = 2^0 = 1).  The
 * special values are that kernel's: a row that holds a NaN, a +Inf or nothing but -Inf is NaN in every element of out of that
 * row and of no other, with lse NaN, +Inf, -Inf; a masked key contributes +0.  A segment whose keys are all masked has
 * m_s = -Inf, l_s = lx_s = 0 and O_s = 0 and contributes exactly nothing.  Every sum has a fixed order and there are no
 * atomics: every run gives the same bits for the same S, independent of H and of the strides.  Different S give different
 * roundings of the same quantities: against S = 1 a term passes at most S more fp32 products and additions, S 2^-24 relative
 * on numerator and divisor alike, inside the bounds NUMERICS of mispmm_attn.h states for out and lse.
 * WORKSPACE.  mispmm_attn_bsr_split_workspace() bytes = 4 * H * numBlockRows * bS * splits * (Dv + 3), 16-byte aligned, fp32.
 * With units = numBlockRows * bS / 16 and item = (h * units + unit) * splits + s: first O as [items][16 rows][Dv], then the
 * states as [items][3][16 rows] = m, l, lx.  Contents are scratch: nothing is kept between calls, nothing need be cleared.
 * It grows with splits; the call neither allocates nor synchronises, so it can be captured into a graph.
 * REFUSALS, before any device work, each with its message in mispmm_last_error(): everything mispmm_attn_bsr_bf16 refuses
 * (shape, scale, null pointers, leading dimensions, alignment, 2 GiB spans, more work items than one launch takes -- now
 * units * splits per head); splits 0 or above 64: MISPMM_ERR_INVALID_ARG; a null, misaligned or too small workspace:
 * MISPMM_ERR_INVALID_ARG, the message names the bytes needed.  H == 0 or numBlockRows == 0: a no-op (after the checks of bS,
 * scale, D, Dv, K and splits).
 * Work split: 4 waves to a workgroup, the items of a head numbered unit * splits + s, so a workgroup holds consecutive
 * segments of one unit: disjoint K / V panels, Q shared through L1.  No LDS, no barrier, no scratch in the partial kernel.  The
 * combine kernel: 256 threads take 8 rows; wave 0 lists the non-empty segments, the states go through LDS, one thread per row
 * forms the weights, then every thread streams a run of 4 columns of the O_s as 16-byte loads.
 * mispmm_last_kernel(): the partial launch notes attn_bsr_split<b16|b32,mask|nomask,D2|D4,T4|T8,S<splits>> (D<n>, T<n> as in
 * mispmm_attn.h), then the combine launch notes attn_bsr_combine<f32|bf16,S<splits>>, which is what is read after the call. */
uint64_t mispmm_attn_bsr_split_workspace(uint32_t H, uint32_t numBlockRows, uint32_t bS, uint32_t Dv, uint32_t splits);

int mispmm_attn_bsr_split_bf16(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                               const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint16_t *Q, uint32_t ldq, uint64_t q_head,
                               const uint16_t *Kmat, uint32_t ldk, uint64_t k_head, const uint16_t *V, uint32_t ldv, uint64_t v_head,
                               uint32_t D, uint32_t Dv, const float *mask, float scale, void *out, uint32_t ldo, uint64_t o_head,
                               int out_bf16, float *lse, uint32_t splits, void *workspace, uint64_t workspace_bytes);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_SPLIT_H */
