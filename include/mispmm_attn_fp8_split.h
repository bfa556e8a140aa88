/* mispmm_attn_fp8_split.h -- C ABI of libmispmm_attn_fp8_split.so: the fused block-sparse attention forward with Q, K and V in
 * fp8 (OCP e4m3) with every block row SPLIT over several waves and K / V heads SHARED by groups of query heads, for AMD CDNA4
 * (gfx950).
 *
 * A sixteenth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's.  Conventions as in mispmm.h: device pointers, row-major dense operands, a call only
 * enqueues on `stream`, and every argument is validated before any device work.
 */
#ifndef MISPMM_ATTN_FP8_SPLIT_H
#define MISPMM_ATTN_FP8_SPLIT_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Fused attention on a BSR pattern, e4m3, block rows split, KV heads shared */
/* What mispmm_attn_bsr_fp8 (mispmm_attn_fp8.h) computes -- the same operands, limits, alignment, special values and layout of
 * out and lse; read that header for them -- for the shapes an fp8 KV cache is read at: few query rows, very many keys, several
 * query heads over fewer K / V heads.  This header states only what differs.  TWO launches on `stream`: a partial kernel in
 * which (head, 16-row unit, segment) is one wave, and a combine kernel.
 * SHARED KV HEADS.  kv_group >= 1 divides H.  Query head h reads K and V of KV head h / kv_group: Kmat + (h / kv_group) * k_head
 * and V + (h / kv_group) * v_head, so Kmat and V hold H / kv_group heads.  q_scale holds H elements; k_scale and v_scale hold
 * H / kv_group elements and are read at h / kv_group:
 *   c_h = fl(fl(scale * q_scale[h]) * k_scale[h / kv_group]).
 * kv_group = 1 is the contract of mispmm_attn_bsr_fp8.
 * SEGMENTS are exactly those of mispmm_attn_split.h.  A block row of n steps, n = ceil(blocks / E), E = 2 blocks at bS = 16 and 1
 * at bS = 32 (a step is 32 keys), is cut at whole steps: segment s of S = `splits` walks steps floor(s n / S) ..
 * floor((s + 1) n / S) - 1 in storage order, computed in the kernels from blockRowPtrs without a 64-bit product.  A segment
 * without steps (n < S) writes nothing and its workspace is never read.  Only the row's true last step can be a half step at
 * bS = 16.
 * THE PARTIAL KERNEL.  Inside its steps a wave does exactly what the wave of mispmm_attn_bsr_fp8 does (its ALGORITHM): the same
 * z, the weights as e4m3 of fl(2^8 w), l from the rounded scaled weights read back, lx from the unrounded ones, the (tx - tx)
 * poison term, the four lanes of a row meeting as (g0 + g1) + (g2 + g3).  It stores per row m_s, l_s, lx_s and the fp32
 * accumulator O_s, unnormalised and not multiplied by v_scale.
 * THE MERGE, per matrix row, over the row's non-empty segments with s ascending -- steps 1 to 6 of mispmm_attn_split.h:
 *   1. M = fmax over the m_s (a NaN is dropped, as in the loop: no m_s is one).
 *   2. mu = 0 if |M| = Inf, else M; mu_s likewise from m_s.
 *   3. w_s = 1 if m_s = -Inf, else exp(mu_s - mu) by v_exp_f32 of fl(t * log2 e), as every exponential of the loop.
 *   4. l = sum w_s l_s, lx = sum w_s lx_s, O = sum w_s O_s: fp32 products and sums, s ascending, each sum STARTING FROM ITS
 *      FIRST TERM and not from zero, so a -0 survives.
 *   5. out = fl(fl(O * fl(1 / l)) * v_scale[h / kv_group]): two separate multiplies, a NULL v_scale is no multiply; rounded
 *      once (to nearest even) if bf16; lse = mu + logf(lx).
 *   6. A block row with no blocks: +0 in its rows of out whatever v_scale holds, and lse = -Inf.
 * Consequences.  splits = 1 with kv_group = 1 gives the bits of mispmm_attn_bsr_fp8: the merge of one term is the identity
 * (w = 2^0 = 1).  out stays a convex combination of V's rows up to fp32 rounding: numerator and divisor carry the same w_s and
 * the same rounded weights, so a column of V that is constant over the row's keys comes back to (L + 16 + 2 S) 2^-24 relative.
 * A segment whose keys are all masked has m_s = -Inf, l_s = lx_s = 0 and O_s = 0 and contributes exactly nothing.  Every sum
 * has a fixed order and there are no atomics: the same S gives the same bits run to run, independent of H and the strides.
 * Against S = 1 a merged term passes one more product and at most S - 1 more additions on numerator and divisor alike: the
 * bounds NUMERICS of mispmm_attn_fp8.h states for out and lse hold with (L + 8 T + 16) become (L + 8 T + 16 + 2 S).
 * WORKSPACE.  mispmm_attn_bsr_fp8_split_workspace() bytes = 4 * H * numBlockRows * bS * splits * (Dv + 3), 16-byte aligned,
 * fp32, the layout of mispmm_attn_split.h: with units = numBlockRows * bS / 16 and item = (h * units + unit) * splits + s, first
 * O as [items][16 rows][Dv], then the states as [items][3][16 rows] = m, l, lx.  Contents are scratch: nothing is kept between
 * calls, nothing need be cleared.  The call neither allocates nor synchronises, so it can be captured into a graph.
 * REFUSALS, before any device work, in this order, each with its message in mispmm_last_error(): bS; scale; D or Dv not a
 * multiple of 8 in 8 .. 128; K not a multiple of bS; D not a multiple of 16 (those of mispmm_attn_bsr_fp8, in its order); then
 * kv_group == 0 or H % kv_group != 0: MISPMM_ERR_INVALID_ARG; splits 0 or above 64: MISPMM_ERR_INVALID_ARG; a null,
 * misaligned or too small workspace: MISPMM_ERR_INVALID_ARG, the message names the bytes needed -- then H == 0 or
 * numBlockRows == 0 is a no-op -- then, as mispmm_attn_bsr_fp8: a null pointer; a leading dimension below its width; alignment
 * of operands and strides; alignment of the scales; a head that spans 2 GiB or more; more work units than one launch takes,
 * now units * splits per head.
 * Work split: 4 waves to a workgroup, the items of a head numbered unit * splits + s, so a workgroup holds consecutive
 * segments of one unit: disjoint K / V panels, Q shared through L1.  The workgroups run in XCD order over (KV head, workgroup
 * of a head, query head of the group): the query heads of one KV group are adjacent, the panel one of them pulls into L2 is
 * the one its neighbours read next.  No LDS, no barrier, no scratch in the partial kernel.  The combine kernel: 256 threads
 * take 8 rows; wave 0 lists the non-empty segments, the states go through LDS, one thread per row forms the weights, then every
 * thread streams a run of 4 columns of the O_s as 16-byte loads.
 * mispmm_last_kernel(): the partial launch notes attn_bsr_fp8_split<b16|b32,mask|nomask,D1|D2,T4|T8,S<splits>> (D<n>, T<n> as
 * in mispmm_attn_fp8.h), then the combine launch notes attn_bsr_fp8_combine<f32|bf16,S<splits>>, which is what is read after
 * the call. */
uint64_t mispmm_attn_bsr_fp8_split_workspace(uint32_t H, uint32_t numBlockRows, uint32_t bS, uint32_t Dv, uint32_t splits);

int mispmm_attn_bsr_fp8_split(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                              const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint8_t *Q, uint32_t ldq, uint64_t q_head,
                              const uint8_t *Kmat, uint32_t ldk, uint64_t k_head, const uint8_t *V, uint32_t ldv, uint64_t v_head,
                              uint32_t D, uint32_t Dv, const float *mask, float scale, const float *q_scale, const float *k_scale,
                              const float *v_scale, void *out, uint32_t ldo, uint64_t o_head, int out_bf16, float *lse, uint32_t kv_group,
                              uint32_t splits, void *workspace, uint64_t workspace_bytes);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_FP8_SPLIT_H */
