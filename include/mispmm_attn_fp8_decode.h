/* mispmm_attn_fp8_decode.h -- C ABI of libmispmm_attn_fp8_decode.so: DECODE attention on a paged fp8 (OCP e4m3) KV cache -- one
 * query token per sequence, H query heads over H / kv_group K / V heads, each sequence with its own list of cache pages -- with
 * the query heads of a KV group PACKED into one MFMA tile, for AMD CDNA4 (gfx950).
 *
 * A seventeenth library beside libmispmm.so (mispmm.h), which it links: status codes, mispmm_stream_t, mispmm_last_error() and
 * mispmm_last_kernel() are that library's.  Conventions as in mispmm.h: device pointers, row-major dense operands, a call only
 * enqueues on `stream`, and every argument is validated before any device work.
 */
#ifndef MISPMM_ATTN_FP8_DECODE_H
#define MISPMM_ATTN_FP8_DECODE_H

#include "mispmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------ Decode attention on a paged KV cache, Q, K and V in e4m3, a KV group per tile */
/* What mispmm_attn_bsr_fp8_split (mispmm_attn_fp8_split.h) computes for a query row, for the shape an fp8 KV cache is read at
 * most often.  mispmm_attn_fp8.h states the arithmetic (ALGORITHM, SPECIAL VALUES, NUMERICS) and mispmm_attn_fp8_split.h the
 * segments and the merge; this header states what differs.  TWO launches on `stream`: a partial kernel in which (sequence, KV
 * head, segment) is one wave, and a combine kernel.
 * OPERANDS.  B sequences, H query heads, kv_group = G with 1 <= G <= 16 dividing H, Hkv = H / G KV heads.
 * pagePtrs [B + 1], pageIdxs [numPages]: uint32.  The keys of sequence b are, in order, the bS rows of each page
 * pageIdxs[pagePtrs[b] .. pagePtrs[b + 1]); page p is rows p * bS .. p * bS + bS - 1 of Kmat and V, bS 16 or 32 -- the arrays a
 * BSR pattern with one block row per sequence holds as blockRowPtrs / blockColIdxs.  Two sequences may list the same page (a
 * shared prefix).  K is the number of cache rows, a multiple of bS; a page at or past K / bS reads zeros for K and V.
 * seqLens [B]: uint32, or NULL.  NULL: every listed page is full.  Otherwise len_b = min(seqLens[b], pages_b * bS) (a device
 * array cannot be validated on the host) and the keys at positions >= len_b of the sequence's key order are MASKED; seqLens[b]
 * = 0 is a sequence without keys.  This replaces the block mask of the other fp8 attention entries: there is no other mask.
 * Every listed page is walked, so list the pages that hold keys: ceil(len_b / bS) of them.
 * Q: e4m3 bytes, element (b, h, :D) at Q + b * ldq + h * q_head.  Kmat, V: as in mispmm_attn_bsr_fp8_split: Hkv heads, row
 * strides ldk / ldv, head strides k_head / v_head (elements = bytes); a cache stored [pages][bS][Hkv][D] is a permuted view of
 * this.  out: element (b, h, :Dv) at out + b * ldo + h * o_head, fp32, or raw bf16 bits with out_bf16.  lse: fp32 [B][H]
 * contiguous, or NULL.  q_scale [H], k_scale [Hkv], v_scale [Hkv]: fp32 device arrays, each nullable, the caller's contract of
 * mispmm_attn_fp8.h.  D a multiple of 16 and Dv of 8, both up to 128; the alignments of mispmm_attn_fp8.h: Q, Kmat and out
 * 16-byte aligned with ldq, ldk, q_head, k_head multiples of 16; V 8-byte with ldv, v_head multiples of 8; ldo and o_head
 * multiples of 4 (bf16: 8); the scales 4-byte aligned.
 * RESULT.  Per (b, h), with kvh = h / G, exactly what mispmm_attn_fp8.h defines for ONE query row of head h against the
 * sequence's unmasked keys of KV head kvh: c_h = fl(fl(scale * q_scale[h]) * k_scale[kvh]) (a NULL scale is no multiply),
 * z = c_h * s (the fp32 product), the weights into the second product as e4m3 of fl(2^8 w), l from the rounded weights read
 * back, lx from the unrounded ones, the (tx - tx) poison term, out = fl(fl(O * fl(1 / l)) * v_scale[kvh]), lse = mu + logf(lx).
 * A sequence WITHOUT unmasked keys (no pages, or len_b = 0) gives +0 in out[b, :, :Dv] whatever v_scale holds and lse = -Inf.
 * SEGMENTS AND THE MERGE are those of mispmm_attn_split.h / mispmm_attn_fp8_split.h, word for word: a sequence of
 * n = ceil(pages_b / E) 32-key steps (E = 2 pages at bS = 16, 1 at bS = 32) is cut at whole steps, segment s of S = `splits`
 * (1 .. 64) walks steps floor(s n / S) .. floor((s + 1) n / S) - 1; a segment without steps writes nothing; the segments'
 * states are merged with s ascending, each sum starting from its first term (steps 1 to 5 of THE MERGE there).
 * TWO CONSEQUENCES.
 *   1. The bytes behind a masked key are never looked at: out and lse do not depend on the bytes of Kmat or V at positions
 *      >= len_b, NaN bytes included (a cache page's tail is uninitialised memory).  A masked score is REPLACED by -Inf with a
 *      select, nothing is added to it, and the V rows of masked keys enter the second product as zero bytes.  Only a step that
 *      holds a masked key (step_end > len_b, a wave-uniform condition) takes that path; a full step pays one scalar compare.
 *   2. Packing changes no bit.  A query row's arithmetic in the transposed score product does not look at the other 15 rows
 *      of its tile, so (b, h) has the bits of mispmm_attn_bsr_fp8_split called with the same splits and kv_group on the
 *      pattern with one block row per sequence, the token's q in one row of the block row, a block mask of 0 / -Inf at the
 *      tail and finite bytes behind it: fma(c, s, 0) and c * s round alike, and a -0 score does not change an exponential.
 *      (A sequence with pages and len_b = 0 is the one exception: there that call gives NaN, this one +0.)
 * NUMERICS.  The bounds of mispmm_attn_fp8.h hold per (b, h) with the (L + 8 T + 16 + 2 S) term of mispmm_attn_fp8_split.h, L
 * the sequence's unmasked keys (nv counts the steps that hold one).
 * WORKSPACE.  mispmm_attn_decode_fp8_workspace() bytes = 4 * B * H * splits * (Dv + 3), 16-byte aligned, fp32: sized by the G
 * REAL rows of a tile, not by 16 (a lane's stores are runs of 4 or 8 floats of one row from a column that is a multiple of as
 * many, and Dv is a multiple of 8: 16-byte runs either way).  kv_group does not enter the size.  With item = (b * Hkv + kvh) *
 * splits + s: first O as [items][G rows][Dv], then the states as [items][3][G rows] = m, l, lx, unnormalised and not multiplied
 * by v_scale.  Contents are scratch: nothing is kept between calls, nothing need be cleared.  The call neither allocates nor
 * synchronises, so it can be captured into a graph.
 * REFUSALS, before any device work, in this order, each with its message in mispmm_last_error(): bS; scale; D or Dv not a
 * multiple of 8 in 8 .. 128; K not a multiple of bS; D not a multiple of 16 (those of mispmm_attn_bsr_fp8, in its order); then
 * kv_group == 0: MISPMM_ERR_INVALID_ARG, kv_group > 16: MISPMM_ERR_UNSUPPORTED, H % kv_group != 0: MISPMM_ERR_INVALID_ARG;
 * splits 0 or above 64: MISPMM_ERR_INVALID_ARG; a null, misaligned or too small workspace: MISPMM_ERR_INVALID_ARG, the message
 * names the bytes needed -- then B == 0 or H == 0 is a no-op -- then a null pointer (pageIdxs may be null when numPages == 0;
 * seqLens, lse and the scales may be null); a leading dimension below its width; alignment of operands and strides; alignment
 * of the scales; the G heads of a KV group of Q, or one head of Kmat or V, spanning 2 GiB or more; more work units than one
 * launch takes (B * splits per KV head, or numPages * bS past 2^32).
 * Work split.  One wave owns (sequence, KV head, segment): lane (i, g) of the transposed score product holds query head
 * kvh * G + i of the token -- lanes with i >= G hold zeros and store nothing -- so K and V are read, transposed and multiplied
 * once per KV head, not once per query head.  4 waves to a workgroup, consecutive segments of one (sequence, KV head); the
 * workgroups run in XCD order over (KV head, sequence, segment), sequences inside a KV head: sequences that share prefix pages
 * read the same K / V panel of that head and are neighbours on one XCD.  No LDS, no barrier, no atomics, no scratch in the
 * partial kernel.  The combine kernel: 256 threads take 8 (b, h) rows, 32 threads each; a ballot lists a row's non-empty
 * segments, the states go through LDS, one thread per row forms the weights, then every thread streams 4 columns of the O_s.
 * mispmm_last_kernel(): the partial launch notes attn_decode_fp8<b16|b32,len|full,D1|D2,T4|T8,S<splits>> (len: seqLens given;
 * D<n>, T<n> as in mispmm_attn_fp8.h), then the combine launch notes attn_decode_fp8_combine<f32|bf16,S<splits>>, which is what
 * is read after the call. */
uint64_t mispmm_attn_decode_fp8_workspace(uint32_t B, uint32_t H, uint32_t kv_group, uint32_t Dv, uint32_t splits);

int mispmm_attn_decode_fp8(mispmm_stream_t stream, uint32_t B, uint32_t H, uint32_t K, uint32_t bS, uint32_t numPages,
                           const uint32_t *pagePtrs, const uint32_t *pageIdxs, const uint32_t *seqLens, const uint8_t *Q, uint32_t ldq,
                           uint64_t q_head, const uint8_t *Kmat, uint32_t ldk, uint64_t k_head, const uint8_t *V, uint32_t ldv,
                           uint64_t v_head, uint32_t D, uint32_t Dv, float scale, const float *q_scale, const float *k_scale,
                           const float *v_scale, void *out, uint32_t ldo, uint64_t o_head, int out_bf16, float *lse, uint32_t kv_group,
                           uint32_t splits, void *workspace, uint64_t workspace_bytes);

#ifdef __cplusplus
}
#endif

#endif /* MISPMM_ATTN_FP8_DECODE_H */
