// libmispmm_attn_csr_split.so: the fused attention forward on a CSR pattern with every LONG ROW SPLIT over several lane groups
// (include/mispmm_attn_csr_split.h), fp32 and bf16 operands from one unit -- the forward of ../attn_csr_fwd.hpp with the batches
// of a row dealt to up to `splits` lane groups, and a second launch that merges their online-softmax states.  The one-launch
// forward gives a (head, row) to one lane group that walks the whole row, one dependent batch after another: a long row sets the
// launch's tail and few long rows (decoding, chunked prefill) leave the card idle.  Here (head, row, segment) is the work item.
//
// PARTIAL KERNEL.  Lane group, butterfly, dropped loads, element policy: ../lane_group.hpp and ../elem.hpp.  A row of n batches
// is cut at whole batches into S' = min(splits, max(1, n / min_batches)) segments, segment s walking batches floor(s n / S') ..
// floor((s + 1) n / S') - 1, computed here from rowPtrs.  The items of a head are numbered row * splits + s: the groups of a
// workgroup are consecutive segments of one row (disjoint K and V rows, Q[r] shared through L1); a group with s >= S' leaves at
// once.  Inside its entries [base, base + len) the group IS the one-launch kernel on a row [base, base + len): the loop below is
// ../attn_csr_fwd.hpp's, spelled a second time on purpose -- shared through a helper it moves the forward's ISA (lane_group.hpp's
// header) -- with the row's bounds replaced by the segment's.  So a slot or a fetch past the segment's end re-reads the
// segment's first entry: never past the row, and only a row's true last segment ends in a partial batch.
// The ending: S' == 1 -- the group stores out and lse itself, the forward's own store (O / l, mu + logf(l)), and the workspace is
// not touched; S' > 1 -- it stores its state UNNORMALISED: O_s (the lanes' columns) and (m_s, l_s) by lane 0.
//
// WORKSPACE (floats).  slot = (h * M + row) * splits + s.  O: [slots][Dvp] from the start, Dvp = Dv rounded up to 4; then the
// states: [slots][2] = m, l.  Slots of s >= S' and of rows with S' == 1 are neither written nor read.
//
// COMBINE KERNEL.  Plain VALU, bandwidth-bound.  One wave per (head, row), four rows to a 256-thread workgroup.  The wave reads
// rowPtrs and leaves where S' == 1.  Otherwise EVERY lane forms M, then the weights and l from the S' state pairs (same-address
// loads: no LDS, no cross-lane move), and streams its 4 columns of the O_s as 16-byte loads, s ascending, every sum starting from
// its first term; then O / l per element and lse by lane 0.  Columns Dv .. Dvp - 1 of a slot may never have been written: a lane
// computes on them and stores none of them.
#include "../attn_csr_entry.hpp"
#include "mispmm_attn_csr_split.h"

namespace mispmm {

namespace {

constexpr uint32_t kMaxSplits = 256;
constexpr int kCombineRows = 4;  // rows to a workgroup of the combine kernel, one wave each

// the partial launch's note of this thread's last call: the combine's note replaces it in mispmm_last_kernel()
thread_local char g_partial_tag[96] = "";

// what both kernels need beyond the forward's block
struct SplitExtra {
    uint32_t splits, min_batches, Dvp;
};

// segments of a row of n batches: every one holds at least min_batches batches, a short row has one
__device__ __forceinline__ uint32_t seg_count(uint32_t n, const SplitExtra &x) {
    const uint32_t fit = n / x.min_batches;
    return fit < 1u ? 1u : (fit < x.splits ? fit : x.splits);
}
// first batch of segment s of a row of n = q * S + r batches: floor(s n / S) without a 64-bit product (s, r <= 256)
__device__ __forceinline__ uint32_t seg_start(uint32_t s, uint32_t q, uint32_t r, uint32_t S) { return s * q + s * r / S; }

template <class Elem, int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_split_kernel(const FwdParams<Elem> p, const SplitExtra x, const uint32_t *__restrict__ rowPtrs,
                                                                  const uint32_t *__restrict__ colIdxs, const typename Elem::in_t *__restrict__ Q,
                                                                  const typename Elem::in_t *__restrict__ K,
                                                                  const typename Elem::in_t *__restrict__ V, const float *__restrict__ bias,
                                                                  typename Elem::out_t *__restrict__ out, float *__restrict__ lse_out,
                                                                  float *__restrict__ ws_o, float *__restrict__ ws_state) {
    using raw_t = typename Elem::template raw_t<VEC>;
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scores sit in the first lanes of a group");
    static_assert(Elem::template fits<G, VEC, NCH>, "no such lane width or chunk count for this element type");
    constexpr int GROUPS = kLgBlock / G, E = kLgBatch;
    constexpr uint32_t CHUNK = G * VEC;
    const uint32_t lane = threadIdx.x % G, sub = lane & (E - 1);
    const uint32_t item = xcd_block(blockIdx.x, p.xcd_chunk);
    if (item >= p.total) return;
    const uint32_t h = item / p.blocks_per_head;  // wave-uniform: a workgroup lies inside one head
    const uint64_t idx64 = static_cast<uint64_t>(item - h * p.blocks_per_head) * GROUPS + threadIdx.x / G;
    if (idx64 >= static_cast<uint64_t>(p.M) * x.splits) return;  // the lanes a move reads from are all in the lane's own group
    const uint32_t idx = static_cast<uint32_t>(idx64);  // M * splits < 2^32 (the entry point)
    const uint32_t row = idx / x.splits, seg = idx - row * x.splits;
    const uint32_t row_base = rowPtrs[row];
    const uint32_t row_len = rowPtrs[row + 1] - row_base;
    const uint32_t n = (row_len + E - 1) / E, S = seg_count(n, x);
    if (seg >= S) return;
    const uint32_t nq = n / S, nr = n - nq * S;
    const uint32_t lo = seg_start(seg, nq, nr, S) * E, hi = seg_start(seg + 1, nq, nr, S) * E;
    // the segment as a row of its own; hi > row_len only in the row's last segment (and lo < row_len wherever n > 0)
    const uint32_t base = row_base + lo;
    const uint32_t len = (hi < row_len ? hi : row_len) - lo;
    const float ninf = -__builtin_huge_valf();

    const typename Elem::row_t out_row = Elem::row_of(out, h, p.o_head, row, p.ldo);
    float o[NCH][VEC];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[c][v] = 0.f;
    // the forward's store: the lane's columns of chunk c are inside Dv or past it together
    auto store = [&](float l, float lse) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t col = c * CHUNK + lane * VEC;
            if (col >= p.Dv) continue;
            float r[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) r[v] = o[c][v] / l;
            if (p.narrow) {  // wave-uniform, and never for fp32 operands; the fp32 quotient rounded once
                if constexpr (Elem::kWidens) store_bf16<VEC>(Elem::template ptr<uint16_t>(out, out_row) + col, r);
            } else {
                store_f32<VEC>(Elem::template ptr<float>(out, out_row) + col, r);
            }
        }
        if (lse_out && lane == 0) lse_out[static_cast<size_t>(h) * p.M + row] = lse;
    };
    if (row_len == 0) {  // an empty row (S == 1, seg == 0): +0 / 1 and lse = log 0
        store(1.f, ninf);
        return;
    }

    const rsrc_t qr = make_rsrc(Q + h * p.q_head, p.q_bytes), kr = make_rsrc(K + h * p.k_head, p.k_bytes);
    const rsrc_t vr = make_rsrc(V + h * p.v_head, p.v_bytes);
    const rsrc_t br = make_rsrc(bias ? bias + h * p.bias_head : nullptr, p.bias_bytes);  // spans nothing without a bias: reads give +0
    uint32_t koff[NCH], voff[NCH];
    typename Elem::template held_t<VEC> xq[NCH];  // Q[r]'s slice
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        koff[c] = Elem::template lane_off<G, VEC>(lane, c, p.D);
        voff[c] = Elem::template lane_off<G, VEC>(lane, c, p.Dv);
        const raw_t qraw = Elem::template load<VEC>(qr, join_off(p.q_row(row), koff[c]));  // past D: zeros
        if constexpr (Elem::kWidens) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) xq[c][v] = Elem::template at<VEC>(qraw, v);
        } else {
            xq[c] = qraw;
        }
    }
    // entry c0 + sub of the segment and its bias; a slot past the segment's end re-reads the segment's first entry (len > 0)
    auto fetch = [&](uint32_t c0, uint32_t &col, float &b) {
        const uint32_t idx = c0 + sub;
        const uint32_t e = base + (idx < len ? idx : 0u);
        col = colIdxs[e];
        b = buffer_load_vec<1>(br, e * 4u, 0);
    };
    uint32_t nxt_col;
    float nxt_bias;
    fetch(0, nxt_col, nxt_bias);
    float m = ninf, mu = 0.f, l = 0.f;
    // the batch of ../attn_csr_fwd.hpp, operation for operation (its comments say why each line stands where it does)
    for (uint32_t s0 = 0; s0 < len; s0 += E) {
        const bool live = s0 + sub < len;
        const uint32_t dead = live ? 0u : kDropLoad;
        const uint32_t kkey = nxt_col * p.ldk | dead;
        const uint32_t vkey = nxt_col * p.ldv | dead;
        const float b = nxt_bias;
        fetch(s0 + E, nxt_col, nxt_bias);  // on its way while this batch is gathered
        __builtin_amdgcn_sched_barrier(0);
        raw_t kv[E][NCH], vv[E][NCH];
        Elem::template gather<VEC, NCH>(kkey, kr, koff, kv);
        Elem::template gather<VEC, NCH>(vkey, vr, voff, vv);
        float acc[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    acc[j] = __builtin_fmaf(Elem::template held<VEC>(xq[c], v), Elem::template at<VEC>(kv[j][c], v), acc[j]);
        }
        const float s = transpose_sum<G>(acc, lane);
        const float z = live ? __builtin_fmaf(p.scale, s, b) : ninf;
        float mx = z;
        mx = __builtin_fmaxf(mx, lane_xor<1>(mx));  // drops a NaN operand: the weight carries it
        mx = __builtin_fmaxf(mx, lane_xor<2>(mx));
        mx = __builtin_fmaxf(mx, lane_xor<4>(mx));
        const float m_new = __builtin_fmaxf(m, mx);
        const float mu_new = __builtin_fabsf(m_new) == __builtin_huge_valf() ? 0.f : m_new;
        const float alpha = m == ninf ? 1.f : lg_exp(mu - mu_new);
        m = m_new;
        mu = mu_new;
        const float w = lg_exp(z - mu);
        float t = w + lane_xor<1>(w);
        t = t + lane_xor<2>(t);
        t = t + lane_xor<4>(t);
        l = l * alpha;
        l = l + t;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) o[c][v] = o[c][v] * alpha;
        static_for<0, E>([&](auto j_tag) {
            constexpr int j = decltype(j_tag)::value;
            const float wj = __uint_as_float(group_bcast<8, j>(__float_as_uint(w)));
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v) o[c][v] = __builtin_fmaf(wj, Elem::template at<VEC>(vv[j][c], v), o[c][v]);
        });
        asm volatile("" : "+v"(nxt_col), "+v"(nxt_bias));
    }
    if (S == 1) {  // the whole row: the forward's ending
        store(l, mu + __builtin_logf(l));
        return;
    }
    const size_t slot = (static_cast<size_t>(h) * p.M + row) * x.splits + seg;
    float *o_to = ws_o + slot * x.Dvp;  // 16-byte aligned: Dvp is a multiple of 4
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t col = c * CHUNK + lane * VEC;
        if (col < p.Dv) store_f32<VEC>(o_to + col, o[c]);
    }
    if (lane == 0) {
        ws_state[slot * 2u] = m;
        ws_state[slot * 2u + 1u] = l;
    }
}

struct CombineParams {
    uint32_t M, Dv, ldo, wgs_per_head, wide;  // wide: 16-byte (fp32) or 8-byte (bf16) stores of a lane's 4 columns
    uint64_t o_head;                          // elements
    SplitExtra x;
};

template <bool OUT_BF16>
__global__ void __launch_bounds__(kWave * kCombineRows)
    attn_csr_combine_kernel(const CombineParams p, const uint32_t *__restrict__ rowPtrs, const float *__restrict__ ws_o,
                            const float *__restrict__ ws_state, void *__restrict__ out, float *__restrict__ lse_out) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const uint32_t h = blockIdx.x / p.wgs_per_head;
    const uint64_t row64 = static_cast<uint64_t>(blockIdx.x - h * p.wgs_per_head) * kCombineRows + wave;
    if (row64 >= p.M) return;
    const uint32_t row = static_cast<uint32_t>(row64);
    const uint32_t len = rowPtrs[row + 1] - rowPtrs[row];
    const uint32_t S = seg_count((len + kLgBatch - 1) / kLgBatch, p.x);
    if (S == 1) return;  // the partial kernel stored this row itself
    const float inf = __builtin_huge_valf();
    const size_t slot0 = (static_cast<size_t>(h) * p.M + row) * p.x.splits;
    const float *st = ws_state + slot0 * 2u;
    // the merge of the header, steps 1 to 4, in every lane alike
    float top = st[0];
    for (uint32_t s = 1; s < S; ++s) top = __builtin_fmaxf(top, st[2u * s]);
    const float mu = __builtin_fabsf(top) == inf ? 0.f : top;
    const uint32_t col = 4u * lane;
    const bool mine = col < p.x.Dvp;
    const float *src = ws_o + slot0 * p.x.Dvp + (mine ? col : 0u);
    float l = 0.f;
    f32x4 o{0.f, 0.f, 0.f, 0.f};
    for (uint32_t s = 0; s < S; ++s) {
        const float ms = st[2u * s];
        const float mus = __builtin_fabsf(ms) == inf ? 0.f : ms;
        const float w = ms == -inf ? 1.f : lg_exp(mus - mu);
        const float tl = w * st[2u * s + 1u];
        const f32x4 to = *reinterpret_cast<const f32x4 *>(src + static_cast<size_t>(s) * p.x.Dvp) * w;
        l = s == 0 ? tl : l + tl;
        o = s == 0 ? to : o + to;
    }
    if (lse_out && lane == 0) lse_out[static_cast<size_t>(h) * p.M + row] = mu + __builtin_logf(l);
    if (!mine) return;
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = o[i] / l;
    const size_t at = static_cast<size_t>(h) * p.o_head + static_cast<size_t>(row) * p.ldo + col;
    if constexpr (OUT_BF16) {
        uint16_t *to = static_cast<uint16_t *>(out) + at;
        if (p.wide) {  // Dv is a multiple of 8
            *reinterpret_cast<uint2 *>(to) = make_uint2(bf16_pair(r[0], r[1]), bf16_pair(r[2], r[3]));
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (col + i < p.Dv) to[i] = static_cast<uint16_t>(bf16_bits(r[i]));
        }
    } else {
        float *to = static_cast<float *>(out) + at;
        if (p.wide) {  // Dv is a multiple of 4
            store_vec<4>(to, f32x4{r[0], r[1], r[2], r[3]});
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (col + i < p.Dv) to[i] = r[i];
        }
    }
}

uint64_t workspace_bytes(uint32_t H, uint32_t M, uint32_t Dv, uint32_t splits) {
    const uint64_t dvp = (static_cast<uint64_t>(Dv) + 3u) & ~3ull;
    uint64_t slots, bytes;
    if (__builtin_mul_overflow(static_cast<uint64_t>(H) * M, static_cast<uint64_t>(splits), &slots) ||
        __builtin_mul_overflow(slots, 4u * (dvp + 2u), &bytes))
        return ~0ull;  // more than any buffer holds
    return bytes;
}

// fwd_entry of ../attn_csr_entry.hpp with the split's own refusals; `ename`: "f32" or "bf16" in the tags
template <class Elem>
int split_entry(const char *name, const char *ename, mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz,
                const uint32_t *rowPtrs, const uint32_t *colIdxs, const typename Elem::in_t *Q, uint64_t q_head_stride, uint32_t ldq,
                const typename Elem::in_t *Kmat, uint64_t k_head_stride, uint32_t ldk, uint32_t D, const typename Elem::in_t *V,
                uint64_t v_head_stride, uint32_t ldv, uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride,
                typename Elem::out_t *out, uint64_t out_head_stride, uint32_t ldo, int out_bf16, float *lse, uint32_t splits,
                uint32_t min_batches, void *workspace, uint64_t workspace_bytes_given) {
    constexpr uint64_t EB = Elem::kBytes, WIDE = Elem::kWide;
    if (const int st = refuse_shape(name, D, Dv, scale); st != MISPMM_OK) return st;
    if (splits == 0 || splits > kMaxSplits) return fail(MISPMM_ERR_INVALID_ARG, "%s: splits must be 1 to %u (got %u)", name, kMaxSplits, splits);
    if (min_batches == 0) return fail(MISPMM_ERR_INVALID_ARG, "%s: min_batches must be at least 1 (got 0)", name);
    if (H == 0 || M == 0) return MISPMM_OK;
    if (!rowPtrs || !Q || !Kmat || !V || !out || (nnz != 0 && !colIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: rowPtrs, colIdxs, Q, K, V or out is null", name);
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)", name, D,
                    ldq, ldk, Dv, ldv, ldo);
    const uint64_t o_elem = out_bf16 ? 2u : 4u;
    const uint64_t qs = span(M, ldq, D), ks = span(K, ldk, D), vs = span(K, ldv, Dv), os = span(M, ldo, Dv);
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) : 0u;
    if (over2g(EB, {qs, ks, vs}) || over2g(o_elem, {os}) || over2g(4, {bs}))
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: Q, K, V, out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu bytes)", name,
                    static_cast<ull>(qs * EB), static_cast<ull>(ks * EB), static_cast<ull>(vs * EB), static_cast<ull>(os * o_elem),
                    static_cast<ull>(bs * 4u));
    const bool wide = D % WIDE == 0 && Dv % WIDE == 0 && mult(ldq, WIDE) && mult(ldk, WIDE) && mult(ldv, WIDE) && mult(ldo, WIDE) &&
                      mult(q_head_stride, WIDE) && mult(k_head_stride, WIDE) && mult(v_head_stride, WIDE) && mult(out_head_stride, WIDE) &&
                      aligned16(Q) && aligned16(Kmat) && aligned16(V) && aligned16(out);
    const int vec = wide ? Elem::kWide : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    const uint64_t items = static_cast<uint64_t>(M) * splits;
    if (items > 0xFFFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: %u rows x %u splits are 2^32 work items of one head or more", name, M, splits);
    if (const int st = refuse_grid(name, static_cast<uint32_t>(items), H, g); st != MISPMM_OK) return st;
    if (const int st = refuse_grid(name, M, H, kLgBlock / kCombineRows); st != MISPMM_OK) return st;  // the combine launch
    if (EB == 2 && !(aligned2s({Q, Kmat, V}) && (!out_bf16 || aligned2(out))))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: Q, K, V and a bf16 out must be 2-byte aligned", name);
    const uint64_t need = workspace_bytes(H, M, Dv, splits);
    if (!workspace || !aligned16(workspace) || workspace_bytes_given < need)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: the workspace must be 16-byte aligned and hold %llu bytes (got %s, %llu bytes)", name,
                    static_cast<ull>(need), !workspace ? "null" : aligned16(workspace) ? "an aligned pointer" : "a misaligned pointer",
                    static_cast<ull>(workspace_bytes_given));
    FwdParams<Elem> p{};
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq = ldq * kFwdLdqUnit<Elem>, p.ldk = static_cast<uint32_t>(ldk * EB), p.ldv = static_cast<uint32_t>(ldv * EB), p.ldo = ldo;
    p.q_bytes = static_cast<uint32_t>(qs * EB), p.k_bytes = static_cast<uint32_t>(ks * EB), p.v_bytes = static_cast<uint32_t>(vs * EB);
    p.bias_bytes = static_cast<uint32_t>(bs * 4u);
    if constexpr (Elem::kWidens) p.narrow = out_bf16 ? 1u : 0u;
    p.scale = scale;
    p.q_head = q_head_stride, p.k_head = k_head_stride, p.v_head = v_head_stride, p.o_head = out_head_stride, p.bias_head = bias_head_stride;
    const SplitExtra x{splits, min_batches, (Dv + 3u) & ~3u};
    float *ws_o = static_cast<float *>(workspace);
    float *ws_state = ws_o + static_cast<uint64_t>(H) * items * x.Dvp;
    const hipStream_t s = as_stream(stream);
    Elem::with_instance(vec, g, width, [&](auto gr, auto v, auto ch) {
        constexpr int G = decltype(gr)::value, VEC = decltype(v)::value, NCH = decltype(ch)::value;
        const uint32_t grid = finish_grid<G>(p, static_cast<uint32_t>(items), H);
        snprintf(g_partial_tag, sizeof(g_partial_tag), "attn_csr_split<%s,G%d,V%d,C%d,S%u>", ename, G, VEC, NCH, splits);
        note_kernel("%s", g_partial_tag);
        hipLaunchKernelGGL((attn_csr_split_kernel<Elem, G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, s, p, x, rowPtrs, colIdxs, Q, Kmat, V, bias,
                           out, lse, ws_o, ws_state);
    });
    MISPMM_LAUNCH_CHECK();
    // a lane's 4 columns as one store: fp32 out under the operands' own wide rule, a bf16 out (8 bytes) under the bf16 one
    const CombineParams c{M, Dv, ldo, ceil_div(M, static_cast<uint32_t>(kCombineRows)), wide ? 1u : 0u, out_head_stride, x};
    with_flag(out_bf16 != 0, [&](auto ob) {
        note_kernel("attn_csr_combine<%s,S%u>", decltype(ob)::value ? "bf16" : "f32", splits);
        hipLaunchKernelGGL((attn_csr_combine_kernel<decltype(ob)::value>), dim3(c.wgs_per_head * H), dim3(kWave * kCombineRows), 0, s, c, rowPtrs,
                           ws_o, ws_state, out, lse);
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" uint64_t mispmm_attn_csr_split_workspace(uint32_t H, uint32_t M, uint32_t Dv, uint32_t splits) {
    return workspace_bytes(H, M, Dv, splits);
}

extern "C" const char *mispmm_attn_csr_split_last_partial(void) { return g_partial_tag; }

extern "C" int mispmm_attn_csr_split_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                         const uint32_t *colIdxs, const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat,
                                         uint64_t k_head_stride, uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv,
                                         uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, float *out,
                                         uint64_t out_head_stride, uint32_t ldo, float *lse, uint32_t splits, uint32_t min_batches,
                                         void *workspace, uint64_t workspace_bytes) {
    return split_entry<ElemF32>("attn_csr_split_f32", "f32", stream, H, M, K, nnz, rowPtrs, colIdxs, Q, q_head_stride, ldq, Kmat, k_head_stride, ldk,
                                D, V, v_head_stride, ldv, Dv, scale, bias, bias_head_stride, out, out_head_stride, ldo, 0, lse, splits, min_batches,
                                workspace, workspace_bytes);
}

extern "C" int mispmm_attn_csr_split_bf16(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                          const uint32_t *colIdxs, const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat,
                                          uint64_t k_head_stride, uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv,
                                          uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, void *out,
                                          uint64_t out_head_stride, uint32_t ldo, int out_bf16, float *lse, uint32_t splits, uint32_t min_batches,
                                          void *workspace, uint64_t workspace_bytes) {
    return split_entry<ElemBf16>("attn_csr_split_bf16", "bf16", stream, H, M, K, nnz, rowPtrs, colIdxs, Q, q_head_stride, ldq, Kmat, k_head_stride,
                                 ldk, D, V, v_head_stride, ldv, Dv, scale, bias, bias_head_stride, out, out_head_stride, ldo, out_bf16, lse, splits,
                                 min_batches, workspace, workspace_bytes);
}
