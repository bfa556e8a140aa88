// libmispmm_attn_csr_bf16.so: fused attention on a CSR pattern with Q, K and V in bf16 (include/mispmm_attn_csr_bf16.h) --
// scores, row softmax and the product with V in ONE launch for all heads, fp32 arithmetic on the exactly widened operands.
//   z[e]      = fma(scale, <Q_h[r, :D], K_h[c, :D]>, bias_h[e])          c = colIdxs[e], e over the stored entries of row r
//   out_h[r]  = sum_e softmax_e(z) * V_h[c, :Dv]                         fp32, or that fp32 result rounded once to bf16
//
// Shape: that of attn_csr/attn_csr.hip, statement for statement, in the lane group of attn_csr/lane_group.hpp (the constants,
// the exp2 wrapper, join_off, the transposing butterfly and the host's span / finish_grid / refuse_* come from there; the
// header is included read-only: its two fp32 users are held to identical ISA).  What is specific to bf16 stands here:
//  - a lane's byte offset (2 bytes per column) and the row gathers: V8, 8 consecutive columns of a row as one 16-byte
//    buffer load (the register cost of the fp32 kernel's V4 row), or V1, one buffer_load_ushort per column;
//  - the widening dot chain: element 2i of a dword is its low half, 2i + 1 its high half, each widened by moving its bits
//    to the upper half of an fp32 (exact, nothing flushed or quieted), then ONE fma chain per lane from +0, columns
//    ascending -- not a packed dot instruction: the bits of z are determined (the header's ALGORITHM);
//  - Q[r]'s slice is widened once and held as floats; the accumulator is 8 floats per lane at V8;
//  - the store: fp32, or v_cvt_pk_bf16_f32 of the same quotients (a wave-uniform branch: no instances of its own).
// Per batch the 8 x NCH K-row reads and the 8 x NCH V-row reads are issued together, the K reads first: the vector-memory
// counter is in order, so the dot products wait for K alone.  The column keys and the bias of a batch are fetched one batch
// ahead; the two statements that pin that fetch in its iteration are those of attn_csr.hip.
// Dead slots and lanes past D / Dv read through the dropped-load offset, joined by the saturating add.
// The sources lie outside csrc/, fused/, rows_bf16/ and attn_csr/: the census tests hold those directories and their
// libraries to their records.
#include "../attn_csr/lane_group.hpp"
#include "mispmm_attn_csr_bf16.h"

namespace mispmm {

namespace {

using u32x4 = uint32_t __attribute__((ext_vector_type(4)));

// VEC bf16 elements of a row as they are loaded: element 2i in the low half of dword i, element 2i + 1 in the high half;
// a single element zero-extended
template <int VEC> struct RawOf;
template <> struct RawOf<1> { using type = uint32_t; };
template <> struct RawOf<8> { using type = u32x4; };

template <int VEC>
__device__ __forceinline__ typename RawOf<VEC>::type buffer_load_bf16(rsrc_t rsrc, uint32_t voffset) {
    if constexpr (VEC == 1) return __builtin_amdgcn_raw_buffer_load_b16(rsrc, voffset, 0, 0);
    else return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, 0, 0);
}

// element i widened to fp32 exactly: the bits moved to the upper half
template <int VEC>
__device__ __forceinline__ float widen(const typename RawOf<VEC>::type &raw, int i) {
    if constexpr (VEC == 1) return __uint_as_float(raw << 16);
    else return __uint_as_float((i & 1) ? (raw[i >> 1] & 0xFFFF0000u) : (raw[i >> 1] << 16));
}

// one rounding to nearest even, a NaN stays a NaN: v_cvt_pk_bf16_f32, as rows_bf16/ and mispmm_f32_to_bf16
__device__ __forceinline__ uint32_t bf16_bits(float x) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(x)); }
__device__ __forceinline__ uint32_t bf16_pair(float lo, float hi) { return bf16_bits(lo) | (bf16_bits(hi) << 16); }

// byte offset of the lane's columns of chunk c in a bf16 row of `width` columns; past the width: the dropped-load mark
template <int G, int VEC>
__device__ __forceinline__ uint32_t lane_off_bf16(uint32_t lane, int c, uint32_t width) {
    const uint32_t col = c * (G * VEC) + lane * VEC;
    return col < width ? col * 2u : kDropLoad;
}

// the lane's slices of the batch's 8 rows of one operand; key: byte offset of the row of entry `sub`, or the mark
template <int VEC, int NCH>
__device__ __forceinline__ void gather_rows_bf16(uint32_t key, rsrc_t r, const uint32_t (&off)[NCH],
                                                 typename RawOf<VEC>::type (&rows)[kLgBatch][NCH]) {
    static_for<0, kLgBatch>([&](auto j_tag) {
        constexpr int j = decltype(j_tag)::value;
        const uint32_t kj = group_bcast<8, j>(key);
#pragma unroll
        for (int c = 0; c < NCH; ++c) rows[j][c] = buffer_load_bf16<VEC>(r, join_off(kj, off[c]));
    });
}

struct AbParams {
    uint32_t M, D, Dv, blocks_per_head, total, xcd_chunk;
    uint32_t ldq2, ldk2, ldv2, ldo;                   // ldq2, ldk2, ldv2: row strides in bytes; ldo in elements of out
    uint32_t q_bytes, k_bytes, v_bytes, bias_bytes;   // one head's span; bias_bytes == 0: no bias
    uint32_t out_bf16;
    float scale;
    uint64_t q_head, k_head, v_head, o_head, bias_head;  // elements
};

template <int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_bf16_kernel(const AbParams p, const uint32_t *__restrict__ rowPtrs,
                                                                 const uint32_t *__restrict__ colIdxs, const uint16_t *__restrict__ Q,
                                                                 const uint16_t *__restrict__ K, const uint16_t *__restrict__ V,
                                                                 const float *__restrict__ bias, void *__restrict__ out,
                                                                 float *__restrict__ lse_out) {
    using raw_t = typename RawOf<VEC>::type;
    static_assert(VEC == 8 || VEC == 1, "16-byte lanes or element lanes: there is no 8-byte form");
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scores sit in the first lanes of a group");
    static_assert(NCH == 1 || (G == kWave && VEC == 1), "more than one chunk only where a whole wave of element lanes owns the row");
    constexpr int GROUPS = kLgBlock / G, E = kLgBatch;
    constexpr uint32_t CHUNK = G * VEC;
    const uint32_t lane = threadIdx.x % G, sub = lane & (E - 1);
    const uint32_t item = xcd_block(blockIdx.x, p.xcd_chunk);
    if (item >= p.total) return;
    const uint32_t h = item / p.blocks_per_head;  // wave-uniform: a workgroup lies inside one head
    const uint64_t row64 = static_cast<uint64_t>(item - h * p.blocks_per_head) * GROUPS + threadIdx.x / G;
    if (row64 >= p.M) return;  // the lanes a move reads from are all in the lane's own group, which leaves as one
    const uint32_t row = static_cast<uint32_t>(row64);
    const uint32_t base = rowPtrs[row];
    const uint32_t len = rowPtrs[row + 1] - base;
    const float ninf = -__builtin_huge_valf();

    const size_t out_at = static_cast<size_t>(h) * p.o_head + static_cast<size_t>(row) * p.ldo;  // elements of out's type
    float o[NCH][VEC];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[c][v] = 0.f;
    // the lane's columns of chunk c are inside Dv or past it together (VEC == 8: Dv is a multiple of 8)
    auto store = [&](float l, float lse) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t col = c * CHUNK + lane * VEC;
            if (col >= p.Dv) continue;
            float r[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) r[v] = o[c][v] / l;
            if (p.out_bf16) {  // wave-uniform; the fp32 quotient rounded once
                uint16_t *at = static_cast<uint16_t *>(out) + out_at + col;
                if constexpr (VEC == 1) *at = static_cast<uint16_t>(bf16_bits(r[0]));
                else *reinterpret_cast<u32x4 *>(at) = u32x4{bf16_pair(r[0], r[1]), bf16_pair(r[2], r[3]), bf16_pair(r[4], r[5]), bf16_pair(r[6], r[7])};
            } else {
                float *at = static_cast<float *>(out) + out_at + col;
                if constexpr (VEC == 1) {
                    *at = r[0];
                } else {
                    store_vec<4>(at, f32x4{r[0], r[1], r[2], r[3]});
                    store_vec<4>(at + 4, f32x4{r[4], r[5], r[6], r[7]});
                }
            }
        }
        if (lse_out && lane == 0) lse_out[static_cast<size_t>(h) * p.M + row] = lse;
    };
    if (len == 0) {  // an empty row: +0 / 1 and lse = log 0
        store(1.f, ninf);
        return;
    }

    const rsrc_t qr = make_rsrc(Q + h * p.q_head, p.q_bytes), kr = make_rsrc(K + h * p.k_head, p.k_bytes);
    const rsrc_t vr = make_rsrc(V + h * p.v_head, p.v_bytes);
    const rsrc_t br = make_rsrc(bias ? bias + h * p.bias_head : nullptr, p.bias_bytes);  // spans nothing without a bias: reads give +0
    uint32_t koff[NCH], voff[NCH];
    float xq[NCH][VEC];  // Q[r]'s slice, widened once
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        koff[c] = lane_off_bf16<G, VEC>(lane, c, p.D);
        voff[c] = lane_off_bf16<G, VEC>(lane, c, p.Dv);
        const raw_t qraw = buffer_load_bf16<VEC>(qr, join_off(row * p.ldq2, koff[c]));  // past D: zeros
#pragma unroll
        for (int v = 0; v < VEC; ++v) xq[c][v] = widen<VEC>(qraw, v);
    }
    // entry c0 + sub of the row and its bias: every 8-lane segment of the group holds the batch's 8 entries.  A slot past the
    // row end re-reads the row's first entry (it exists: len > 0); what it yields is replaced below.
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
    for (uint32_t s0 = 0; s0 < len; s0 += E) {
        const bool live = s0 + sub < len;
        // the mark is OR-ed in, not selected: with a select the compiler sinks the column fetch into a branch on `live` at the
        // top of the NEXT batch and waits for it there, and the fetch is no longer a batch ahead (a live key is below 2^31)
        const uint32_t dead = live ? 0u : kDropLoad;
        const uint32_t kkey = nxt_col * p.ldk2 | dead;
        const uint32_t vkey = nxt_col * p.ldv2 | dead;
        const float b = nxt_bias;
        fetch(s0 + E, nxt_col, nxt_bias);  // on its way while this batch is gathered
        __builtin_amdgcn_sched_barrier(0);  // ... issued here, ahead of the batch's own reads (see the end of the loop body)
        raw_t kv[E][NCH], vv[E][NCH];
        gather_rows_bf16<VEC, NCH>(kkey, kr, koff, kv);
        gather_rows_bf16<VEC, NCH>(vkey, vr, voff, vv);
        float acc[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[j] = __builtin_fmaf(xq[c][v], widen<VEC>(kv[j][c], v), acc[j]);
        }
        const float s = transpose_sum<G>(acc, lane);
        // lane (any segment, position sub) now holds the score of entry s0 + sub
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
                for (int v = 0; v < VEC; ++v) o[c][v] = __builtin_fmaf(wj, widen<VEC>(vv[j][c], v), o[c][v]);
        });
        // the next batch's column and bias must be in their registers HERE: without this the compiler moves the fetch over
        // the loop edge to the top of the batch that uses it and waits for it there, one exposed round trip per batch.  The
        // batch's own reads have all been waited for by now, so the empty statement costs no wait of its own.
        asm volatile("" : "+v"(nxt_col), "+v"(nxt_bias));
    }
    store(l, mu + __builtin_logf(l));
}

struct AbCall {
    hipStream_t stream;
    uint32_t H;
    AbParams p;
    const uint32_t *rowPtrs, *colIdxs;
    const uint16_t *Q, *K, *V;
    const float *bias;
    void *out;
    float *lse;
};

template <int G, int VEC, int NCH>
void launch_attn_csr_bf16(const AbCall &c) {
    AbParams p = c.p;
    const uint32_t grid = finish_grid<G>(p, p.M, c.H);
    note_kernel("attn_csr_bf16<G%d,V%d,C%d>", G, VEC, NCH);
    hipLaunchKernelGGL((attn_csr_bf16_kernel<G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.rowPtrs, c.colIdxs, c.Q, c.K, c.V,
                       c.bias, c.out, c.lse);
}

// f(G, VEC, NCH) as constants: the one list of the 3 + 6 instances that exist.  V8: 32 x 8 covers 256
template <class F>
void with_instance_bf16(int vec, int g, uint32_t width, F &&f) {
    using std::integral_constant;
    if (vec == 8) {
        with_const<8, 16, 32>(g, [&](auto gr) { f(gr, integral_constant<int, 8>{}, integral_constant<int, 1>{}); });
    } else if (!try_const<8, 16, 32>(g, [&](auto gr) { f(gr, integral_constant<int, 1>{}, integral_constant<int, 1>{}); })) {
        const uint32_t chunks = ceil_div(width, static_cast<uint32_t>(kWave));
        with_const<1, 2, 4>(chunks <= 1 ? 1 : chunks == 2 ? 2 : 4,
                            [&](auto ch) { f(integral_constant<int, 64>{}, integral_constant<int, 1>{}, ch); });
    }
}

inline bool aligned2(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 1u) == 0; }

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_attn_csr_bf16(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                    const uint32_t *colIdxs, const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat,
                                    uint64_t k_head_stride, uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv,
                                    uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, void *out,
                                    uint64_t out_head_stride, uint32_t ldo, int out_bf16, float *lse) {
    if (const int st = refuse_shape("attn_csr_bf16", D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0) return MISPMM_OK;
    if (!rowPtrs || !Q || !Kmat || !V || !out || (nnz != 0 && !colIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16: rowPtrs, colIdxs, Q, K, V or out is null");
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)",
                    D, ldq, ldk, Dv, ldv, ldo);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load: bytes of the element type
    const uint64_t o_elem = out_bf16 ? 2u : 4u;
    const uint64_t qs = span(M, ldq, D) * 2u, ks = span(K, ldk, D) * 2u, vs = span(K, ldv, Dv) * 2u, os = span(M, ldo, Dv) * o_elem;
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) * 4u : 0u;
    if (qs > 0x7FFFFFFFull || ks > 0x7FFFFFFFull || vs > 0x7FFFFFFFull || os > 0x7FFFFFFFull || bs > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "attn_csr_bf16: Q, K, V, out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu bytes)",
                    static_cast<unsigned long long>(qs), static_cast<unsigned long long>(ks), static_cast<unsigned long long>(vs),
                    static_cast<unsigned long long>(os), static_cast<unsigned long long>(bs));
    const bool wide = D % 8 == 0 && Dv % 8 == 0 && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && q_head_stride % 8 == 0 &&
                      k_head_stride % 8 == 0 && v_head_stride % 8 == 0 && out_head_stride % 8 == 0 && aligned16(Q) && aligned16(Kmat) &&
                      aligned16(V) && aligned16(out);
    const int vec = wide ? 8 : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid("attn_csr_bf16", M, H, g); st != MISPMM_OK) return st;
    if (!aligned2(Q) || !aligned2(Kmat) || !aligned2(V) || (out_bf16 && !aligned2(out)))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16: Q, K, V and a bf16 out must be 2-byte aligned");
    AbCall c{};
    c.stream = as_stream(stream);
    c.H = H;
    c.rowPtrs = rowPtrs, c.colIdxs = colIdxs;
    c.Q = Q, c.K = Kmat, c.V = V, c.bias = bias, c.out = out, c.lse = lse;
    AbParams &p = c.p;
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq2 = ldq * 2u, p.ldk2 = ldk * 2u, p.ldv2 = ldv * 2u, p.ldo = ldo;
    p.q_bytes = static_cast<uint32_t>(qs), p.k_bytes = static_cast<uint32_t>(ks), p.v_bytes = static_cast<uint32_t>(vs);
    p.bias_bytes = static_cast<uint32_t>(bs);
    p.out_bf16 = out_bf16 ? 1u : 0u;
    p.scale = scale;
    p.q_head = q_head_stride, p.k_head = k_head_stride, p.v_head = v_head_stride, p.o_head = out_head_stride, p.bias_head = bias_head_stride;
    with_instance_bf16(vec, g, width,
                       [&](auto gr, auto v, auto ch) { launch_attn_csr_bf16<decltype(gr)::value, decltype(v)::value, decltype(ch)::value>(c); });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
