// libmispmm_attn_csr_bf16_bwd.so: the backward of fused attention on a CSR pattern with Q, K, V and grad_out in bf16
// (include/mispmm_attn_csr_bf16_bwd.h) -- dQ, dK and dV for all heads in at most two launches, fp32 arithmetic on the exactly
// widened operands, no fp32 copy of any operand.  The only thing that goes through memory between the launches is delta [H][M].
//   z[e]   = fma(scale, <Q_h[r, :D], K_h[c, :D]>, bias_h[e])
//   P[e]   = exp(z[e] - lse_h[r])                 dP[e] = <dO_h[r, :Dv], V_h[c, :Dv]>          delta_h[r] = <dO_h[r], out_h[r]>
//   dS[e]  = scale * P[e] * (dP[e] - delta_h[r])
//   dQ_h[r] = sum over row r of dS[e] K_h[c]      dK_h[c] = sum over column c of dS[e] Q_h[r]  dV_h[c] = sum over column c of P[e] dO_h[r]
//
// Shape: the two passes of attn_csr/bwd/attn_csr_bwd.hip, statement for statement, in the lane group of
// attn_csr/lane_group.hpp (included read-only, as the bf16 forward does).  What is specific to bf16 is the forward's
// (attn_csr_bf16/attn_csr_bf16.hip), restated here so that the forward's translation unit stays as it is:
//  - RawOf / buffer_load_bf16 / widen / lane_off_bf16 / gather_rows_bf16: V8, 8 consecutive columns of a row as one 16-byte
//    buffer load, or V1, one buffer_load_ushort per column; element 2i of a dword is its low half;
//  - every dot product is ONE fma chain per lane from +0, columns ascending, on widened values -- no packed dot instruction;
//  - the values a group holds for its own row (Q[r] and dO[r]; K[c] and V[c]) are widened once into floats;
//  - the store: fp32, or v_cvt_pk_bf16_f32 of the same accumulators (a wave-uniform branch: no instances of its own).
// out and lse are the fp32 ones the bf16 forward wrote; out[r] is read once per row for delta (V8: two 16-byte loads).
// The per-entry arithmetic (z, P, dS), the dead slots, the index fetch a batch ahead with its two pinning statements and the
// column pass's per-entry scalars issued first are those of the fp32 backward.  On V1 a lane's chains are the fp32 kernel's
// V1 chains on the widened values: every output has that kernel's bits.  On V8 a lane's chain covers 8 columns against 4.
#include "../../attn_csr/lane_group.hpp"
#include "mispmm_attn_csr_bf16_bwd.h"

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

// one rounding to nearest even, a NaN stays a NaN: v_cvt_pk_bf16_f32, as the forward's bf16 out
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

// the lane's VEC gradient columns to row `at` (elements of the gradient's own type): fp32, or the same values rounded once
template <int VEC>
__device__ __forceinline__ void store_grad(void *base, size_t at, const float *r, bool bf16) {
    if (bf16) {  // wave-uniform
        uint16_t *to = static_cast<uint16_t *>(base) + at;
        if constexpr (VEC == 1) *to = static_cast<uint16_t>(bf16_bits(r[0]));
        else *reinterpret_cast<u32x4 *>(to) = u32x4{bf16_pair(r[0], r[1]), bf16_pair(r[2], r[3]), bf16_pair(r[4], r[5]), bf16_pair(r[6], r[7])};
    } else {
        float *to = static_cast<float *>(base) + at;
        if constexpr (VEC == 1) {
            *to = r[0];
        } else {
            store_vec<4>(to, f32x4{r[0], r[1], r[2], r[3]});
            store_vec<4>(to + 4, f32x4{r[4], r[5], r[6], r[7]});
        }
    }
}

// P of one entry: exp(z - lse) with one rounding of the difference; a row whose lse is not finite is NaN throughout, as a
// softmax over a +Inf, a NaN or nothing but -Inf is (z - (+Inf) alone would give +0)
__device__ __forceinline__ float weight(float z, float lse) {
    return __builtin_fabsf(lse) < __builtin_huge_valf() ? lg_exp(z - lse) : __builtin_nanf("");
}

struct AbParams {
    uint32_t M, N, D, Dv, blocks_per_head, total, xcd_chunk;  // N: rows of the pass's own pattern (M for the row pass, K for the column pass)
    uint32_t ldq2, ldk2, ldv2, ldg2, ldo4;                     // row strides in bytes: 2 per element of Q, K, V and dO, 4 of out
    uint32_t ldd0, ldd1;                                       // row strides of the pass's outputs in elements (dQ | dK, dV)
    uint32_t q_bytes, k_bytes, v_bytes, g_bytes, o_bytes, bias_bytes;  // one head's span; bias_bytes == 0: no bias
    uint32_t grads_bf16;
    float scale;
    uint64_t q_head, k_head, v_head, g_head, o_head, bias_head, d0_head, d1_head;  // elements
};

struct AbPtrs {
    const uint32_t *ptrs, *idxs, *perm;  // the pass's own pattern; perm: column pass with a bias, else null
    const uint16_t *Q, *K, *V, *dO;
    const float *out, *lse, *bias;
    float *delta;  // written by the row pass, read by the column pass
    void *d0, *d1;  // row pass: dQ, -; column pass: dK, dV; null: not asked for
};

template <int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_bf16_bwd_row_kernel(const AbParams p, const AbPtrs a) {
    using raw_t = typename RawOf<VEC>::type;
    static_assert(VEC == 8 || VEC == 1, "16-byte lanes or element lanes: there is no 8-byte form");
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scalars sit in the first lanes of a group");
    static_assert(NCH == 1 || (G == kWave && VEC == 1), "more than one chunk only where a whole wave of element lanes owns the row");
    constexpr int GROUPS = kLgBlock / G, E = kLgBatch;
    constexpr uint32_t CHUNK = G * VEC;
    const uint32_t lane = threadIdx.x % G, sub = lane & (E - 1);
    const uint32_t item = xcd_block(blockIdx.x, p.xcd_chunk);
    if (item >= p.total) return;
    const uint32_t h = item / p.blocks_per_head;  // wave-uniform: a workgroup lies inside one head
    const uint64_t row64 = static_cast<uint64_t>(item - h * p.blocks_per_head) * GROUPS + threadIdx.x / G;
    if (row64 >= p.N) return;  // the lanes a move reads from are all in the lane's own group, which leaves as one
    const uint32_t row = static_cast<uint32_t>(row64);

    const rsrc_t qr = make_rsrc(a.Q + h * p.q_head, p.q_bytes), kr = make_rsrc(a.K + h * p.k_head, p.k_bytes);
    const rsrc_t vr = make_rsrc(a.V + h * p.v_head, p.v_bytes), gr = make_rsrc(a.dO + h * p.g_head, p.g_bytes);
    const rsrc_t orr = make_rsrc(a.out + h * p.o_head, p.o_bytes);
    const rsrc_t br = make_rsrc(a.bias ? a.bias + h * p.bias_head : nullptr, p.bias_bytes);  // spans nothing without a bias: reads give +0
    uint32_t koff[NCH], voff[NCH];
    float xq[NCH][VEC], xg[NCH][VEC];  // Q[r]'s and dO[r]'s slices, widened once
    float dsum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        koff[c] = lane_off_bf16<G, VEC>(lane, c, p.D);
        voff[c] = lane_off_bf16<G, VEC>(lane, c, p.Dv);
        const raw_t qraw = buffer_load_bf16<VEC>(qr, join_off(row * p.ldq2, koff[c]));  // past D: zeros
        const raw_t graw = buffer_load_bf16<VEC>(gr, join_off(row * p.ldg2, voff[c]));  // past Dv: zeros
        // out is fp32: the same columns at 4 bytes each (twice the bf16 offset; the mark stays the mark)
        const uint32_t ooff = join_off(row * p.ldo4, join_off(voff[c], voff[c]));
        float xo[VEC];
        if constexpr (VEC == 1) {
            xo[0] = buffer_load_vec<1>(orr, ooff, 0);
        } else {
            const f32x4 lo = buffer_load_vec<4>(orr, ooff, 0), hi = buffer_load_vec<4>(orr, join_off(ooff, 16u), 0);
#pragma unroll
            for (int v = 0; v < 4; ++v) xo[v] = lo[v], xo[v + 4] = hi[v];
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            xq[c][v] = widen<VEC>(qraw, v);
            xg[c][v] = widen<VEC>(graw, v);
            dsum = __builtin_fmaf(xg[c][v], xo[v], dsum);
        }
    }
    const float delta = group_all_reduce<G>(dsum, [](float x, float y) { return x + y; });  // lanes 1, 2, 4, ... apart: the same bits in every lane
    const size_t hr = static_cast<size_t>(h) * p.M + row;
    if (lane == 0) a.delta[hr] = delta;
    if (!a.d0) return;  // dQ is not asked for: the pass was launched for delta

    float dq[NCH][VEC];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) dq[c][v] = 0.f;
    const size_t dq_at = static_cast<size_t>(h) * p.d0_head + static_cast<size_t>(row) * p.ldd0;
    // the lane's columns of chunk c are inside D or past it together (VEC == 8: D is a multiple of 8)
    auto store = [&]() {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t col = c * CHUNK + lane * VEC;
            if (col >= p.D) continue;
            store_grad<VEC>(a.d0, dq_at + col, dq[c], p.grads_bf16 != 0);
        }
    };
    const uint32_t base = a.ptrs[row];
    const uint32_t len = a.ptrs[row + 1] - base;
    if (len == 0) {  // an empty row: +0
        store();
        return;
    }
    const float lse = a.lse[hr];
    // entry c0 + sub of the row and its bias: every 8-lane segment of the group holds the batch's 8 entries.  A slot past the
    // row end re-reads the row's first entry (it exists: len > 0); what it yields is replaced below.
    auto fetch = [&](uint32_t c0, uint32_t &col, float &b) {
        const uint32_t idx = c0 + sub;
        const uint32_t e = base + (idx < len ? idx : 0u);
        col = a.idxs[e];
        b = buffer_load_vec<1>(br, e * 4u, 0);
    };
    uint32_t nxt_col;
    float nxt_bias;
    fetch(0, nxt_col, nxt_bias);
    for (uint32_t s0 = 0; s0 < len; s0 += E) {
        const bool live = s0 + sub < len;
        // the mark is OR-ed in, not selected (attn_csr.hip: a select lets the compiler sink the fetch into a branch on `live`)
        const uint32_t dead = live ? 0u : kDropLoad;
        const uint32_t kkey = nxt_col * p.ldk2 | dead;
        const uint32_t vkey = nxt_col * p.ldv2 | dead;
        const float b = nxt_bias;
        fetch(s0 + E, nxt_col, nxt_bias);  // on its way while this batch is gathered
        __builtin_amdgcn_sched_barrier(0);  // ... issued here, ahead of the batch's own reads (see the end of the loop body)
        raw_t kv[E][NCH], vv[E][NCH];
        gather_rows_bf16<VEC, NCH>(kkey, kr, koff, kv);
        gather_rows_bf16<VEC, NCH>(vkey, vr, voff, vv);
        float acc_s[E], acc_p[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc_s[j] = 0.f;
            acc_p[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc_s[j] = __builtin_fmaf(xq[c][v], widen<VEC>(kv[j][c], v), acc_s[j]);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc_p[j] = __builtin_fmaf(xg[c][v], widen<VEC>(vv[j][c], v), acc_p[j]);
            }
        }
        const float s = transpose_sum<G>(acc_s, lane);
        const float dp = transpose_sum<G>(acc_p, lane);
        // lane (any segment, position sub) now holds s and dP of entry s0 + sub
        const float z = __builtin_fmaf(p.scale, s, b);
        const float w = weight(z, lse);
        float ds = dp - delta;
        ds = w * ds;
        ds = ds * p.scale;
        ds = live ? ds : 0.f;
        static_for<0, E>([&](auto j_tag) {
            constexpr int j = decltype(j_tag)::value;
            const float dj = __uint_as_float(group_bcast<8, j>(__float_as_uint(ds)));
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v) dq[c][v] = __builtin_fmaf(dj, widen<VEC>(kv[j][c], v), dq[c][v]);
        });
        // the next batch's column and bias must be in their registers HERE (attn_csr.hip): otherwise the fetch moves over the
        // loop edge to the top of the batch that uses it
        asm volatile("" : "+v"(nxt_col), "+v"(nxt_bias));
    }
    store();
}

template <int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_bf16_bwd_col_kernel(const AbParams p, const AbPtrs a) {
    using raw_t = typename RawOf<VEC>::type;
    static_assert(VEC == 8 || VEC == 1, "16-byte lanes or element lanes: there is no 8-byte form");
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scalars sit in the first lanes of a group");
    static_assert(NCH == 1 || (G == kWave && VEC == 1), "more than one chunk only where a whole wave of element lanes owns the row");
    constexpr int GROUPS = kLgBlock / G, E = kLgBatch;
    constexpr uint32_t CHUNK = G * VEC;
    const uint32_t lane = threadIdx.x % G, sub = lane & (E - 1);
    const uint32_t item = xcd_block(blockIdx.x, p.xcd_chunk);
    if (item >= p.total) return;
    const uint32_t h = item / p.blocks_per_head;
    const uint64_t key64 = static_cast<uint64_t>(item - h * p.blocks_per_head) * GROUPS + threadIdx.x / G;
    if (key64 >= p.N) return;
    const uint32_t key = static_cast<uint32_t>(key64);
    const bool want_dk = a.d0 != nullptr, want_dv = a.d1 != nullptr;  // uniform over the launch

    float dk[NCH][VEC], dv[NCH][VEC];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) dk[c][v] = 0.f, dv[c][v] = 0.f;
    auto store = [&]() {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t col = c * CHUNK + lane * VEC;
            if (want_dk && col < p.D)
                store_grad<VEC>(a.d0, static_cast<size_t>(h) * p.d0_head + static_cast<size_t>(key) * p.ldd0 + col, dk[c], p.grads_bf16 != 0);
            if (want_dv && col < p.Dv)
                store_grad<VEC>(a.d1, static_cast<size_t>(h) * p.d1_head + static_cast<size_t>(key) * p.ldd1 + col, dv[c], p.grads_bf16 != 0);
        }
    };
    const uint32_t base = a.ptrs[key];
    const uint32_t len = a.ptrs[key + 1] - base;
    if (len == 0) {  // a key no row attends to: +0
        store();
        return;
    }
    const rsrc_t qr = make_rsrc(a.Q + h * p.q_head, p.q_bytes), kr = make_rsrc(a.K + h * p.k_head, p.k_bytes);
    const rsrc_t vr = make_rsrc(a.V + h * p.v_head, p.v_bytes), gr = make_rsrc(a.dO + h * p.g_head, p.g_bytes);
    const rsrc_t br = make_rsrc(a.bias ? a.bias + h * p.bias_head : nullptr, p.bias_bytes);
    const float *lse_h = a.lse + static_cast<size_t>(h) * p.M;
    const float *delta_h = a.delta + static_cast<size_t>(h) * p.M;  // not read without dK
    uint32_t qoff[NCH], goff[NCH];
    float xk[NCH][VEC], xv[NCH][VEC];  // K[c]'s and V[c]'s slices, widened once
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        qoff[c] = lane_off_bf16<G, VEC>(lane, c, p.D);
        goff[c] = lane_off_bf16<G, VEC>(lane, c, p.Dv);
        const raw_t kraw = buffer_load_bf16<VEC>(kr, join_off(key * p.ldk2, qoff[c]));  // past D: zeros
        const raw_t vraw = buffer_load_bf16<VEC>(vr, join_off(key * p.ldv2, goff[c]));  // past Dv: zeros; read only for dP
#pragma unroll
        for (int v = 0; v < VEC; ++v) xk[c][v] = widen<VEC>(kraw, v), xv[c][v] = widen<VEC>(vraw, v);
    }
    // entry c0 + sub of the column: the row it lies in, and where its bias lies in A's order.  A slot past the end re-reads
    // the column's first entry (it exists), so the per-entry scalars of a dead slot are read from a real row.
    auto fetch = [&](uint32_t c0, uint32_t &r, uint32_t &e_a) {
        const uint32_t idx = c0 + sub;
        const uint32_t t = base + (idx < len ? idx : 0u);
        r = a.idxs[t];
        e_a = a.perm ? a.perm[t] : 0u;  // uniform: perm is handed in with a bias only
    };
    uint32_t nxt_r, nxt_e;
    fetch(0, nxt_r, nxt_e);
    for (uint32_t s0 = 0; s0 < len; s0 += E) {
        const bool live = s0 + sub < len;
        const uint32_t dead = live ? 0u : kDropLoad;
        const uint32_t r = nxt_r;
        const uint32_t qkey = r * p.ldq2 | dead;
        const uint32_t gkey = r * p.ldg2 | dead;
        const uint32_t e_a = nxt_e;
        fetch(s0 + E, nxt_r, nxt_e);
        __builtin_amdgcn_sched_barrier(0);
        // the entry's own scalars first: they are behind the rows in no queue
        const float lse = lse_h[r];
        const float delta = want_dk ? delta_h[r] : 0.f;
        const float b = buffer_load_vec<1>(br, e_a * 4u, 0);
        raw_t qv[E][NCH], gv[E][NCH];
        gather_rows_bf16<VEC, NCH>(qkey, qr, qoff, qv);
        gather_rows_bf16<VEC, NCH>(gkey, gr, goff, gv);
        float acc_s[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc_s[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc_s[j] = __builtin_fmaf(widen<VEC>(qv[j][c], v), xk[c][v], acc_s[j]);
        }
        const float s = transpose_sum<G>(acc_s, lane);
        const float z = __builtin_fmaf(p.scale, s, b);
        float w = weight(z, lse);
        w = live ? w : 0.f;
        if (want_dv) {
            static_for<0, E>([&](auto j_tag) {
                constexpr int j = decltype(j_tag)::value;
                const float wj = __uint_as_float(group_bcast<8, j>(__float_as_uint(w)));
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) dv[c][v] = __builtin_fmaf(wj, widen<VEC>(gv[j][c], v), dv[c][v]);
            });
        }
        if (want_dk) {
            // the rows stay in their 64 loaded registers: each element is widened again where it is used a second time.  Without
            // these statements the compiler keeps all 128 widened floats of a batch alive from their first use to their second
            // (192 VGPRs and 2 waves per SIMD at V8; 1 instruction per element is what the second widening costs)
            if constexpr (VEC == 8) {
#pragma unroll
                for (int j = 0; j < E; ++j)
#pragma unroll
                    for (int c = 0; c < NCH; ++c) asm volatile("" : "+v"(gv[j][c]));
            }
            float acc_p[E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                acc_p[j] = 0.f;
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc_p[j] = __builtin_fmaf(widen<VEC>(gv[j][c], v), xv[c][v], acc_p[j]);
            }
            const float dp = transpose_sum<G>(acc_p, lane);
            float ds = dp - delta;
            ds = w * ds;
            ds = ds * p.scale;
            ds = live ? ds : 0.f;
            if constexpr (VEC == 8) {
#pragma unroll
                for (int j = 0; j < E; ++j)
#pragma unroll
                    for (int c = 0; c < NCH; ++c) asm volatile("" : "+v"(qv[j][c]));
            }
            static_for<0, E>([&](auto j_tag) {
                constexpr int j = decltype(j_tag)::value;
                const float dj = __uint_as_float(group_bcast<8, j>(__float_as_uint(ds)));
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) dk[c][v] = __builtin_fmaf(dj, widen<VEC>(qv[j][c], v), dk[c][v]);
            });
        }
        asm volatile("" : "+v"(nxt_r), "+v"(nxt_e));
    }
    store();
}

struct AbCall {
    hipStream_t stream;
    uint32_t H;
    AbParams p;
    AbPtrs a;
};

template <bool ROW, int G, int VEC, int NCH>
void launch_pass(const AbCall &c) {
    AbParams p = c.p;
    const uint32_t grid = finish_grid<G>(p, p.N, c.H);
    if constexpr (ROW) {
        note_kernel("attn_csr_bf16_bwd_row<G%d,V%d,C%d>", G, VEC, NCH);
        hipLaunchKernelGGL((attn_csr_bf16_bwd_row_kernel<G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.a);
    } else {
        note_kernel("attn_csr_bf16_bwd_col<G%d,V%d,C%d>", G, VEC, NCH);
        hipLaunchKernelGGL((attn_csr_bf16_bwd_col_kernel<G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.a);
    }
}

// f(G, VEC, NCH) as constants: the forward's list of 3 + 6 instances, here per pass.  V8: 32 x 8 covers 256
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

template <bool ROW>
void dispatch_pass(const AbCall &c, int vec, int g, uint32_t width) {
    with_instance_bf16(vec, g, width,
                       [&](auto gr, auto v, auto ch) { launch_pass<ROW, decltype(gr)::value, decltype(v)::value, decltype(ch)::value>(c); });
}

inline bool aligned2(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 1u) == 0; }

struct Extent {
    const char *lo, *hi;
};
// bytes H heads of an operand of `elem`-byte elements cover (a head stride of 0: one head's); strides and span in elements
Extent extent(const void *base, uint32_t H, uint64_t head_stride, uint64_t head_span, uint64_t elem) {
    const char *lo = static_cast<const char *>(base);
    return {lo, base && head_span ? lo + ((H - 1) * head_stride + head_span) * elem : lo};
}
bool meet(const Extent &x, const Extent &y) { return x.lo < y.hi && y.lo < x.hi; }

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_attn_csr_bf16_bwd(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                        const uint32_t *colIdxs, const uint32_t *tRowPtrs, const uint32_t *tColIdxs, const uint32_t *perm,
                                        const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat, uint64_t k_head_stride,
                                        uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv, uint32_t Dv,
                                        float scale, const float *bias, uint64_t bias_head_stride, const float *out,
                                        uint64_t out_head_stride, uint32_t ldo, const float *lse, const uint16_t *grad_out,
                                        uint64_t g_head_stride, uint32_t ldg, float *delta, int grads_bf16, void *dQ,
                                        uint64_t dq_head_stride, uint32_t lddq, void *dK, uint64_t dk_head_stride, uint32_t lddk, void *dV,
                                        uint64_t dv_head_stride, uint32_t lddv) {
    if (const int st = refuse_shape("attn_csr_bf16_bwd", D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0 || (!dQ && !dK && !dV)) return MISPMM_OK;
    const bool col_pass = (dK || dV) && K != 0;
    const bool row_pass = dQ || (dK && K != 0);  // dK reads delta
    if (!rowPtrs || !Q || !Kmat || !V || (nnz != 0 && !colIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: rowPtrs, colIdxs, Q, K or V is null");
    if (!out || !lse || !grad_out || (row_pass && !delta))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: out, lse, grad_out or delta is null");
    if (col_pass && (!tRowPtrs || (nnz != 0 && !tColIdxs)))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: dK and dV need the pattern of A^T: tRowPtrs or tColIdxs is null");
    if (col_pass && bias && nnz != 0 && !perm)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: with a bias, dK and dV need perm, which is null");
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv || ldg < Dv || (dQ && lddq < D) || (dK && lddk < D) || (dV && lddv < Dv))
        return fail(MISPMM_ERR_INVALID_ARG,
                    "attn_csr_bf16_bwd: leading dimension smaller than the width (D=%u ldq=%u ldk=%u lddq=%u lddk=%u, Dv=%u ldv=%u ldo=%u ldg=%u lddv=%u)",
                    D, ldq, ldk, lddq, lddk, Dv, ldv, ldo, ldg, lddv);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load: bytes of the element type
    const uint64_t qs = span(M, ldq, D), ks = span(K, ldk, D), vs = span(K, ldv, Dv), os = span(M, ldo, Dv), gs = span(M, ldg, Dv);
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) : 0u;
    const uint64_t lim = 0x7FFFFFFFull;
    if (qs * 2u > lim || ks * 2u > lim || vs * 2u > lim || os * 4u > lim || gs * 2u > lim || bs * 4u > lim)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "attn_csr_bf16_bwd: Q, K, V, out, grad_out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu, %llu bytes)",
                    static_cast<unsigned long long>(qs * 2u), static_cast<unsigned long long>(ks * 2u), static_cast<unsigned long long>(vs * 2u),
                    static_cast<unsigned long long>(os * 4u), static_cast<unsigned long long>(gs * 2u), static_cast<unsigned long long>(bs * 4u));
    const uint64_t d_elem = grads_bf16 ? 2u : 4u, d_mult = grads_bf16 ? 8u : 4u;
    auto mult = [](uint64_t x, uint64_t m) { return x % m == 0; };
    bool wide = D % 8 == 0 && Dv % 8 == 0 && mult(ldq, 8) && mult(ldk, 8) && mult(ldv, 8) && mult(ldg, 8) && mult(ldo, 4) &&
                mult(q_head_stride, 8) && mult(k_head_stride, 8) && mult(v_head_stride, 8) && mult(g_head_stride, 8) &&
                mult(out_head_stride, 4) && aligned16(Q) && aligned16(Kmat) && aligned16(V) && aligned16(out) && aligned16(grad_out);
    wide = wide && (!dQ || (mult(lddq, d_mult) && mult(dq_head_stride, d_mult) && aligned16(dQ))) &&
           (!dK || (mult(lddk, d_mult) && mult(dk_head_stride, d_mult) && aligned16(dK))) &&
           (!dV || (mult(lddv, d_mult) && mult(dv_head_stride, d_mult) && aligned16(dV)));
    const int vec = wide ? 8 : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid("attn_csr_bf16_bwd", M > K ? M : K, H, g); st != MISPMM_OK) return st;
    if (!aligned2(Q) || !aligned2(Kmat) || !aligned2(V) || !aligned2(grad_out) ||
        (grads_bf16 && (!aligned2(dQ) || !aligned2(dK) || !aligned2(dV))))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: Q, K, V, grad_out and bf16 gradients must be 2-byte aligned");
    // an output must not overlap an input, the workspace or another output: extents in bytes of each operand's own type
    const Extent ins[] = {extent(Q, H, q_head_stride, qs, 2),           extent(Kmat, H, k_head_stride, ks, 2),
                          extent(V, H, v_head_stride, vs, 2),           extent(out, H, out_head_stride, os, 4),
                          extent(grad_out, H, g_head_stride, gs, 2),    extent(bias, H, bias_head_stride, bs, 4),
                          extent(lse, 1, 0, static_cast<uint64_t>(H) * M, 4)};
    const Extent outs[] = {extent(dQ, H, dq_head_stride, dQ ? span(M, lddq, D) : 0, d_elem), extent(dK, H, dk_head_stride, dK ? span(K, lddk, D) : 0, d_elem),
                           extent(dV, H, dv_head_stride, dV ? span(K, lddv, Dv) : 0, d_elem),
                           extent(row_pass ? delta : nullptr, 1, 0, static_cast<uint64_t>(H) * M, 4)};
    for (size_t i = 0; i < 4; ++i) {
        for (const Extent &in : ins)
            if (meet(outs[i], in)) return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: dQ, dK, dV or delta overlaps an input");
        for (size_t j = i + 1; j < 4; ++j)
            if (meet(outs[i], outs[j])) return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: dQ, dK, dV and delta overlap one another");
    }
    AbCall c{};
    c.stream = as_stream(stream);
    c.H = H;
    AbParams &p = c.p;
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq2 = ldq * 2u, p.ldk2 = ldk * 2u, p.ldv2 = ldv * 2u, p.ldg2 = ldg * 2u, p.ldo4 = ldo * 4u;
    p.q_bytes = static_cast<uint32_t>(qs * 2u), p.k_bytes = static_cast<uint32_t>(ks * 2u), p.v_bytes = static_cast<uint32_t>(vs * 2u);
    p.g_bytes = static_cast<uint32_t>(gs * 2u), p.o_bytes = static_cast<uint32_t>(os * 4u), p.bias_bytes = static_cast<uint32_t>(bs * 4u);
    p.grads_bf16 = grads_bf16 ? 1u : 0u;
    p.scale = scale;
    p.q_head = q_head_stride, p.k_head = k_head_stride, p.v_head = v_head_stride, p.g_head = g_head_stride, p.o_head = out_head_stride;
    p.bias_head = bias_head_stride;
    AbPtrs &a = c.a;
    a.Q = Q, a.K = Kmat, a.V = V, a.dO = grad_out, a.out = out, a.lse = lse, a.bias = bias, a.delta = delta;
    if (row_pass) {
        p.N = M;
        a.ptrs = rowPtrs, a.idxs = colIdxs, a.perm = nullptr;
        a.d0 = dQ, a.d1 = nullptr;
        p.ldd0 = lddq, p.d0_head = dq_head_stride;
        dispatch_pass<true>(c, vec, g, width);
        MISPMM_LAUNCH_CHECK();
    }
    if (col_pass) {
        p.N = K;
        a.ptrs = tRowPtrs, a.idxs = tColIdxs, a.perm = bias ? perm : nullptr;
        a.d0 = dK, a.d1 = dV;
        p.ldd0 = lddk, p.d0_head = dk_head_stride, p.ldd1 = lddv, p.d1_head = dv_head_stride;
        dispatch_pass<false>(c, vec, g, width);
        MISPMM_LAUNCH_CHECK();
    }
    return MISPMM_OK;
}
