// The bias gradient of the fused attention on a CSR pattern, written once over the element policy of elem.hpp and instantiated
// by attn_csr_dbias/attn_csr_dbias.hip for both element types (ElemF32: 10 instances, ElemBf16: 9) -- one launch for all heads,
// fp32 arithmetic (bf16 operands exactly widened), nothing but dBias written.
//   z[e]   = fma(scale, <Q_h[r, :D], K_h[c, :D]>, bias_h[e])
//   P[e]   = exp(z[e] - lse_h[r])                 dP[e] = <dO_h[r, :Dv], V_h[c, :Dv]>          delta_h[r] = <dO_h[r], out_h[r]>
//   dBias_h[e] = P[e] * (dP[e] - delta_h[r])                                              (dz / dbias = 1: no scale)
//
// Shape: the ROW PASS of attn_csr_bwd.hpp without its dQ accumulator, on the lane group of lane_group.hpp: a group per
// (head, row r) of A's pattern holds Q[r] and dO[r]; delta[r] from dO[r] and out[r] before the loop, by the same chain and the
// same tree, kept in a register (the `delta` workspace of the backward is neither read nor written: the kernel runs alone and in
// any order relative to the backward); per batch the K rows and the V rows of the entries' columns, s and dP through the
// butterfly, then in the lane that holds entry i: z, weight(z, lse) and ds = fl(P * fl(dP - delta)) -- the row pass's ds BEFORE
// its last multiply by the scale, so fl(dBias * scale) is the row pass's dS bit for bit.  Every 8-lane segment of the group
// holds the same 8 values; the FIRST segment stores them (lane i entry s0 + i, live slots only), one 4-byte store per entry.
// An empty row stores nothing.  The fetch of the next batch's column and bias stands where the row pass has it.
// No LDS, no atomics, no scratch; every entry has one owner; a head's result does not depend on H.
#pragma once
#include "elem.hpp"

namespace mispmm {

namespace {

// the kernel's parameter block.  ldq .. ldo: row strides in bytes (out is fp32); the spans are one head's, bias_bytes == 0: no
// bias; head strides in elements
struct DbiasParams {
    uint32_t M, D, Dv, blocks_per_head, total, xcd_chunk;
    uint32_t ldq, ldk, ldv, ldg, ldo;
    uint32_t q_bytes, k_bytes, v_bytes, g_bytes, o_bytes, bias_bytes;
    float scale;
    uint64_t q_head, k_head, v_head, g_head, o_head, bias_head, dbias_head;
};

template <class Elem>
struct DbiasPtrs {
    const uint32_t *ptrs, *idxs;  // A's pattern
    const typename Elem::in_t *Q, *K, *V, *dO;
    const float *out, *lse, *bias;
    float *dbias;
};

template <class Elem, int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_dbias_kernel(const DbiasParams p, const DbiasPtrs<Elem> a) {
    using raw_t = typename Elem::template raw_t<VEC>;
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scalars sit in the first lanes of a group");
    static_assert(Elem::template fits<G, VEC, NCH>, "no such lane width or chunk count for this element type");
    constexpr int GROUPS = kLgBlock / G, E = kLgBatch;
    const uint32_t lane = threadIdx.x % G, sub = lane & (E - 1);
    const uint32_t item = xcd_block(blockIdx.x, p.xcd_chunk);
    if (item >= p.total) return;
    const uint32_t h = item / p.blocks_per_head;  // wave-uniform: a workgroup lies inside one head
    const uint64_t row64 = static_cast<uint64_t>(item - h * p.blocks_per_head) * GROUPS + threadIdx.x / G;
    if (row64 >= p.M) return;  // the lanes a move reads from are all in the lane's own group, which leaves as one
    const uint32_t row = static_cast<uint32_t>(row64);
    const uint32_t base = a.ptrs[row];
    const uint32_t len = a.ptrs[row + 1] - base;
    if (len == 0) return;  // an empty row has no entry

    const rsrc_t qr = make_rsrc(a.Q + h * p.q_head, p.q_bytes), kr = make_rsrc(a.K + h * p.k_head, p.k_bytes);
    const rsrc_t vr = make_rsrc(a.V + h * p.v_head, p.v_bytes), gr = make_rsrc(a.dO + h * p.g_head, p.g_bytes);
    const rsrc_t orr = make_rsrc(a.out + h * p.o_head, p.o_bytes);
    const rsrc_t br = make_rsrc(a.bias ? a.bias + h * p.bias_head : nullptr, p.bias_bytes);  // spans nothing without a bias: reads give +0
    uint32_t koff[NCH], voff[NCH];
    typename Elem::template held_t<VEC> xq[NCH], xg[NCH];  // Q[r]'s and dO[r]'s slices
    float dsum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        koff[c] = Elem::template lane_off<G, VEC>(lane, c, p.D);
        voff[c] = Elem::template lane_off<G, VEC>(lane, c, p.Dv);
        const raw_t qraw = Elem::template load<VEC>(qr, join_off(row * p.ldq, koff[c]));  // past D: zeros
        const raw_t graw = Elem::template load<VEC>(gr, join_off(row * p.ldg, voff[c]));  // past Dv: zeros
        if constexpr (Elem::kWidens) {
            // out is fp32: the same columns at 4 bytes each (twice the bf16 offset; the mark stays the mark)
            const uint32_t ooff = join_off(row * p.ldo, join_off(voff[c], voff[c]));
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
                xq[c][v] = Elem::template at<VEC>(qraw, v);
                xg[c][v] = Elem::template at<VEC>(graw, v);
                dsum = __builtin_fmaf(xg[c][v], xo[v], dsum);
            }
        } else {
            xq[c] = qraw;
            xg[c] = graw;
            const raw_t xo = buffer_load_vec<VEC>(orr, join_off(row * p.ldo, voff[c]), 0);
#pragma unroll
            for (int v = 0; v < VEC; ++v) dsum = __builtin_fmaf(vec_get<VEC>(xg[c], v), vec_get<VEC>(xo, v), dsum);
        }
    }
    const float delta = group_all_reduce<G>(dsum, [](float x, float y) { return x + y; });  // lanes 1, 2, 4, ... apart: the same bits in every lane
    const float lse = a.lse[static_cast<size_t>(h) * p.M + row];
    float *const to = a.dbias + static_cast<size_t>(h) * p.dbias_head + base;  // the row's entries of this head
    // entry c0 + sub of the row and its bias: every 8-lane segment of the group holds the batch's 8 entries.  A slot past the
    // row end re-reads the row's first entry (it exists: len > 0); what it yields is stored nowhere.
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
        // the mark is OR-ed in, not selected (attn_csr_fwd.hpp: a select lets the compiler sink the fetch into a branch on `live`)
        const uint32_t dead = live ? 0u : kDropLoad;
        const uint32_t kkey = nxt_col * p.ldk | dead;
        const uint32_t vkey = nxt_col * p.ldv | dead;
        const float b = nxt_bias;
        fetch(s0 + E, nxt_col, nxt_bias);  // on its way while this batch is gathered
        __builtin_amdgcn_sched_barrier(0);  // ... issued here, ahead of the batch's own reads (see the end of the loop body)
        raw_t kv[E][NCH], vv[E][NCH];
        Elem::template gather<VEC, NCH>(kkey, kr, koff, kv);
        Elem::template gather<VEC, NCH>(vkey, vr, voff, vv);
        float acc_s[E], acc_p[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc_s[j] = 0.f;
            acc_p[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    acc_s[j] = __builtin_fmaf(Elem::template held<VEC>(xq[c], v), Elem::template at<VEC>(kv[j][c], v), acc_s[j]);
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    acc_p[j] = __builtin_fmaf(Elem::template held<VEC>(xg[c], v), Elem::template at<VEC>(vv[j][c], v), acc_p[j]);
            }
        }
        const float s = transpose_sum<G>(acc_s, lane);
        const float dp = transpose_sum<G>(acc_p, lane);
        // lane (any segment, position sub) now holds s and dP of entry s0 + sub
        const float z = __builtin_fmaf(p.scale, s, b);
        const float w = weight(z, lse);
        float ds = dp - delta;
        ds = w * ds;
        // the first segment stores: lane == sub there, and a dead slot has no entry of this row (the word after the row's last
        // is the next row's first)
        if (live && lane < E) to[s0 + sub] = ds;
        // the next batch's column and bias must be in their registers HERE (attn_csr_fwd.hpp): otherwise the fetch moves over
        // the loop edge to the top of the batch that uses it
        asm volatile("" : "+v"(nxt_col), "+v"(nxt_bias));
    }
}

// what an entry point hands to its launch
template <class Elem>
struct DbiasCall {
    hipStream_t stream;
    uint32_t H;
    DbiasParams p;
    DbiasPtrs<Elem> a;
};

// `tag`: the note_kernel format, with G, VEC and NCH to fill in
template <class Elem>
void dispatch_dbias(const DbiasCall<Elem> &c, int vec, int g, uint32_t width, const char *tag) {
    Elem::with_instance(vec, g, width, [&](auto gr, auto v, auto ch) {
        constexpr int G = decltype(gr)::value, VEC = decltype(v)::value, NCH = decltype(ch)::value;
        DbiasParams p = c.p;
        const uint32_t grid = finish_grid<G>(p, p.M, c.H);
        note_kernel(tag, G, VEC, NCH);
        hipLaunchKernelGGL((attn_csr_dbias_kernel<Elem, G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.a);
    });
}

}  // namespace

}  // namespace mispmm
