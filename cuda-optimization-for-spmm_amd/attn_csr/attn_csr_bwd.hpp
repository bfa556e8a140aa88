// The two backward kernels of the fused attention on a CSR pattern, written once over the element policy of elem.hpp and
// instantiated by bwd/attn_csr_bwd.hip (ElemF32: 10 + 10 instances) and attn_csr_bf16/bwd/attn_csr_bf16_bwd.hip (ElemBf16:
// 9 + 9) -- dQ, dK and dV for all heads in at most two launches, fp32 arithmetic (bf16 operands exactly widened, no fp32 copy of
// any operand).  Scores, weights and their gradients are written nowhere; the only thing that goes through memory between the
// two launches is delta [H][M].
//   z[e]   = fma(scale, <Q_h[r, :D], K_h[c, :D]>, bias_h[e])
//   P[e]   = exp(z[e] - lse_h[r])                 dP[e] = <dO_h[r, :Dv], V_h[c, :Dv]>          delta_h[r] = <dO_h[r], out_h[r]>
//   dS[e]  = scale * P[e] * (dP[e] - delta_h[r])
//   dQ_h[r] = sum over row r of dS[e] K_h[c]      dK_h[c] = sum over column c of dS[e] Q_h[r]  dV_h[c] = sum over column c of P[e] dO_h[r]
//
// Shape: both kernels stand on the lane group of lane_group.hpp, as the forward does (G lanes own one output row, batches of 8
// entries, the transposing butterfly, the saturating join: explained there).  The two dot products of a batch (s and dP) go
// through the butterfly so that lane i of every 8-lane segment holds entry i's pair, the exponential and dS are computed once
// per entry in that lane, and the 8 results come back by a segment broadcast for the accumulating fmas.  Every dot product is
// ONE fma chain per lane from +0, columns ascending -- for bf16 on the widened values, no packed dot instruction.
// ROW PASS (A's pattern, a group per (head, row r)): holds Q[r], dO[r] and the dQ accumulator; delta[r] from dO[r] and out[r]
// before the loop (written by lane 0: the column pass reads it); per batch the K rows and the V rows of the entries' columns;
// dQ = fma(dS_i, K[c_i], dQ) from the K rows that are in registers already.
// COLUMN PASS (A^T's pattern, a group per (head, key c)): holds K[c], V[c] and the dK and dV accumulators; per batch the Q rows
// and the dO rows of the entries' rows r_t; lane i reads lse[r_i], delta[r_i] and bias[perm[t_i]] for its own entry.  These
// three depend on the index that is fetched a batch ahead, so they are issued FIRST at the top of the batch, ahead of the 16
// row reads: the vector-memory counter is in order and they have arrived when the rows have.
// s has the same bits in both passes (the same products in the same lane chains and the same tree), hence so do z, P and dS.
// A dead slot's P and dS are replaced by +0.  Every output row has one owner and a fixed order.
// out and lse are fp32 for either element type (the bf16 forward wrote them so); out[r] is read once per row for delta.  The
// gradients of bf16 operands are fp32, or the same accumulators rounded once (a wave-uniform branch: no instances of its own).
// On V1 a bf16 lane's chains are the fp32 V1 chains on the widened values: every output has that kernel's bits.  On V8 a
// lane's chain covers 8 columns against 4.
#pragma once
#include "elem.hpp"

namespace mispmm {

namespace {

// the kernels' parameter block, one per element type so that each keeps its kernel-argument offsets.  N: rows of the pass's
// own pattern (M for the row pass, K for the column pass); ldq .. ldo: row strides in bytes (out is fp32); ldd0, ldd1: row
// strides of the pass's outputs in elements (dQ | dK, dV); the spans are one head's, bias_bytes == 0: no bias; head strides
// in elements
template <class Elem> struct BwdParams;
template <> struct BwdParams<ElemF32> {
    uint32_t M, N, D, Dv, blocks_per_head, total, xcd_chunk;
    uint32_t ldq, ldk, ldv, ldg, ldo;
    uint32_t ldd0, ldd1;
    uint32_t q_bytes, k_bytes, v_bytes, g_bytes, o_bytes, bias_bytes;
    float scale;
    uint64_t q_head, k_head, v_head, g_head, o_head, bias_head, d0_head, d1_head;
    static constexpr bool narrow = false;
};
template <> struct BwdParams<ElemBf16> {
    uint32_t M, N, D, Dv, blocks_per_head, total, xcd_chunk;
    uint32_t ldq, ldk, ldv, ldg, ldo;
    uint32_t ldd0, ldd1;
    uint32_t q_bytes, k_bytes, v_bytes, g_bytes, o_bytes, bias_bytes;
    uint32_t narrow;  // the gradients are bf16
    float scale;
    uint64_t q_head, k_head, v_head, g_head, o_head, bias_head, d0_head, d1_head;
};

template <class Elem>
struct BwdPtrs {
    const uint32_t *ptrs, *idxs, *perm;  // the pass's own pattern; perm: column pass with a bias, else null
    const typename Elem::in_t *Q, *K, *V, *dO;
    const float *out, *lse, *bias;
    float *delta;  // written by the row pass, read by the column pass
    typename Elem::out_t *d0, *d1;  // row pass: dQ, -; column pass: dK, dV; null: not asked for
};

// the VEC gradient columns of accumulator `acc` to `at`: fp32, or the same values rounded once (`narrow` is wave-uniform).
// How the accumulator gets here is what each element type's instances had, and either way moves the other's registers: the
// fp32 values are copied out first, where the call stands, and meet no branch (not even one on a constant that the optimiser
// folds later: with either, the empty row's store and the last one of a V4 pass are no longer merged into one block); the
// bf16 ones are read in place.  A macro because every function tried in its place is one of the forms that move something
// (DESIGN.md section 9 item 22).  The forward spells its branch out in its own store: behind a helper the blocks of the bf16
// V1 epilogue change places
#define MISPMM_STORE_GRAD(base, at, acc)                                                               \
    do {                                                                                               \
        if constexpr (Elem::kWidens) {                                                                 \
            store_grad_bf16<Elem, VEC>(base, at, acc, p.narrow != 0);                                  \
        } else {                                                                                       \
            float r_[VEC];                                                                             \
            _Pragma("unroll") for (int v = 0; v < VEC; ++v) r_[v] = (acc)[v];                          \
            store_f32<VEC>(Elem::template ptr<float>(base, at), r_);                                   \
        }                                                                                              \
    } while (0)
template <class Elem, int VEC>
__device__ __forceinline__ void store_grad_bf16(typename Elem::out_t *base, typename Elem::row_t at, const float *r, bool narrow) {
    if (narrow) store_bf16<VEC>(Elem::template ptr<uint16_t>(base, at), r);
    else store_f32<VEC>(Elem::template ptr<float>(base, at), r);
}

template <class Elem, int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_bwd_row_kernel(const BwdParams<Elem> p, const BwdPtrs<Elem> a) {
    using raw_t = typename Elem::template raw_t<VEC>;
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scalars sit in the first lanes of a group");
    static_assert(Elem::template fits<G, VEC, NCH>, "no such lane width or chunk count for this element type");
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
    typename Elem::template held_t<VEC> xq[NCH], xg[NCH];  // Q[r]'s and dO[r]'s slices
    float dsum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        koff[c] = Elem::template lane_off<G, VEC>(lane, c, p.D);
        voff[c] = Elem::template lane_off<G, VEC>(lane, c, p.Dv);
        const raw_t qraw = Elem::template load<VEC>(qr, join_off(row * p.ldq, koff[c]));  // past D: zeros
        const raw_t graw = Elem::template load<VEC>(gr, join_off(row * p.ldg, voff[c]));  // past Dv: zeros
        // (spelled out per element type, as the forward's hold of Q[r] is: see there)
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
    const size_t hr = static_cast<size_t>(h) * p.M + row;
    if (lane == 0) a.delta[hr] = delta;
    if (!a.d0) return;  // dQ is not asked for: the pass was launched for delta

    float dq[NCH][VEC];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) dq[c][v] = 0.f;
    const typename Elem::row_t dq_row = Elem::row_of(a.d0, h, p.d0_head, row, p.ldd0);
    // the lane's columns of chunk c are inside D or past it together (wide lanes: D is a multiple of the lane width)
    auto store = [&]() {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t col = c * CHUNK + lane * VEC;
            if (col >= p.D) continue;
            MISPMM_STORE_GRAD(a.d0, dq_row + col, dq[c]);
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
        ds = ds * p.scale;
        ds = live ? ds : 0.f;
        static_for<0, E>([&](auto j_tag) {
            constexpr int j = decltype(j_tag)::value;
            const float dj = __uint_as_float(group_bcast<8, j>(__float_as_uint(ds)));
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v) dq[c][v] = __builtin_fmaf(dj, Elem::template at<VEC>(kv[j][c], v), dq[c][v]);
        });
        // the next batch's column and bias must be in their registers HERE (attn_csr_fwd.hpp): otherwise the fetch moves over
        // the loop edge to the top of the batch that uses it
        asm volatile("" : "+v"(nxt_col), "+v"(nxt_bias));
    }
    store();
}

template <class Elem, int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_bwd_col_kernel(const BwdParams<Elem> p, const BwdPtrs<Elem> a) {
    using raw_t = typename Elem::template raw_t<VEC>;
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scalars sit in the first lanes of a group");
    static_assert(Elem::template fits<G, VEC, NCH>, "no such lane width or chunk count for this element type");
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
            if (want_dk && col < p.D) MISPMM_STORE_GRAD(a.d0, Elem::row_of(a.d0, h, p.d0_head, key, p.ldd0) + col, dk[c]);
            if (want_dv && col < p.Dv) MISPMM_STORE_GRAD(a.d1, Elem::row_of(a.d1, h, p.d1_head, key, p.ldd1) + col, dv[c]);
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
    typename Elem::template held_t<VEC> xk[NCH], xv[NCH];  // K[c]'s and V[c]'s slices
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        qoff[c] = Elem::template lane_off<G, VEC>(lane, c, p.D);
        goff[c] = Elem::template lane_off<G, VEC>(lane, c, p.Dv);
        const raw_t kraw = Elem::template load<VEC>(kr, join_off(key * p.ldk, qoff[c]));  // past D: zeros
        const raw_t vraw = Elem::template load<VEC>(vr, join_off(key * p.ldv, goff[c]));  // past Dv: zeros; read only for dP
        if constexpr (Elem::kWidens) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) xk[c][v] = Elem::template at<VEC>(kraw, v), xv[c][v] = Elem::template at<VEC>(vraw, v);
        } else {
            xk[c] = kraw;
            xv[c] = vraw;
        }
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
        const uint32_t qkey = r * p.ldq | dead;
        const uint32_t gkey = r * p.ldg | dead;
        const uint32_t e_a = nxt_e;
        fetch(s0 + E, nxt_r, nxt_e);
        __builtin_amdgcn_sched_barrier(0);
        // the entry's own scalars first: they are behind the rows in no queue
        const float lse = lse_h[r];
        const float delta = want_dk ? delta_h[r] : 0.f;
        const float b = buffer_load_vec<1>(br, e_a * 4u, 0);
        raw_t qv[E][NCH], gv[E][NCH];
        Elem::template gather<VEC, NCH>(qkey, qr, qoff, qv);
        Elem::template gather<VEC, NCH>(gkey, gr, goff, gv);
        float acc_s[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc_s[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    acc_s[j] = __builtin_fmaf(Elem::template at<VEC>(qv[j][c], v), Elem::template held<VEC>(xk[c], v), acc_s[j]);
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
                    for (int v = 0; v < VEC; ++v) dv[c][v] = __builtin_fmaf(wj, Elem::template at<VEC>(gv[j][c], v), dv[c][v]);
            });
        }
        if (want_dk) {
            // bf16, wide lanes: the rows stay in their 64 loaded registers, each element is widened again where it is used a
            // second time.  Without these statements the compiler keeps all 128 widened floats of a batch alive from their first
            // use to their second (192 VGPRs and 2 waves per SIMD at V8; 1 instruction per element is what the second widening
            // costs)
            constexpr bool REWIDEN = Elem::kWidens && VEC == Elem::kWide;
            if constexpr (REWIDEN) {
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
                    for (int v = 0; v < VEC; ++v)
                        acc_p[j] = __builtin_fmaf(Elem::template at<VEC>(gv[j][c], v), Elem::template held<VEC>(xv[c], v), acc_p[j]);
            }
            const float dp = transpose_sum<G>(acc_p, lane);
            float ds = dp - delta;
            ds = w * ds;
            ds = ds * p.scale;
            ds = live ? ds : 0.f;
            if constexpr (REWIDEN) {
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
                    for (int v = 0; v < VEC; ++v) dk[c][v] = __builtin_fmaf(dj, Elem::template at<VEC>(qv[j][c], v), dk[c][v]);
            });
        }
        asm volatile("" : "+v"(nxt_r), "+v"(nxt_e));
    }
    store();
}

#undef MISPMM_STORE_GRAD

// what an entry point hands to its launches
template <class Elem>
struct BwdCall {
    hipStream_t stream;
    uint32_t H;
    BwdParams<Elem> p;
    BwdPtrs<Elem> a;
};

// `tag`: the library's own note_kernel format of the pass, with G, VEC and NCH to fill in
template <class Elem, bool ROW, int G, int VEC, int NCH>
void launch_pass(const BwdCall<Elem> &c, const char *tag) {
    BwdParams<Elem> p = c.p;
    const uint32_t grid = finish_grid<G>(p, p.N, c.H);
    note_kernel(tag, G, VEC, NCH);
    if constexpr (ROW) hipLaunchKernelGGL((attn_csr_bwd_row_kernel<Elem, G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.a);
    else hipLaunchKernelGGL((attn_csr_bwd_col_kernel<Elem, G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.a);
}

template <class Elem, bool ROW>
void dispatch_pass(const BwdCall<Elem> &c, int vec, int g, uint32_t width, const char *tag) {
    Elem::with_instance(vec, g, width, [&](auto gr, auto v, auto ch) {
        launch_pass<Elem, ROW, decltype(gr)::value, decltype(v)::value, decltype(ch)::value>(c, tag);
    });
}

}  // namespace

}  // namespace mispmm
