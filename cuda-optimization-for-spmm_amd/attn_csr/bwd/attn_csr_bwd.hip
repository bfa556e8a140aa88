// libmispmm_attn_csr_bwd.so: the backward of fused attention on a CSR pattern in fp32 (include/mispmm_attn_csr_bwd.h) -- dQ, dK
// and dV for all heads in at most two launches.  Scores, weights and their gradients are written nowhere; the only thing that
// goes through memory between the two launches is delta [H][M].
//   z[e]   = fma(scale, <Q_h[r, :D], K_h[c, :D]>, bias_h[e])
//   P[e]   = exp(z[e] - lse_h[r])                 dP[e] = <dO_h[r, :Dv], V_h[c, :Dv]>          delta_h[r] = <dO_h[r], out_h[r]>
//   dS[e]  = scale * P[e] * (dP[e] - delta_h[r])
//   dQ_h[r] = sum over row r of dS[e] K_h[c]      dK_h[c] = sum over column c of dS[e] Q_h[r]  dV_h[c] = sum over column c of P[e] dO_h[r]
//
// Shape: both kernels stand on the lane group of attn_csr/lane_group.hpp, as the forward does (G lanes own one output row,
// batches of 8 entries, the transposing butterfly, the saturating join: explained there).  The two dot products of a batch
// (s and dP) go through the butterfly so that lane i of every 8-lane segment holds entry i's pair, the exponential and dS are
// computed once per entry in that lane, and the 8 results come back by a segment broadcast for the accumulating fmas.
// ROW PASS (A's pattern, a group per (head, row r)): holds Q[r], dO[r] and the dQ accumulator; delta[r] from dO[r] and out[r]
// before the loop (written by lane 0: the column pass reads it); per batch the K rows and the V rows of the entries' columns;
// dQ = fma(dS_i, K[c_i], dQ) from the K rows that are in registers already.
// COLUMN PASS (A^T's pattern, a group per (head, key c)): holds K[c], V[c] and the dK and dV accumulators; per batch the Q rows
// and the dO rows of the entries' rows r_t; lane i reads lse[r_i], delta[r_i] and bias[perm[t_i]] for its own entry.  These
// three depend on the index that is fetched a batch ahead, so they are issued FIRST at the top of the batch, ahead of the 16
// row reads: the vector-memory counter is in order and they have arrived when the rows have.
// s has the same bits in both passes (the same products in the same lane chains and the same tree), hence so do z, P and dS.
// A dead slot's P and dS are replaced by +0.  Every output row has one owner and a fixed order.
#include "../lane_group.hpp"
#include "mispmm_attn_csr_bwd.h"

namespace mispmm {

namespace {

// P of one entry: exp(z - lse) with one rounding of the difference; a row whose lse is not finite is NaN throughout, as a
// softmax over a +Inf, a NaN or nothing but -Inf is (z - (+Inf) alone would give +0)
__device__ __forceinline__ float weight(float z, float lse) {
    return __builtin_fabsf(lse) < __builtin_huge_valf() ? lg_exp(z - lse) : __builtin_nanf("");
}

struct AbParams {
    uint32_t M, N, D, Dv, blocks_per_head, total, xcd_chunk;  // N: rows of the pass's own pattern (M for the row pass, K for the column pass)
    uint32_t ldq4, ldk4, ldv4, ldg4, ldo4;                     // row strides in bytes
    uint32_t ldd0, ldd1;                                       // row strides of the pass's outputs in elements (dQ | dK, dV)
    uint32_t q_bytes, k_bytes, v_bytes, g_bytes, o_bytes, bias_bytes;  // one head's span; bias_bytes == 0: no bias
    float scale;
    uint64_t q_head, k_head, v_head, g_head, o_head, bias_head, d0_head, d1_head;  // elements
};

struct AbPtrs {
    const uint32_t *ptrs, *idxs, *perm;  // the pass's own pattern; perm: column pass with a bias, else null
    const float *Q, *K, *V, *dO, *out, *lse, *bias;
    float *delta;  // written by the row pass, read by the column pass
    float *d0, *d1;  // row pass: dQ, -; column pass: dK, dV; null: not asked for
};

template <int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_bwd_row_kernel(const AbParams p, const AbPtrs a) {
    using vec_t = typename VecOf<VEC>::type;
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scalars sit in the first lanes of a group");
    static_assert(NCH == 1 || G == kWave, "more than one chunk only where a whole wave owns the row");
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
    vec_t xq[NCH], xg[NCH];
    float dsum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        koff[c] = lane_off<G, VEC>(lane, c, p.D);
        voff[c] = lane_off<G, VEC>(lane, c, p.Dv);
        xq[c] = buffer_load_vec<VEC>(qr, join_off(row * p.ldq4, koff[c]), 0);  // past D: zeros
        xg[c] = buffer_load_vec<VEC>(gr, join_off(row * p.ldg4, voff[c]), 0);  // past Dv: zeros
        const vec_t xo = buffer_load_vec<VEC>(orr, join_off(row * p.ldo4, voff[c]), 0);
#pragma unroll
        for (int v = 0; v < VEC; ++v) dsum = __builtin_fmaf(vec_get<VEC>(xg[c], v), vec_get<VEC>(xo, v), dsum);
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
    float *dq_row = a.d0 + static_cast<size_t>(h) * p.d0_head + static_cast<size_t>(row) * p.ldd0;
    // the lane's columns of chunk c are inside D or past it together (VEC == 4: D is a multiple of 4)
    auto store = [&]() {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t col = c * CHUNK + lane * VEC;
            if (col >= p.D) continue;
            vec_t r;
#pragma unroll
            for (int v = 0; v < VEC; ++v) vec_set<VEC>(r, v, dq[c][v]);
            store_vec<VEC>(dq_row + col, r);
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
        const uint32_t kkey = nxt_col * p.ldk4 | dead;
        const uint32_t vkey = nxt_col * p.ldv4 | dead;
        const float b = nxt_bias;
        fetch(s0 + E, nxt_col, nxt_bias);  // on its way while this batch is gathered
        __builtin_amdgcn_sched_barrier(0);  // ... issued here, ahead of the batch's own reads (see the end of the loop body)
        vec_t kv[E][NCH], vv[E][NCH];
        gather_rows<VEC, NCH>(kkey, kr, koff, kv);
        gather_rows<VEC, NCH>(vkey, vr, voff, vv);
        float acc_s[E], acc_p[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc_s[j] = 0.f;
            acc_p[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                acc_s[j] = dot_chain<VEC>(xq[c], kv[j][c], acc_s[j]);
                acc_p[j] = dot_chain<VEC>(xg[c], vv[j][c], acc_p[j]);
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
                for (int v = 0; v < VEC; ++v) dq[c][v] = __builtin_fmaf(dj, vec_get<VEC>(kv[j][c], v), dq[c][v]);
        });
        // the next batch's column and bias must be in their registers HERE (attn_csr.hip): otherwise the fetch moves over the
        // loop edge to the top of the batch that uses it
        asm volatile("" : "+v"(nxt_col), "+v"(nxt_bias));
    }
    store();
}

template <int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_bwd_col_kernel(const AbParams p, const AbPtrs a) {
    using vec_t = typename VecOf<VEC>::type;
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scalars sit in the first lanes of a group");
    static_assert(NCH == 1 || G == kWave, "more than one chunk only where a whole wave owns the row");
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
            vec_t r;
            if (want_dk && col < p.D) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) vec_set<VEC>(r, v, dk[c][v]);
                store_vec<VEC>(a.d0 + static_cast<size_t>(h) * p.d0_head + static_cast<size_t>(key) * p.ldd0 + col, r);
            }
            if (want_dv && col < p.Dv) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) vec_set<VEC>(r, v, dv[c][v]);
                store_vec<VEC>(a.d1 + static_cast<size_t>(h) * p.d1_head + static_cast<size_t>(key) * p.ldd1 + col, r);
            }
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
    vec_t xk[NCH], xv[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        qoff[c] = lane_off<G, VEC>(lane, c, p.D);
        goff[c] = lane_off<G, VEC>(lane, c, p.Dv);
        xk[c] = buffer_load_vec<VEC>(kr, join_off(key * p.ldk4, qoff[c]), 0);  // past D: zeros
        xv[c] = buffer_load_vec<VEC>(vr, join_off(key * p.ldv4, goff[c]), 0);  // past Dv: zeros; read only for dP
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
        const uint32_t qkey = r * p.ldq4 | dead;
        const uint32_t gkey = r * p.ldg4 | dead;
        const uint32_t e_a = nxt_e;
        fetch(s0 + E, nxt_r, nxt_e);
        __builtin_amdgcn_sched_barrier(0);
        // the entry's own scalars first: they are behind the rows in no queue
        const float lse = lse_h[r];
        const float delta = want_dk ? delta_h[r] : 0.f;
        const float b = buffer_load_vec<1>(br, e_a * 4u, 0);
        vec_t qv[E][NCH], gv[E][NCH];
        gather_rows<VEC, NCH>(qkey, qr, qoff, qv);
        gather_rows<VEC, NCH>(gkey, gr, goff, gv);
        float acc_s[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc_s[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                acc_s[j] = dot_chain<VEC>(qv[j][c], xk[c], acc_s[j]);
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
                    for (int v = 0; v < VEC; ++v) dv[c][v] = __builtin_fmaf(wj, vec_get<VEC>(gv[j][c], v), dv[c][v]);
            });
        }
        if (want_dk) {
            float acc_p[E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                acc_p[j] = 0.f;
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    acc_p[j] = dot_chain<VEC>(gv[j][c], xv[c], acc_p[j]);
            }
            const float dp = transpose_sum<G>(acc_p, lane);
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
                    for (int v = 0; v < VEC; ++v) dk[c][v] = __builtin_fmaf(dj, vec_get<VEC>(qv[j][c], v), dk[c][v]);
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
        note_kernel("attn_csr_bwd_row<f32,G%d,V%d,C%d>", G, VEC, NCH);
        hipLaunchKernelGGL((attn_csr_bwd_row_kernel<G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.a);
    } else {
        note_kernel("attn_csr_bwd_col<f32,G%d,V%d,C%d>", G, VEC, NCH);
        hipLaunchKernelGGL((attn_csr_bwd_col_kernel<G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.a);
    }
}

template <bool ROW>
void dispatch_pass(const AbCall &c, int vec, int g, uint32_t width) {
    with_instance(vec, g, width, [&](auto gr, auto v, auto ch) { launch_pass<ROW, decltype(gr)::value, decltype(v)::value, decltype(ch)::value>(c); });
}

struct Extent {
    const char *lo, *hi;
};
// bytes H heads of an operand cover (a head stride of 0: one head's)
Extent extent(const float *base, uint32_t H, uint64_t head_stride, uint64_t head_span) {
    const char *lo = reinterpret_cast<const char *>(base);
    return {lo, base && head_span ? lo + ((H - 1) * head_stride + head_span) * 4u : lo};
}
bool meet(const Extent &x, const Extent &y) { return x.lo < y.hi && y.lo < x.hi; }

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_attn_csr_bwd_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                       const uint32_t *colIdxs, const uint32_t *tRowPtrs, const uint32_t *tColIdxs, const uint32_t *perm,
                                       const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat, uint64_t k_head_stride,
                                       uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv, uint32_t Dv,
                                       float scale, const float *bias, uint64_t bias_head_stride, const float *out,
                                       uint64_t out_head_stride, uint32_t ldo, const float *lse, const float *grad_out,
                                       uint64_t g_head_stride, uint32_t ldg, float *delta, float *dQ, uint64_t dq_head_stride,
                                       uint32_t lddq, float *dK, uint64_t dk_head_stride, uint32_t lddk, float *dV,
                                       uint64_t dv_head_stride, uint32_t lddv) {
    if (const int st = refuse_shape("attn_csr_bwd_f32", D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0 || (!dQ && !dK && !dV)) return MISPMM_OK;
    const bool col_pass = (dK || dV) && K != 0;
    const bool row_pass = dQ || (dK && K != 0);  // dK reads delta
    if (!rowPtrs || !Q || !Kmat || !V || (nnz != 0 && !colIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: rowPtrs, colIdxs, Q, K or V is null");
    if (!out || !lse || !grad_out || (row_pass && !delta))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: out, lse, grad_out or delta is null");
    if (col_pass && (!tRowPtrs || (nnz != 0 && !tColIdxs)))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: dK and dV need the pattern of A^T: tRowPtrs or tColIdxs is null");
    if (col_pass && bias && nnz != 0 && !perm)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: with a bias, dK and dV need perm, which is null");
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv || ldg < Dv || (dQ && lddq < D) || (dK && lddk < D) || (dV && lddv < Dv))
        return fail(MISPMM_ERR_INVALID_ARG,
                    "attn_csr_bwd_f32: leading dimension smaller than the width (D=%u ldq=%u ldk=%u lddq=%u lddk=%u, Dv=%u ldv=%u ldo=%u ldg=%u lddv=%u)",
                    D, ldq, ldk, lddq, lddk, Dv, ldv, ldo, ldg, lddv);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    const uint64_t qs = span(M, ldq, D), ks = span(K, ldk, D), vs = span(K, ldv, Dv), os = span(M, ldo, Dv), gs = span(M, ldg, Dv);
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) : 0u;
    const uint64_t lim = 0x7FFFFFFFull / 4u;
    if (qs > lim || ks > lim || vs > lim || os > lim || gs > lim || bs > lim)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "attn_csr_bwd_f32: Q, K, V, out, grad_out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu, %llu bytes)",
                    static_cast<unsigned long long>(qs * 4u), static_cast<unsigned long long>(ks * 4u), static_cast<unsigned long long>(vs * 4u),
                    static_cast<unsigned long long>(os * 4u), static_cast<unsigned long long>(gs * 4u), static_cast<unsigned long long>(bs * 4u));
    auto mult4 = [](uint64_t x) { return x % 4 == 0; };
    bool wide = D % 4 == 0 && Dv % 4 == 0 && mult4(ldq) && mult4(ldk) && mult4(ldv) && mult4(ldo) && mult4(ldg) && mult4(q_head_stride) &&
                mult4(k_head_stride) && mult4(v_head_stride) && mult4(out_head_stride) && mult4(g_head_stride) && aligned16(Q) &&
                aligned16(Kmat) && aligned16(V) && aligned16(out) && aligned16(grad_out);
    wide = wide && (!dQ || (mult4(lddq) && mult4(dq_head_stride) && aligned16(dQ))) && (!dK || (mult4(lddk) && mult4(dk_head_stride) && aligned16(dK))) &&
           (!dV || (mult4(lddv) && mult4(dv_head_stride) && aligned16(dV)));
    const int vec = wide ? 4 : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid("attn_csr_bwd_f32", M > K ? M : K, H, g); st != MISPMM_OK) return st;
    // an output must not overlap an input, the workspace or another output
    const Extent ins[] = {extent(Q, H, q_head_stride, qs),           extent(Kmat, H, k_head_stride, ks), extent(V, H, v_head_stride, vs),
                          extent(out, H, out_head_stride, os),       extent(grad_out, H, g_head_stride, gs), extent(bias, H, bias_head_stride, bs),
                          extent(lse, 1, 0, static_cast<uint64_t>(H) * M)};
    const Extent outs[] = {extent(dQ, H, dq_head_stride, dQ ? span(M, lddq, D) : 0), extent(dK, H, dk_head_stride, dK ? span(K, lddk, D) : 0),
                           extent(dV, H, dv_head_stride, dV ? span(K, lddv, Dv) : 0), extent(row_pass ? delta : nullptr, 1, 0, static_cast<uint64_t>(H) * M)};
    for (size_t i = 0; i < 4; ++i) {
        for (const Extent &in : ins)
            if (meet(outs[i], in)) return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: dQ, dK, dV or delta overlaps an input");
        for (size_t j = i + 1; j < 4; ++j)
            if (meet(outs[i], outs[j])) return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: dQ, dK, dV and delta overlap one another");
    }
    AbCall c{};
    c.stream = as_stream(stream);
    c.H = H;
    AbParams &p = c.p;
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq4 = ldq * 4u, p.ldk4 = ldk * 4u, p.ldv4 = ldv * 4u, p.ldg4 = ldg * 4u, p.ldo4 = ldo * 4u;
    p.q_bytes = static_cast<uint32_t>(qs * 4u), p.k_bytes = static_cast<uint32_t>(ks * 4u), p.v_bytes = static_cast<uint32_t>(vs * 4u);
    p.g_bytes = static_cast<uint32_t>(gs * 4u), p.o_bytes = static_cast<uint32_t>(os * 4u), p.bias_bytes = static_cast<uint32_t>(bs * 4u);
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
