// libmispmm_attn_csr.so: fused attention on a CSR pattern in fp32 (include/mispmm_attn_csr.h) -- scores, row softmax and the
// product with V in ONE launch for all heads.  Neither the scores nor the weights are written; per row only out and, where
// asked for, a log-sum-exp.
//   z[e]      = fma(scale, <Q_h[r, :D], K_h[c, :D]>, bias_h[e])          c = colIdxs[e], e over the stored entries of row r
//   out_h[r]  = sum_e softmax_e(z) * V_h[c, :Dv]
//
// Shape: the two halves are those of csrc/sddmm.hip and csrc/row_gather.hpp, in the lane group of lane_group.hpp (G lanes per
// (head, row), batches of 8 entries, the transposing butterfly, the saturating join of dropped offsets: all explained there).
// A lane holds its slice of Q[r] and of the fp32 accumulator O.  A batch's 8 x NCH K-row reads and 8 x NCH V-row reads are
// issued together, the K reads first: the vector-memory counter is in order, so the dot products wait for K alone and V
// arrives under them and under the softmax arithmetic.  The column keys (and the bias) of a batch are fetched one batch ahead.
// V is NOT fetched a batch ahead: a second register stage of 8 x NCH vectors would double the kernel's largest array for a
// latency the K-side arithmetic already covers.
// Online softmax per batch: the batch maximum over the 8 lanes of a segment (3 moves), folded into the running maximum m;
// mu = m with an infinite m replaced by 0 (what torch.logsumexp subtracts); alpha = exp(mu_old - mu_new), exactly 1 while m
// is still -Inf; one v_exp_f32 per lane for the weight; the 8 weights are summed by a fixed tree over the segment (3 moves)
// into l = fl(fl(l * alpha) + t) and reach the group by DPP row_newbcast for O = fl(alpha * O), then O = fma(w_i, V[c_i], O)
// for i = 0..7.  Every lane of the group holds the same alpha bits, so O and l are scaled by the same number.
// After the row: out = O / l (an IEEE division per element), lse = mu + log l.
// A dead slot's score is replaced by -Inf before the maximum: its weight is exp2(-Inf) = +0.
// The bias is read through a descriptor of its own that spans nothing where there is no bias: every read then returns +0
// and no branch stands in the loop.  Run to run identical.
// The sources lie outside csrc/, fused/ and rows_bf16/: the census tests hold those directories and their libraries to their
// records.
#include "lane_group.hpp"
#include "mispmm_attn_csr.h"

namespace mispmm {

namespace {

struct AcParams {
    uint32_t M, D, Dv, blocks_per_head, total, xcd_chunk;
    uint32_t ldq, ldk4, ldv4, ldo;                    // ldk4, ldv4: row strides in bytes
    uint32_t q_bytes, k_bytes, v_bytes, bias_bytes;   // one head's span; bias_bytes == 0: no bias
    float scale;
    uint64_t q_head, k_head, v_head, o_head, bias_head;  // elements
};

template <int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_kernel(const AcParams p, const uint32_t *__restrict__ rowPtrs,
                                                            const uint32_t *__restrict__ colIdxs, const float *__restrict__ Q,
                                                            const float *__restrict__ K, const float *__restrict__ V,
                                                            const float *__restrict__ bias, float *__restrict__ out,
                                                            float *__restrict__ lse_out) {
    using vec_t = typename VecOf<VEC>::type;
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scores sit in the first lanes of a group");
    static_assert(NCH == 1 || G == kWave, "more than one chunk only where a whole wave owns the row");
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

    float *out_row = out + static_cast<size_t>(h) * p.o_head + static_cast<size_t>(row) * p.ldo;
    float o[NCH][VEC];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[c][v] = 0.f;
    // the lane's columns of chunk c are inside Dv or past it together (VEC == 4: Dv is a multiple of 4)
    auto store = [&](float l, float lse) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t col = c * CHUNK + lane * VEC;
            if (col >= p.Dv) continue;
            vec_t r;
#pragma unroll
            for (int v = 0; v < VEC; ++v) vec_set<VEC>(r, v, o[c][v] / l);
            store_vec<VEC>(out_row + col, r);
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
    vec_t xv[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        koff[c] = lane_off<G, VEC>(lane, c, p.D);
        voff[c] = lane_off<G, VEC>(lane, c, p.Dv);
        xv[c] = buffer_load_vec<VEC>(qr, join_off(row * p.ldq * 4u, koff[c]), 0);  // past D: zeros
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
        const uint32_t kkey = nxt_col * p.ldk4 | dead;
        const uint32_t vkey = nxt_col * p.ldv4 | dead;
        const float b = nxt_bias;
        fetch(s0 + E, nxt_col, nxt_bias);  // on its way while this batch is gathered
        __builtin_amdgcn_sched_barrier(0);  // ... issued here, ahead of the batch's own reads (see the end of the loop body)
        vec_t kv[E][NCH], vv[E][NCH];
        gather_rows<VEC, NCH>(kkey, kr, koff, kv);
        gather_rows<VEC, NCH>(vkey, vr, voff, vv);
        float acc[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[j] = __builtin_fmaf(vec_get<VEC>(xv[c], v), vec_get<VEC>(kv[j][c], v), acc[j]);  // not dot_chain: see there
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
                for (int v = 0; v < VEC; ++v) o[c][v] = __builtin_fmaf(wj, vec_get<VEC>(vv[j][c], v), o[c][v]);
        });
        // the next batch's column and bias must be in their registers HERE: without this the compiler moves the fetch over
        // the loop edge to the top of the batch that uses it and waits for it there, one exposed round trip per batch.  The
        // batch's own reads have all been waited for by now, so the empty statement costs no wait of its own.
        asm volatile("" : "+v"(nxt_col), "+v"(nxt_bias));
    }
    store(l, mu + __builtin_logf(l));
}

struct AcCall {
    hipStream_t stream;
    uint32_t H;
    AcParams p;
    const uint32_t *rowPtrs, *colIdxs;
    const float *Q, *K, *V, *bias;
    float *out, *lse;
};

template <int G, int VEC, int NCH>
void launch_attn_csr(const AcCall &c) {
    AcParams p = c.p;
    const uint32_t grid = finish_grid<G>(p, p.M, c.H);
    note_kernel("attn_csr<f32,G%d,V%d,C%d>", G, VEC, NCH);
    hipLaunchKernelGGL((attn_csr_kernel<G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.rowPtrs, c.colIdxs, c.Q, c.K, c.V,
                       c.bias, c.out, c.lse);
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_attn_csr_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                   const uint32_t *colIdxs, const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat,
                                   uint64_t k_head_stride, uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv,
                                   uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, float *out,
                                   uint64_t out_head_stride, uint32_t ldo, float *lse) {
    if (const int st = refuse_shape("attn_csr_f32", D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0) return MISPMM_OK;
    if (!rowPtrs || !Q || !Kmat || !V || !out || (nnz != 0 && !colIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_f32: rowPtrs, colIdxs, Q, K, V or out is null");
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_f32: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)", D,
                    ldq, ldk, Dv, ldv, ldo);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    const uint64_t qs = span(M, ldq, D) * 4u, ks = span(K, ldk, D) * 4u, vs = span(K, ldv, Dv) * 4u, os = span(M, ldo, Dv) * 4u;
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) * 4u : 0u;
    if (qs > 0x7FFFFFFFull || ks > 0x7FFFFFFFull || vs > 0x7FFFFFFFull || os > 0x7FFFFFFFull || bs > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "attn_csr_f32: Q, K, V, out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu bytes)",
                    static_cast<unsigned long long>(qs), static_cast<unsigned long long>(ks), static_cast<unsigned long long>(vs),
                    static_cast<unsigned long long>(os), static_cast<unsigned long long>(bs));
    const bool wide = D % 4 == 0 && Dv % 4 == 0 && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 && q_head_stride % 4 == 0 &&
                      k_head_stride % 4 == 0 && v_head_stride % 4 == 0 && out_head_stride % 4 == 0 && aligned16(Q) && aligned16(Kmat) &&
                      aligned16(V) && aligned16(out);
    const int vec = wide ? 4 : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid("attn_csr_f32", M, H, g); st != MISPMM_OK) return st;
    AcCall c{};
    c.stream = as_stream(stream);
    c.H = H;
    c.rowPtrs = rowPtrs, c.colIdxs = colIdxs;
    c.Q = Q, c.K = Kmat, c.V = V, c.bias = bias, c.out = out, c.lse = lse;
    AcParams &p = c.p;
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq = ldq, p.ldk4 = ldk * 4u, p.ldv4 = ldv * 4u, p.ldo = ldo;
    p.q_bytes = static_cast<uint32_t>(qs), p.k_bytes = static_cast<uint32_t>(ks), p.v_bytes = static_cast<uint32_t>(vs);
    p.bias_bytes = static_cast<uint32_t>(bs);
    p.scale = scale;
    p.q_head = q_head_stride, p.k_head = k_head_stride, p.v_head = v_head_stride, p.o_head = out_head_stride, p.bias_head = bias_head_stride;
    with_instance(vec, g, width, [&](auto gr, auto v, auto ch) { launch_attn_csr<decltype(gr)::value, decltype(v)::value, decltype(ch)::value>(c); });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
