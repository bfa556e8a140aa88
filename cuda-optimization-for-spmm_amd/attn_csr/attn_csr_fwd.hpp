// The forward kernel of the fused attention on a CSR pattern, written once over the element policy of elem.hpp and
// instantiated by attn_csr.hip (ElemF32: 10 instances) and attn_csr_bf16/attn_csr_bf16.hip (ElemBf16: 9) -- scores, row softmax
// and the product with V in ONE launch for all heads, fp32 arithmetic (bf16 operands exactly widened).
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
// Every dot product is ONE fma chain per lane from +0, columns ascending -- for bf16 on the widened values, not a packed dot
// instruction: the bits of z are determined (the headers' ALGORITHM).
// Online softmax per batch: the batch maximum over the 8 lanes of a segment (3 moves), folded into the running maximum m;
// mu = m with an infinite m replaced by 0 (what torch.logsumexp subtracts); alpha = exp(mu_old - mu_new), exactly 1 while m
// is still -Inf; one v_exp_f32 per lane for the weight; the 8 weights are summed by a fixed tree over the segment (3 moves)
// into l = fl(fl(l * alpha) + t) and reach the group by DPP row_newbcast for O = fl(alpha * O), then O = fma(w_i, V[c_i], O)
// for i = 0..7.  Every lane of the group holds the same alpha bits, so O and l are scaled by the same number.
// After the row: out = O / l (an IEEE division per element; a bf16 out is that quotient rounded once), lse = mu + log l.
// A dead slot's score is replaced by -Inf before the maximum: its weight is exp2(-Inf) = +0.
// The bias is read through a descriptor of its own that spans nothing where there is no bias: every read then returns +0
// and no branch stands in the loop.  Run to run identical.
#pragma once
#include "elem.hpp"

namespace mispmm {

namespace {

// the kernel's parameter block, one per element type so that each keeps its kernel-argument offsets.  Row strides of K and V
// in bytes, ldo in elements of out; Q's, read once per row, is kept as each kernel had it and q_row gives the row's byte offset
// either way.  The spans are one head's, bias_bytes == 0: no bias; head strides in elements
template <class Elem> struct FwdParams;
template <> struct FwdParams<ElemF32> {
    uint32_t M, D, Dv, blocks_per_head, total, xcd_chunk;
    uint32_t ldq, ldk, ldv, ldo;  // ldq in elements here
    uint32_t q_bytes, k_bytes, v_bytes, bias_bytes;
    float scale;
    uint64_t q_head, k_head, v_head, o_head, bias_head;
    static constexpr bool narrow = false;
    __device__ uint32_t q_row(uint32_t row) const { return row * ldq * 4u; }
};
template <> struct FwdParams<ElemBf16> {
    uint32_t M, D, Dv, blocks_per_head, total, xcd_chunk;
    uint32_t ldq, ldk, ldv, ldo;
    uint32_t q_bytes, k_bytes, v_bytes, bias_bytes;
    uint32_t narrow;  // out is bf16
    float scale;
    uint64_t q_head, k_head, v_head, o_head, bias_head;
    __device__ uint32_t q_row(uint32_t row) const { return row * ldq; }
};

template <class Elem, int G, int VEC, int NCH>
__global__ void __launch_bounds__(kLgBlock) attn_csr_kernel(const FwdParams<Elem> p, const uint32_t *__restrict__ rowPtrs,
                                                            const uint32_t *__restrict__ colIdxs, const typename Elem::in_t *__restrict__ Q,
                                                            const typename Elem::in_t *__restrict__ K,
                                                            const typename Elem::in_t *__restrict__ V, const float *__restrict__ bias,
                                                            typename Elem::out_t *__restrict__ out, float *__restrict__ lse_out) {
    using raw_t = typename Elem::template raw_t<VEC>;
    static_assert(G >= kLgBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's scores sit in the first lanes of a group");
    static_assert(Elem::template fits<G, VEC, NCH>, "no such lane width or chunk count for this element type");
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

    const typename Elem::row_t out_row = Elem::row_of(out, h, p.o_head, row, p.ldo);
    float o[NCH][VEC];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[c][v] = 0.f;
    // the lane's columns of chunk c are inside Dv or past it together (wide lanes: Dv is a multiple of the lane width)
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
    if (len == 0) {  // an empty row: +0 / 1 and lse = log 0
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
        if constexpr (Elem::kWidens) {  // spelled out here: behind a helper that fills xq[c] the bf16 V8 prologue changes
#pragma unroll
            for (int v = 0; v < VEC; ++v) xq[c][v] = Elem::template at<VEC>(qraw, v);
        } else {
            xq[c] = qraw;
        }
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
        const uint32_t kkey = nxt_col * p.ldk | dead;
        const uint32_t vkey = nxt_col * p.ldv | dead;
        const float b = nxt_bias;
        fetch(s0 + E, nxt_col, nxt_bias);  // on its way while this batch is gathered
        __builtin_amdgcn_sched_barrier(0);  // ... issued here, ahead of the batch's own reads (see the end of the loop body)
        raw_t kv[E][NCH], vv[E][NCH];
        Elem::template gather<VEC, NCH>(kkey, kr, koff, kv);
        Elem::template gather<VEC, NCH>(vkey, vr, voff, vv);
        float acc[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            acc[j] = 0.f;
            // spelled out, not through a helper that takes the two slices: that moves the Q[r] read of the fp32 V4 instances
            // behind the first key fetch
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    acc[j] = __builtin_fmaf(Elem::template held<VEC>(xq[c], v), Elem::template at<VEC>(kv[j][c], v), acc[j]);
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
                for (int v = 0; v < VEC; ++v) o[c][v] = __builtin_fmaf(wj, Elem::template at<VEC>(vv[j][c], v), o[c][v]);
        });
        // the next batch's column and bias must be in their registers HERE: without this the compiler moves the fetch over
        // the loop edge to the top of the batch that uses it and waits for it there, one exposed round trip per batch.  The
        // batch's own reads have all been waited for by now, so the empty statement costs no wait of its own.
        asm volatile("" : "+v"(nxt_col), "+v"(nxt_bias));
    }
    store(l, mu + __builtin_logf(l));
}

// what an entry point hands to its launch
template <class Elem>
struct FwdCall {
    hipStream_t stream;
    uint32_t H;
    FwdParams<Elem> p;
    const uint32_t *rowPtrs, *colIdxs;
    const typename Elem::in_t *Q, *K, *V;
    const float *bias;
    typename Elem::out_t *out;
    float *lse;
};

// `tag`: the library's own note_kernel format, with G, VEC and NCH to fill in
template <class Elem, int G, int VEC, int NCH>
void launch_attn_csr(const FwdCall<Elem> &c, const char *tag) {
    FwdParams<Elem> p = c.p;
    const uint32_t grid = finish_grid<G>(p, p.M, c.H);
    note_kernel(tag, G, VEC, NCH);
    hipLaunchKernelGGL((attn_csr_kernel<Elem, G, VEC, NCH>), dim3(grid), dim3(kLgBlock), 0, c.stream, p, c.rowPtrs, c.colIdxs, c.Q, c.K, c.V,
                       c.bias, c.out, c.lse);
}

}  // namespace

}  // namespace mispmm
