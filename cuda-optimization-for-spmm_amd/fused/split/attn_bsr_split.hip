// Split-row fused block-sparse attention forward in bf16 (mispmm_attn_split.h): the forward of ../attn_bsr.hip with the steps
// of every block row dealt to S waves in different workgroups, and a second launch that merges their online-softmax states.
// The one-wave forward gives a block row to one wave, so M = 64 rows and 8 heads are 32 waves however many keys a row holds;
// here (head, 16-row unit, segment) is the work item and the card fills at S * units * H waves.
//
// PARTIAL KERNEL.  Unit, lane layout, transposed products, loads, MFMA hazard: ../attn_bsr_tiles.hpp.  A block row of n steps
// (n = ceil(blocks / EPS), 32 keys a step) is cut at whole steps: segment s walks steps floor(s n / S) .. floor((s + 1) n / S) - 1,
// computed here from blockRowPtrs.  The items of one head are numbered unit * S + s: the waves of a workgroup are consecutive
// segments of one unit (S >= 4), their K / V panels disjoint, Q shared through L1.  Inside its range [bs, be) of blocks the wave
// IS the one-wave kernel on a block row [bs, be): the loop below is ../attn_bsr.hip's, spelled a second time on purpose -- a
// loop shared through a helper moves the forward's ISA -- with the row's bounds replaced by the
// segment's.  So a prefetch past the segment's end is dropped (K, V) or re-reads the segment's last block (block column, mask):
// never past the row.  Only a row's true last step can be a half step at bS = 16.  A segment with no steps writes nothing.
// After the loop the four lanes of a row meet as there, and the wave stores its state UNNORMALISED: m, l, lx per row and the
// fp32 accumulator O (store_run with inv = 1).  No LDS, no barrier, no atomics.
//
// WORKSPACE (floats).  item = (h * units + unit) * S + s.  O: [items][16 rows][Dv] from the start; then the states:
// [items][3][16 rows] = m, l, lx.  A wave's O is one contiguous 64 Dv bytes x 16 span.
//
// COMBINE KERNEL.  Plain VALU, bandwidth-bound.  A 256-thread workgroup takes 8 rows of one unit (so one block row), 32
// threads to a row.  Wave 0 lists the non-empty segments (a ballot over s = lane; the same list for all 8 rows) in LDS; the
// rows' threads fetch the listed states into LDS; thread 0 of each row forms M, the weights, l and lx (the merge of the header,
// s ascending, every sum starting from its first term) and writes lse; then every thread streams its run of 4 columns of the
// listed O partials as 16-byte loads, s ascending, and stores O * (1 / l).  An empty segment's workspace is never read.
#include "../attn_bsr_tiles.hpp"
#include "mispmm_attn_split.h"

namespace mispmm {

namespace {

constexpr uint32_t kMaxSplits = 64;
constexpr uint32_t kCombineRows = 8;  // rows to a workgroup of the combine kernel, 32 threads each; divides 16: one unit, one block row

struct SplitParams {
    uint32_t units, wgs_per_head, total, xcd_chunk;  // units: work items of one head = 16-row units * S (finish_grid)
    uint32_t Kb, D, Dv, rows;                        // rows = numBlockRows * bS
    uint32_t ldq2, ldk2, ldv2, S;                    // ld*2: row strides in bytes
    uint32_t q_bytes, k_bytes, v_bytes;              // one head's span
    float scale;
    uint64_t q_head, k_head, v_head;                 // elements
};

// first step of segment s of a row of n = q * S + r steps: floor(s n / S) without a 64-bit product
__device__ __forceinline__ uint32_t seg_start(uint32_t s, uint32_t q, uint32_t r, uint32_t S) { return s * q + s * r / S; }

template <int BS, int DS, int TPL, bool MASK>
__global__ void __launch_bounds__(64 * kTileWaves)
    attn_bsr_split_kernel(const SplitParams p, const uint32_t *__restrict__ blockRowPtrs, const uint32_t *__restrict__ blockColIdxs,
                          const uint16_t *__restrict__ Q, const uint16_t *__restrict__ K, const uint16_t *__restrict__ V, const float *__restrict__ mask,
                          float *__restrict__ ws_o, float *__restrict__ ws_state) {
    using W = Walk<BS>;
    constexpr uint32_t kSecond = W::kSecond, EPS = W::EPS;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wg = xcd_block(blockIdx.x, p.xcd_chunk);
    if (wg >= p.total) return;
    const uint32_t h = wg / p.wgs_per_head;
    const uint32_t idx = (wg - h * p.wgs_per_head) * kTileWaves + wave;
    if (idx >= p.units) return;
    const uint32_t unit = idx / p.S, seg = idx - unit * p.S;
    const uint32_t R = unit / W::T, sub = unit % W::T;
    const uint32_t i = lane & 15, g = lane >> 4;
    const uint32_t row = unit * 16u + i;  // < rows
    const uint32_t rs = blockRowPtrs[R], re = blockRowPtrs[R + 1];
    if (re <= rs) return;  // an empty block row: the combine kernel writes its zeros
    const uint32_t n = (re - rs + EPS - 1) / EPS, nq = n / p.S, nr = n - nq * p.S;
    const uint32_t lo = seg_start(seg, nq, nr, p.S), hi = seg_start(seg + 1, nq, nr, p.S);
    if (hi <= lo) return;  // an empty segment writes nothing
    const uint32_t bs = rs + lo * EPS, be = min(re, rs + hi * EPS);  // the segment as a block row of its own
    const float ninf = -__builtin_huge_valf();

    f32x4_t acc[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto settle_acc = [&] { settle<TPL>(acc); };

    const rsrc_t qr = make_rsrc(Q + h * p.q_head, p.q_bytes), kr = make_rsrc(K + h * p.k_head, p.k_bytes), vr = make_rsrc(V + h * p.v_head, p.v_bytes);
    const uint32_t kcol = g * 8u;  // the lane's 8 columns of a 32-column step of D
    bf16x8_t qf[DS];
#pragma unroll
    for (int s = 0; s < DS; ++s) qf[s] = load_frag(qr, row * p.ldq2, s * 32u + kcol, p.D);

    uint32_t koff[DS], voff[4];
#pragma unroll
    for (int s = 0; s < DS; ++s) koff[s] = s * 32u + kcol < p.D ? i * p.ldk2 + (s * 32u + kcol) * 2u : kDropLoad;
    const uint32_t vcol = i * TPL;
#pragma unroll
    for (int j = 0; j < 4; ++j) voff[j] = vcol < p.Dv ? (4u * g + j) * p.ldv2 + vcol * 2u : kDropLoad;
    const size_t mask_at = static_cast<size_t>(sub * 16u + i) * BS + 4u * g;

    // the block columns behind the two 16-key tiles of the step that starts at block e; past the segment's end: none
    struct Cols {
        uint32_t a, b;
    };
    const uint32_t last = be - 1;
    auto cols_at = [&](uint32_t e) {
        const uint32_t ca = blockColIdxs[min(e, last)];
        if constexpr (BS == 16) {
            const uint32_t cb = blockColIdxs[min(e + 1, last)];
            return Cols{e < be ? ca : 0xFFFFFFFFu, e + 1 < be ? cb : 0xFFFFFFFFu};
        } else {
            return Cols{e < be ? ca : 0xFFFFFFFFu, e < be ? ca : 0xFFFFFFFFu};
        }
    };
    struct Stage {
        bf16x8_t k[2][DS];
        f32x4_t ma, mb;
        TRows<TPL> v;
    };
    auto load_stage = [&](Cols c, uint32_t e, Stage &st) {
        const bool va = c.a < p.Kb, vb = c.b < p.Kb;  // wave-uniform
        const uint32_t ra = va ? c.a * BS : 0u, rb = vb ? c.b * BS + kSecond : 0u;
#pragma unroll
        for (int s = 0; s < DS; ++s) {
            st.k[0][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(kr, va ? koff[s] : kDropLoad, ra * p.ldk2, 0));
            st.k[1][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(kr, vb ? koff[s] : kDropLoad, rb * p.ldk2, 0));
        }
        if constexpr (MASK) {  // a step past the segment's end re-reads the segment's last block: valid memory, never used
            const size_t ea = static_cast<size_t>(min(e, last)) * (BS * BS);
            const size_t eb = BS == 32 ? ea + 16u : static_cast<size_t>(min(e + 1, last)) * (BS * BS);
            st.ma = *reinterpret_cast<const f32x4_t *>(mask + ea + mask_at);
            st.mb = *reinterpret_cast<const f32x4_t *>(mask + eb + mask_at);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) load_trow<TPL>(st.v, j, vr, (j < 4 ? va : vb) ? voff[j & 3] : kDropLoad, (j < 4 ? ra : rb) * p.ldv2);
    };

    float m = ninf, mu = 0.f, l = 0.f, lx = 0.f;
    uint32_t e = bs;
    Cols nxt = cols_at(e + EPS);

    // the step of ../attn_bsr.hip, operation for operation: splits = 1 has that kernel's bits
    auto step = [&](const Stage &use, Stage &fill) {
        const Cols after = cols_at(e + 2 * EPS);
        load_stage(nxt, e + EPS, fill);
        const bool second = BS == 32 || e + 1 < be;  // wave-uniform: a half step (the row's last) has no second tile
        f32x4_t sa{0.f, 0.f, 0.f, 0.f}, sb{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DS; ++s) sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(use.k[0][s], qf[s], sa, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < DS; ++s) sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(use.k[1][s], qf[s], sb, 0, 0, 0);
        float z[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            z[j] = scaled<MASK>(p.scale, sa[j], use.ma, j);
            z[4 + j] = second ? scaled<MASK>(p.scale, sb[j], use.mb, j) : ninf;
        }
        float mx = z[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) mx = __builtin_fmaxf(mx, z[j]);  // drops a NaN operand: the weight carries it
        mx = __builtin_fmaxf(mx, lane_xor<16>(mx));
        mx = __builtin_fmaxf(mx, lane_xor<32>(mx));
        const float m_new = __builtin_fmaxf(m, mx);
        const float mu_new = __builtin_fabsf(m_new) == __builtin_huge_valf() ? 0.f : m_new;
        const float alpha = m == ninf ? 1.f : tile_exp(mu - mu_new);
        m = m_new;
        mu = mu_new;
        u32x4_t pw;
        float t = 0.f, tx = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float p0 = tile_exp(z[2 * w] - mu), p1 = tile_exp(z[2 * w + 1] - mu);
            pw[w] = __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(p0), static_cast<__bf16>(p1)});
            t = t + __uint_as_float(pw[w] << 16);
            t = t + __uint_as_float(pw[w] & 0xFFFF0000u);
            tx = tx + p0;
            tx = tx + p1;
        }
        l = l * alpha + t;
        lx = lx * alpha + tx;
        settle_acc();
#pragma unroll
        for (int tt = 0; tt < TPL; ++tt) acc[tt] = acc[tt] * alpha;
        const bf16x8_t pfrag = __builtin_bit_cast(bf16x8_t, pw);
#pragma unroll
        for (int w = 0; w < TPL / 2; ++w) mfma_trow_pair<TPL>(acc[2 * w], acc[2 * w + 1], use.v, w, pfrag);
        nxt = after;
        e += EPS;
    };

    Stage s0, s1;
    load_stage(cols_at(e), e, s0);
    for (;;) {
        step(s0, s1);
        if (e >= be) break;
        step(s1, s0);
        if (e >= be) break;
    }
    // the four lanes of a row meet: (g0 + g1) + (g2 + g3)
    l = l + lane_xor<16>(l);
    l = l + lane_xor<32>(l);
    lx = lx + lane_xor<16>(lx);
    lx = lx + lane_xor<32>(lx);
    settle_acc();
    const size_t item = (static_cast<size_t>(h) * (p.units / p.S) + unit) * p.S + seg;
    const size_t base = (item * 16u + i) * p.Dv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t col = TPL * (4u * g + k);
        if (col < p.Dv) store_run<TPL>(acc, k, 1.f, ws_o, base, col, false);
    }
    if (g == 0) {
        float *st = ws_state + item * 48u + i;
        st[0] = m;
        st[16] = l;
        st[32] = lx;
    }
}

struct CombineParams {
    uint32_t rows, units, S, Dv, ldo, eps, log2_bs;  // units: 16-row units of one head; eps: blocks per step
    uint64_t o_head;                                 // elements
};

template <bool OUT_BF16>
__global__ void __launch_bounds__(32 * kCombineRows)
    attn_bsr_combine_kernel(const CombineParams p, const uint32_t *__restrict__ blockRowPtrs, const float *__restrict__ ws_o,
                            const float *__restrict__ ws_state, void *__restrict__ out, float *__restrict__ lse_out) {
    __shared__ uint32_t s_list[kMaxSplits], s_count;
    __shared__ float s_m[kCombineRows][kMaxSplits], s_l[kCombineRows][kMaxSplits], s_lx[kCombineRows][kMaxSplits], s_w[kCombineRows][kMaxSplits];
    __shared__ float s_inv[kCombineRows];
    const uint32_t rw = threadIdx.x >> 5, j = threadIdx.x & 31;
    const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kCombineRows;  // of all heads; the grid is exact
    const uint32_t h = static_cast<uint32_t>(first / p.rows);
    const uint32_t row = static_cast<uint32_t>(first - static_cast<uint64_t>(h) * p.rows) + rw;
    const uint32_t R = (row - rw) >> p.log2_bs;  // workgroup-uniform: 8 consecutive rows of one 16-row unit
    const uint32_t unit = row >> 4, i = row & 15;
    const uint32_t blocks = blockRowPtrs[R + 1] - blockRowPtrs[R];
    const uint32_t col = 4u * j;
    const size_t o_at = static_cast<size_t>(h) * p.o_head + static_cast<size_t>(row) * p.ldo + col;
    auto store = [&](f32x4_t v) {
        if (col >= p.Dv) return;
        if constexpr (OUT_BF16) {
            const uint32_t o0 = __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(v[0]), static_cast<__bf16>(v[1])});
            const uint32_t o1 = __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(v[2]), static_cast<__bf16>(v[3])});
            *reinterpret_cast<u32x2_t *>(static_cast<uint16_t *>(out) + o_at) = u32x2_t{o0, o1};
        } else {
            *reinterpret_cast<f32x4_t *>(static_cast<float *>(out) + o_at) = v;
        }
    };
    if (static_cast<int32_t>(blocks) <= 0) {  // an empty block row: zero rows, lse = log 0
        store(f32x4_t{0.f, 0.f, 0.f, 0.f});
        if (lse_out && j == 0) lse_out[static_cast<size_t>(h) * p.rows + row] = -__builtin_huge_valf();
        return;
    }
    // the non-empty segments, ascending: the same for every row of the block row
    if (threadIdx.x < 64) {
        const uint32_t s = threadIdx.x;
        const uint32_t n = (blocks + p.eps - 1) / p.eps, nq = n / p.S, nr = n - nq * p.S;
        const bool live = s < p.S && seg_start(s, nq, nr, p.S) < seg_start(s + 1, nq, nr, p.S);
        const uint64_t lives = __ballot(live);
        if (live) s_list[__popcll(lives & ((1ull << s) - 1ull))] = s;
        if (s == 0) s_count = static_cast<uint32_t>(__popcll(lives));
    }
    __syncthreads();
    const uint32_t count = s_count;  // >= 1: the row has a step
    const size_t item0 = (static_cast<size_t>(h) * p.units + unit) * p.S;
    for (uint32_t k = j; k < count; k += 32) {
        const float *st = ws_state + (item0 + s_list[k]) * 48u + i;
        s_m[rw][k] = st[0];
        s_l[rw][k] = st[16];
        s_lx[rw][k] = st[32];
    }
    __syncthreads();
    if (j == 0) {  // the merge of mispmm_attn_split.h, steps 1 to 4 for l and lx
        const float inf = __builtin_huge_valf();
        float M = s_m[rw][0];
        for (uint32_t k = 1; k < count; ++k) M = __builtin_fmaxf(M, s_m[rw][k]);
        const float mu = __builtin_fabsf(M) == inf ? 0.f : M;
        float l = 0.f, lx = 0.f;
        for (uint32_t k = 0; k < count; ++k) {
            const float ms = s_m[rw][k];
            const float mus = __builtin_fabsf(ms) == inf ? 0.f : ms;
            const float w = ms == -inf ? 1.f : tile_exp(mus - mu);
            s_w[rw][k] = w;
            const float tl = w * s_l[rw][k], tlx = w * s_lx[rw][k];
            l = k == 0 ? tl : l + tl;
            lx = k == 0 ? tlx : lx + tlx;
        }
        s_inv[rw] = 1.f / l;
        if (lse_out) lse_out[static_cast<size_t>(h) * p.rows + row] = mu + __builtin_logf(lx);
    }
    __syncthreads();
    if (col >= p.Dv) return;
    const size_t stride = 16u * static_cast<size_t>(p.Dv);  // floats between the same row of two segments
    const float *src = ws_o + (item0 * 16u + i) * p.Dv + col;
    f32x4_t o = *reinterpret_cast<const f32x4_t *>(src + s_list[0] * stride) * s_w[rw][0];
#pragma unroll 4
    for (uint32_t k = 1; k < count; ++k) o = o + *reinterpret_cast<const f32x4_t *>(src + s_list[k] * stride) * s_w[rw][k];
    store(o * s_inv[rw]);
}

struct SplitCall {
    hipStream_t stream;
    uint32_t H, Mb, bS;
    SplitParams p;
    CombineParams c;
    const uint32_t *blockRowPtrs, *blockColIdxs;
    const uint16_t *Q, *K, *V;
    const float *mask;
    float *ws_o, *ws_state;
    void *out;
    float *lse;
};

template <int BS, int DS, int TPL, bool MASK>
void launch_partial(const SplitCall &c) {
    SplitParams p = c.p;
    const uint32_t grid = finish_grid(p, c.Mb * (BS / 16) * p.S, c.H);
    note_kernel("attn_bsr_split<b%d,%s,D%d,T%d,S%u>", BS, MASK ? "mask" : "nomask", DS, TPL, p.S);
    hipLaunchKernelGGL((attn_bsr_split_kernel<BS, DS, TPL, MASK>), dim3(grid), dim3(64 * kTileWaves), 0, c.stream, p, c.blockRowPtrs, c.blockColIdxs,
                       c.Q, c.K, c.V, c.mask, c.ws_o, c.ws_state);
}

template <bool OUT_BF16>
void launch_combine(const SplitCall &c) {
    const uint32_t grid = static_cast<uint32_t>(static_cast<uint64_t>(c.H) * c.c.rows / kCombineRows);
    note_kernel("attn_bsr_combine<%s,S%u>", OUT_BF16 ? "bf16" : "f32", c.c.S);
    hipLaunchKernelGGL((attn_bsr_combine_kernel<OUT_BF16>), dim3(grid), dim3(32 * kCombineRows), 0, c.stream, c.c, c.blockRowPtrs, c.ws_o, c.ws_state,
                       c.out, c.lse);
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" uint64_t mispmm_attn_bsr_split_workspace(uint32_t H, uint32_t numBlockRows, uint32_t bS, uint32_t Dv, uint32_t splits) {
    return static_cast<uint64_t>(H) * numBlockRows * bS * splits * (static_cast<uint64_t>(Dv) + 3u) * 4u;
}

extern "C" int mispmm_attn_bsr_split_bf16(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                                          const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint16_t *Q, uint32_t ldq,
                                          uint64_t q_head, const uint16_t *Kmat, uint32_t ldk, uint64_t k_head, const uint16_t *V, uint32_t ldv,
                                          uint64_t v_head, uint32_t D, uint32_t Dv, const float *mask, float scale, void *out, uint32_t ldo,
                                          uint64_t o_head, int out_bf16, float *lse, uint32_t splits, void *workspace, uint64_t workspace_bytes) {
    if (const int refused = refuse_shape("attn_bsr_split_bf16", bS, scale, D, Dv, K)) return refused;
    if (splits == 0 || splits > kMaxSplits)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_split_bf16: splits must be 1 to %u (got %u)", kMaxSplits, splits);
    if (H == 0 || numBlockRows == 0) return MISPMM_OK;
    if (!blockRowPtrs || !Q || !Kmat || !V || !out || (numBlocks != 0 && !blockColIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_split_bf16: blockRowPtrs, blockColIdxs, Q, K, V or out is null");
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_split_bf16: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)",
                    D, ldq, ldk, Dv, ldv, ldo);
    // every lane reads 16-byte vectors; a combine thread writes 4 columns: 16 bytes of fp32, 8 of bf16 (alignment as mispmm_attn_bsr_bf16)
    const uint32_t oq = out_bf16 ? 8u : 4u;
    if (!aligned16(Q) || !aligned16(Kmat) || !aligned16(V) || !aligned16(out) || (mask && !aligned16(mask)) || ldq % 8 || ldk % 8 || ldv % 8 ||
        ldo % oq || q_head % 8 || k_head % 8 || v_head % 8 || o_head % oq)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "attn_bsr_split_bf16: Q, K, V, mask and out must be 16-byte aligned, and so every row and head stride (ldq=%u ldk=%u ldv=%u "
                    "ldo=%u heads %llu %llu %llu %llu)",
                    ldq, ldk, ldv, ldo, static_cast<unsigned long long>(q_head), static_cast<unsigned long long>(k_head),
                    static_cast<unsigned long long>(v_head), static_cast<unsigned long long>(o_head));
    const uint64_t rows = static_cast<uint64_t>(numBlockRows) * bS;
    const uint64_t qs = span(rows, ldq, D) * 2u, ks = span(K, ldk, D) * 2u, vs = span(K, ldv, Dv) * 2u;
    if (qs > 0x7FFFFFFFull || ks > 0x7FFFFFFFull || vs > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "attn_bsr_split_bf16: Q, K or V of one head spans 2 GiB or more (%llu, %llu, %llu bytes)",
                    static_cast<unsigned long long>(qs), static_cast<unsigned long long>(ks), static_cast<unsigned long long>(vs));
    if (rows > 0x7FFFFFFFull || ceil_div64(rows / 16 * splits, kTileWaves) * H > 0x7FFFFFFFull || rows / kCombineRows * H > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "attn_bsr_split_bf16: %llu rows x %u heads x %u splits are more work units than one launch takes",
                    static_cast<unsigned long long>(rows), H, splits);
    const uint64_t need = mispmm_attn_bsr_split_workspace(H, numBlockRows, bS, Dv, splits);
    if (!workspace || !aligned16(workspace) || workspace_bytes < need)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_split_bf16: the workspace must be 16-byte aligned and hold %llu bytes (got %s, %llu bytes)",
                    static_cast<unsigned long long>(need), !workspace ? "null" : aligned16(workspace) ? "an aligned pointer" : "a misaligned pointer",
                    static_cast<unsigned long long>(workspace_bytes));
    SplitCall c{};
    c.stream = as_stream(stream);
    c.H = H, c.Mb = numBlockRows, c.bS = bS;
    c.blockRowPtrs = blockRowPtrs, c.blockColIdxs = blockColIdxs;
    c.Q = Q, c.K = Kmat, c.V = V;
    c.mask = mask, c.out = out, c.lse = lse;
    c.ws_o = static_cast<float *>(workspace);
    c.ws_state = c.ws_o + static_cast<uint64_t>(H) * rows * splits * Dv;
    SplitParams &p = c.p;
    p.Kb = K / bS, p.D = D, p.Dv = Dv, p.rows = static_cast<uint32_t>(rows), p.S = splits;
    p.ldq2 = ldq * 2u, p.ldk2 = ldk * 2u, p.ldv2 = ldv * 2u;
    p.q_bytes = static_cast<uint32_t>(qs), p.k_bytes = static_cast<uint32_t>(ks), p.v_bytes = static_cast<uint32_t>(vs);
    p.q_head = q_head, p.k_head = k_head, p.v_head = v_head;
    p.scale = scale;
    c.c = CombineParams{p.rows, p.rows / 16u, splits, Dv, ldo, bS == 16 ? 2u : 1u, bS == 16 ? 4u : 5u, o_head};
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_const<2, 4>(D <= 64 ? 2 : 4, [&](auto ds) {
            with_const<4, 8>(Dv <= 64 ? 4 : 8, [&](auto tpl) {
                with_flag(mask != nullptr, [&](auto mk) { launch_partial<decltype(bs)::value, decltype(ds)::value, decltype(tpl)::value, decltype(mk)::value>(c); });
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    with_flag(out_bf16 != 0, [&](auto ob) { launch_combine<decltype(ob)::value>(c); });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
