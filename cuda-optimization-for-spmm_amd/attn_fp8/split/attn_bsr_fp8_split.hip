// libmispmm_attn_fp8_split.so: the fused block-sparse attention forward on e4m3 operands (../attn_bsr_fp8.hip) with the steps of
// every block row dealt to S waves in different workgroups, a second launch that merges their online-softmax states, and K / V
// heads shared by groups of query heads (include/mispmm_attn_fp8_split.h).  The one-launch kernel gives a block row to one
// wave: M = 64 rows and 8 heads are 32 waves however long the context.  Here (head, 16-row unit, segment) is the work item.
//
// PARTIAL KERNEL.  Lane layout, the transposed score product on 16-byte K reads feeding two MFMAs, the weights as e4m3 of
// fl(2^8 w), V in the V layout through v_perm_b32 byte transposes, the two named stages: ../attn_bsr_fp8.hip, whose header says
// why each is so.  A block row of n steps (n = ceil(blocks / EPS), 32 keys a step) is cut at whole steps: segment s walks steps
// floor(s n / S) .. floor((s + 1) n / S) - 1, computed here from blockRowPtrs.  The items of one head are numbered unit * S + s:
// the waves of a workgroup are consecutive segments of one unit, their K / V panels disjoint, Q shared through L1.  Inside its
// range [bs, be) of blocks the wave IS the one-launch wave on a block row [bs, be): the loop below is ../attn_bsr_fp8.hip's,
// spelled a second time on purpose -- a loop shared through a helper moves the ISA of that library's 32 instances (DESIGN.md
// section 9 items 25 and 30) -- with the row's bounds replaced by the segment's.  So a prefetch past the segment's end is
// dropped (K, V) or re-reads the segment's last block (block column, mask): never past the row.  Only a row's true last step
// can be a half step at bS = 16.  A segment with no steps writes nothing.  After the loop the four lanes of a row meet as
// there, and the wave stores its state UNNORMALISED and not multiplied by v_scale: m, l, lx per row and the fp32 accumulator O
// in 16-byte stores.  No LDS, no barrier, no atomics.  transpose4, low8, high8, mfma8 and kWeightScale are spelled here as
// there: ../attn_bsr_fp8.hip stays byte for byte what it was.
//
// SHARED KV HEADS.  Query head h reads K, V, k_scale and v_scale of KV head h / G, G = kv_group.  The workgroups are numbered
// (KV head, workgroup of a head, query head of the group), the query head innermost: in XCD order (xcd_block: an XCD owns a
// contiguous run of that numbering) the G workgroups that walk the same segments of the same unit over the SAME K / V panel
// are neighbours on one XCD, so the panel the first pulls into that XCD's L2 is the one the next G - 1 read.  Heads outermost
// -- the numbering of the one-launch kernel -- would put a group's heads units * S / 4 workgroups apart, and on different
// XCDs once that passes an eighth of the grid.  G = 1 is the one-launch numbering.
//
// WORKSPACE (floats).  item = (h * units + unit) * S + s.  O: [items][16 rows][Dv] from the start; then the states:
// [items][3][16 rows] = m, l, lx.
//
// COMBINE KERNEL.  The shape of fused/split/attn_bsr_split.hip's: plain VALU, bandwidth-bound.  A 256-thread workgroup takes 8
// rows of one unit, 32 threads to a row.  Wave 0 lists the non-empty segments (a ballot over s = lane) in LDS; the rows'
// threads fetch the listed states into LDS; thread 0 of each row forms M, the weights, l and lx (the merge of the header, s
// ascending, every sum starting from its first term) and writes lse; then every thread streams its run of 4 columns of the
// listed O partials as 16-byte loads, s ascending, and stores fl(fl(O * (1 / l)) * v_scale[h / G]).
#include "../../fused/attn_bsr_tiles.hpp"
#include "mispmm_attn_fp8_split.h"

namespace mispmm {

namespace {

constexpr uint32_t kMaxSplits = 64;
constexpr uint32_t kCombineRows = 8;  // rows to a workgroup of the combine kernel, 32 threads each; divides 16: one unit, one block row

struct Fp8SplitParams {
    uint32_t units, wgs_per_head, total, xcd_chunk;  // units: work items of one head = 16-row units * S (finish_grid)
    uint32_t Kb, D, Dv, rows;                        // rows = numBlockRows * bS
    uint32_t ldq, ldk, ldv, S;                       // row strides in elements = bytes
    uint32_t q_bytes, k_bytes, v_bytes, G;           // one head's span; G: query heads to a KV head
    float scale;
    uint64_t q_head, k_head, v_head;                 // elements
};

constexpr float kWeightScale = 256.f;  // the weights enter e4m3 times 2^8

// rows r0 .. r3 hold byte j = tile j; out[j] holds byte e = row e of tile j
__device__ __forceinline__ void transpose4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t (&out)[4]) {
    const uint32_t lo01 = __builtin_amdgcn_perm(r1, r0, 0x05010400u);  // {r0.b0, r1.b0, r0.b1, r1.b1}
    const uint32_t hi01 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);  // {r0.b2, r1.b2, r0.b3, r1.b3}
    const uint32_t lo23 = __builtin_amdgcn_perm(r3, r2, 0x05010400u);
    const uint32_t hi23 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
    out[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

// the two 8-byte operands of a 16-byte read: the low half goes to one MFMA, the high half to the next
__device__ __forceinline__ long low8(u32x4_t v) { return __builtin_bit_cast(long, u32x2_t{v[0], v[1]}); }
__device__ __forceinline__ long high8(u32x4_t v) { return __builtin_bit_cast(long, u32x2_t{v[2], v[3]}); }

__device__ __forceinline__ f32x4_t mfma8(long a, long b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0); }

// first step of segment s of a row of n = q * S + r steps: floor(s n / S) without a 64-bit product (s <= S <= 64, r < S)
__device__ __forceinline__ uint32_t seg_start(uint32_t s, uint32_t q, uint32_t r, uint32_t S) { return s * q + s * r / S; }

// BS: block size.  DS: 64-column steps of D held (D <= 64 DS).  TPL: accumulator tiles = consecutive V bytes per lane
// (Dv <= 16 TPL).  The arrays are kernel arguments of their own, `const __restrict__`: block columns and scales come by
// scalar loads.
template <int BS, int DS, int TPL, bool MASK>
__global__ void __launch_bounds__(64 * kTileWaves)
    attn_bsr_fp8_split_kernel(const Fp8SplitParams p, const uint32_t *__restrict__ blockRowPtrs, const uint32_t *__restrict__ blockColIdxs,
                              const uint8_t *__restrict__ Q, const uint8_t *__restrict__ K, const uint8_t *__restrict__ V,
                              const float *__restrict__ q_scale, const float *__restrict__ k_scale, const float *__restrict__ mask,
                              float *__restrict__ ws_o, float *__restrict__ ws_state) {
    static_assert((BS == 16 || BS == 32) && (DS == 1 || DS == 2) && (TPL == 4 || TPL == 8), "the instances of the header");
    using W = Walk<BS>;
    constexpr int VW = TPL / 4;  // dwords of one V row read
    constexpr uint32_t kSecond = W::kSecond, EPS = W::EPS;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wg = xcd_block(blockIdx.x, p.xcd_chunk);
    if (wg >= p.total) return;
    // (KV head, workgroup of a head, query head of the group): the heads that share a K / V panel are neighbours
    const uint32_t per_kv = p.wgs_per_head * p.G;
    const uint32_t kvh = wg / per_kv, in_kv = wg - kvh * per_kv;
    const uint32_t w_in_head = in_kv / p.G;
    const uint32_t h = kvh * p.G + (in_kv - w_in_head * p.G);
    const uint32_t idx = w_in_head * kTileWaves + wave;
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
    const uint32_t bs = rs + lo * EPS, be = min(re, rs + hi * EPS);  // the segment as a block row of its own: rs <= bs < be <= re
    const float ninf = -__builtin_huge_valf();

    f32x4_t acc[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto settle_acc = [&] { settle<TPL>(acc); };

    // c_h = fl(fl(scale * q_scale[h]) * k_scale[h / G]), once per wave; a NULL scale is no multiply
    float c_h = p.scale;
    if (q_scale) c_h = c_h * q_scale[h];
    if (k_scale) c_h = c_h * k_scale[kvh];

    const rsrc_t qr = make_rsrc(Q + h * p.q_head, p.q_bytes), kr = make_rsrc(K + kvh * p.k_head, p.k_bytes),
                 vr = make_rsrc(V + kvh * p.v_head, p.v_bytes);
    const uint32_t dcol = g * 16u;  // the lane's 16 columns of a 64-column step of D
    u32x4_t qf[DS];
    uint32_t koff[DS], voff[4];
#pragma unroll
    for (int s = 0; s < DS; ++s) {
        const bool in = s * 64u + dcol < p.D;  // all 16 columns or none: D is a multiple of 16
        qf[s] = __builtin_amdgcn_raw_buffer_load_b128(qr, in ? row * p.ldq + s * 64u + dcol : kDropLoad, 0, 0);  // < 2 GiB: the host declines more
        koff[s] = in ? i * p.ldk + s * 64u + dcol : kDropLoad;
    }
    const uint32_t vcol = i * TPL;  // first of the lane's TPL V columns, one per accumulator tile
#pragma unroll
    for (int j = 0; j < 4; ++j) voff[j] = vcol < p.Dv ? (4u * g + j) * p.ldv + vcol : kDropLoad;
    const size_t mask_at = static_cast<size_t>(sub * 16u + i) * BS + 4u * g;  // the lane's 4 mask elements inside a block (32 x 32: + 16 for the second tile)

    // the block columns behind the two 16-key tiles of the step that starts at block e (bS = 32: one block); past the segment's end: none
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
    // everything a step reads, fetched one step ahead: K's 16-byte fragments, the mask's elements, V's rows
    struct Stage {
        u32x4_t k[2][DS];
        f32x4_t ma, mb;
        uint32_t v[8][VW];
    };
    auto load_stage = [&](Cols c, uint32_t e, Stage &st) {
        const bool va = c.a < p.Kb, vb = c.b < p.Kb;  // wave-uniform
        const uint32_t ra = va ? c.a * BS : 0u, rb = vb ? c.b * BS + kSecond : 0u;
#pragma unroll
        for (int s = 0; s < DS; ++s) {
            st.k[0][s] = __builtin_amdgcn_raw_buffer_load_b128(kr, va ? koff[s] : kDropLoad, ra * p.ldk, 0);
            st.k[1][s] = __builtin_amdgcn_raw_buffer_load_b128(kr, vb ? koff[s] : kDropLoad, rb * p.ldk, 0);
        }
        if constexpr (MASK) {  // a step past the segment's end re-reads the segment's last block: valid memory, never used
            const size_t ea = static_cast<size_t>(min(e, last)) * (BS * BS);
            const size_t eb = BS == 32 ? ea + 16u : static_cast<size_t>(min(e + 1, last)) * (BS * BS);
            st.ma = *reinterpret_cast<const f32x4_t *>(mask + ea + mask_at);
            st.mb = *reinterpret_cast<const f32x4_t *>(mask + eb + mask_at);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t vo = (j < 4 ? va : vb) ? voff[j & 3] : kDropLoad, so = (j < 4 ? ra : rb) * p.ldv;
            if constexpr (TPL == 8) {
                const auto r = __builtin_amdgcn_raw_buffer_load_b64(vr, vo, so, 0);
                st.v[j][0] = r[0];
                st.v[j][1] = r[1];
            } else {
                st.v[j][0] = __builtin_amdgcn_raw_buffer_load_b32(vr, vo, so, 0);
            }
        }
    };

    float m = ninf, mu = 0.f, l = 0.f, lx = 0.f;
    uint32_t e = bs;
    Cols nxt = cols_at(e + EPS);

    // the step of ../attn_bsr_fp8.hip, operation for operation: splits = 1 has that kernel's bits
    auto step = [&](const Stage &use, Stage &fill) {
        const Cols after = cols_at(e + 2 * EPS);
        load_stage(nxt, e + EPS, fill);
        const bool second = BS == 32 || e + 1 < be;  // wave-uniform: a half step (the row's last) has no second tile
        // per tile: columns 64 s + 16 g + 0 .. 7, then + 8 .. 15, s ascending; the two tiles' chains interleaved
        f32x4_t sa{0.f, 0.f, 0.f, 0.f}, sb{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DS; ++s) {
            sa = mfma8(low8(use.k[0][s]), low8(qf[s]), sa);
            sb = mfma8(low8(use.k[1][s]), low8(qf[s]), sb);
            sa = mfma8(high8(use.k[0][s]), high8(qf[s]), sa);
            sb = mfma8(high8(use.k[1][s]), high8(qf[s]), sb);
        }
        float z[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            z[j] = scaled<MASK>(c_h, sa[j], use.ma, j);
            z[4 + j] = second ? scaled<MASK>(c_h, sb[j], use.mb, j) : ninf;
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
        // the lane's 8 weights: unrounded into tx, times 2^8 into the two dwords of the B operand, read back into t
        uint32_t pw[2] = {0u, 0u};
        float t = 0.f, tx = 0.f;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            float pz[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pz[j] = tile_exp(z[4 * w + j] - mu);
                tx = tx + pz[j];
            }
            int d = __builtin_amdgcn_cvt_pk_fp8_f32(pz[0] * kWeightScale, pz[1] * kWeightScale, 0, false);
            d = __builtin_amdgcn_cvt_pk_fp8_f32(pz[2] * kWeightScale, pz[3] * kWeightScale, d, true);
            const auto lo8 = __builtin_amdgcn_cvt_pk_f32_fp8(d, false), hi8 = __builtin_amdgcn_cvt_pk_f32_fp8(d, true);
            t = t + lo8[0];
            t = t + lo8[1];
            t = t + hi8[0];
            t = t + hi8[1];
            pw[w] = static_cast<uint32_t>(d);
        }
        t = t + (tx - tx);  // +0, or NaN where a weight is +Inf or NaN: the row is NaN whatever the converter made of it
        l = l * alpha + t;
        lx = lx * alpha + tx;
        settle_acc();
#pragma unroll
        for (int tt = 0; tt < TPL; ++tt) acc[tt] = acc[tt] * alpha;
        const long pfrag = __builtin_bit_cast(long, u32x2_t{pw[0], pw[1]});
#pragma unroll
        for (int w = 0; w < VW; ++w) {
            uint32_t tl[4], th[4];
            transpose4(use.v[0][w], use.v[1][w], use.v[2][w], use.v[3][w], tl);
            transpose4(use.v[4][w], use.v[5][w], use.v[6][w], use.v[7][w], th);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * w + j] = mfma8(__builtin_bit_cast(long, u32x2_t{tl[j], th[j]}), pfrag, acc[4 * w + j]);
        }
        nxt = after;
        e += EPS;
    };

    // two stages in turn (a copy `cur = nxt` would wait for the loads it is meant to hide)
    Stage s0, s1;
    load_stage(cols_at(e), e, s0);
    for (;;) {
        step(s0, s1);
        if (e >= be) break;
        step(s1, s0);
        if (e >= be) break;
    }
    // the four lanes of a row meet: (g0 + g1) + (g2 + g3), both partners of a move holding the same sum
    l = l + lane_xor<16>(l);
    l = l + lane_xor<32>(l);
    lx = lx + lane_xor<16>(lx);
    lx = lx + lane_xor<32>(lx);
    settle_acc();
    // item < H * (units / S) * S and col + TPL <= Dv: inside the O part of the workspace the host sized
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

struct Fp8CombineParams {
    uint32_t rows, units, S, Dv, ldo, eps, log2_bs, G;  // units: 16-row units of one head; eps: blocks per step; G: query heads to a KV head
    uint64_t o_head;                                    // elements
};

template <bool OUT_BF16>
__global__ void __launch_bounds__(32 * kCombineRows)
    attn_bsr_fp8_combine_kernel(const Fp8CombineParams p, const uint32_t *__restrict__ blockRowPtrs, const float *__restrict__ ws_o,
                                const float *__restrict__ ws_state, const float *__restrict__ v_scale, void *__restrict__ out,
                                float *__restrict__ lse_out) {
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
    if (static_cast<int32_t>(blocks) <= 0) {  // an empty block row: +0 whatever v_scale holds, lse = log 0
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
    if (j == 0) {  // the merge of the header, steps 1 to 4 for l and lx
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
    // out = fl(fl(O * inv) * vs): two multiplies; a NULL v_scale: the first alone
    o = o * s_inv[rw];
    if (v_scale) o = o * v_scale[h / p.G];
    store(o);
}

struct Fp8SplitCall {
    hipStream_t stream;
    uint32_t H, Mb;
    Fp8SplitParams p;
    Fp8CombineParams c;
    const uint32_t *blockRowPtrs, *blockColIdxs;
    const uint8_t *Q, *K, *V;
    const float *q_scale, *k_scale, *v_scale, *mask;
    float *ws_o, *ws_state;
    void *out;
    float *lse;
};

template <int BS, int DS, int TPL, bool MASK>
void launch_partial(const Fp8SplitCall &c) {
    Fp8SplitParams p = c.p;
    const uint32_t grid = finish_grid(p, c.Mb * (BS / 16) * p.S, c.H);
    note_kernel("attn_bsr_fp8_split<b%d,%s,D%d,T%d,S%u>", BS, MASK ? "mask" : "nomask", DS, TPL, p.S);
    hipLaunchKernelGGL((attn_bsr_fp8_split_kernel<BS, DS, TPL, MASK>), dim3(grid), dim3(64 * kTileWaves), 0, c.stream, p, c.blockRowPtrs,
                       c.blockColIdxs, c.Q, c.K, c.V, c.q_scale, c.k_scale, c.mask, c.ws_o, c.ws_state);
}

template <bool OUT_BF16>
void launch_combine(const Fp8SplitCall &c) {
    const uint32_t grid = static_cast<uint32_t>(static_cast<uint64_t>(c.H) * c.c.rows / kCombineRows);
    note_kernel("attn_bsr_fp8_combine<%s,S%u>", OUT_BF16 ? "bf16" : "f32", c.c.S);
    hipLaunchKernelGGL((attn_bsr_fp8_combine_kernel<OUT_BF16>), dim3(grid), dim3(32 * kCombineRows), 0, c.stream, c.c, c.blockRowPtrs, c.ws_o,
                       c.ws_state, c.v_scale, c.out, c.lse);
}

bool aligned4(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 3u) == 0; }

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" uint64_t mispmm_attn_bsr_fp8_split_workspace(uint32_t H, uint32_t numBlockRows, uint32_t bS, uint32_t Dv, uint32_t splits) {
    return static_cast<uint64_t>(H) * numBlockRows * bS * splits * (static_cast<uint64_t>(Dv) + 3u) * 4u;
}

extern "C" int mispmm_attn_bsr_fp8_split(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                                         const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint8_t *Q, uint32_t ldq,
                                         uint64_t q_head, const uint8_t *Kmat, uint32_t ldk, uint64_t k_head, const uint8_t *V, uint32_t ldv,
                                         uint64_t v_head, uint32_t D, uint32_t Dv, const float *mask, float scale, const float *q_scale,
                                         const float *k_scale, const float *v_scale, void *out, uint32_t ldo, uint64_t o_head, int out_bf16,
                                         float *lse, uint32_t kv_group, uint32_t splits, void *workspace, uint64_t workspace_bytes) {
    constexpr const char *fn = "attn_bsr_fp8_split";
    if (const int refused = refuse_shape(fn, bS, scale, D, Dv, K)) return refused;
    if (D % 16 != 0)  // a lane reads 16 bytes of a row of Q or K: wholly inside D or wholly dropped
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: D must be a multiple of 16 from 16 to 128 (got D=%u)", fn, D);
    if (kv_group == 0 || H % kv_group != 0)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: kv_group must be 1 or more and divide H (got kv_group=%u, H=%u)", fn, kv_group, H);
    if (splits == 0 || splits > kMaxSplits) return fail(MISPMM_ERR_INVALID_ARG, "%s: splits must be 1 to %u (got %u)", fn, kMaxSplits, splits);
    const uint64_t need = mispmm_attn_bsr_fp8_split_workspace(H, numBlockRows, bS, Dv, splits);
    if (!workspace || !aligned16(workspace) || workspace_bytes < need)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: the workspace must be 16-byte aligned and hold %llu bytes (got %s, %llu bytes)", fn,
                    static_cast<unsigned long long>(need), !workspace ? "null" : aligned16(workspace) ? "an aligned pointer" : "a misaligned pointer",
                    static_cast<unsigned long long>(workspace_bytes));
    if (H == 0 || numBlockRows == 0) return MISPMM_OK;
    if (!blockRowPtrs || !Q || !Kmat || !V || !out || (numBlocks != 0 && !blockColIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: blockRowPtrs, blockColIdxs, Q, K, V or out is null", fn);
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)", fn, D, ldq,
                    ldk, Dv, ldv, ldo);
    // a lane reads 16 bytes of Q and K, 8 (T4: 4) of V and 16 of the mask; a combine thread writes 4 columns: 16 bytes of fp32, 8 of
    // bf16 (the alignment of mispmm_attn_bsr_fp8)
    const uint32_t oq = out_bf16 ? 8u : 4u;
    if (!aligned16(Q) || !aligned16(Kmat) || !aligned8(V) || !aligned16(out) || (mask && !aligned16(mask)) || ldq % 16 || ldk % 16 || ldv % 8 ||
        ldo % oq || q_head % 16 || k_head % 16 || v_head % 8 || o_head % oq)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "%s: Q, K, mask and out must be 16-byte aligned and V 8-byte, and so every row and head stride (ldq=%u ldk=%u ldv=%u ldo=%u "
                    "heads %llu %llu %llu %llu)",
                    fn, ldq, ldk, ldv, ldo, static_cast<unsigned long long>(q_head), static_cast<unsigned long long>(k_head),
                    static_cast<unsigned long long>(v_head), static_cast<unsigned long long>(o_head));
    if (!aligned4(q_scale) || !aligned4(k_scale) || !aligned4(v_scale))
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: q_scale, k_scale and v_scale must be 4-byte aligned", fn);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    const uint64_t rows = static_cast<uint64_t>(numBlockRows) * bS;
    const uint64_t qs = span(rows, ldq, D), ks = span(K, ldk, D), vs = span(K, ldv, Dv);
    if (qs > 0x7FFFFFFFull || ks > 0x7FFFFFFFull || vs > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: Q, K or V of one head spans 2 GiB or more (%llu, %llu, %llu bytes)", fn,
                    static_cast<unsigned long long>(qs), static_cast<unsigned long long>(ks), static_cast<unsigned long long>(vs));
    if (rows > 0x7FFFFFFFull || rows / 16 * splits > 0xFFFFFFFFull || ceil_div64(rows / 16 * splits, kTileWaves) * H > 0x7FFFFFFFull ||
        rows / kCombineRows * H > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: %llu rows x %u heads x %u splits are more work units than one launch takes", fn,
                    static_cast<unsigned long long>(rows), H, splits);
    Fp8SplitCall c{};
    c.stream = as_stream(stream);
    c.H = H, c.Mb = numBlockRows;
    c.blockRowPtrs = blockRowPtrs, c.blockColIdxs = blockColIdxs;
    c.Q = Q, c.K = Kmat, c.V = V;
    c.q_scale = q_scale, c.k_scale = k_scale, c.v_scale = v_scale;
    c.mask = mask, c.out = out, c.lse = lse;
    c.ws_o = static_cast<float *>(workspace);
    c.ws_state = c.ws_o + static_cast<uint64_t>(H) * rows * splits * Dv;
    Fp8SplitParams &p = c.p;
    p.Kb = K / bS, p.D = D, p.Dv = Dv, p.rows = static_cast<uint32_t>(rows), p.S = splits, p.G = kv_group;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv;
    p.q_bytes = static_cast<uint32_t>(qs), p.k_bytes = static_cast<uint32_t>(ks), p.v_bytes = static_cast<uint32_t>(vs);
    p.q_head = q_head, p.k_head = k_head, p.v_head = v_head;
    p.scale = scale;
    c.c = Fp8CombineParams{p.rows, p.rows / 16u, splits, Dv, ldo, bS == 16 ? 2u : 1u, bS == 16 ? 4u : 5u, kv_group, o_head};
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_const<1, 2>(D <= 64 ? 1 : 2, [&](auto ds) {
            with_const<4, 8>(Dv <= 64 ? 4 : 8, [&](auto tpl) {
                with_flag(mask != nullptr,
                          [&](auto mk) { launch_partial<decltype(bs)::value, decltype(ds)::value, decltype(tpl)::value, decltype(mk)::value>(c); });
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    with_flag(out_bf16 != 0, [&](auto ob) { launch_combine<decltype(ob)::value>(c); });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
