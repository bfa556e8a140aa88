// libmispmm_attn_fp8.so: fused block-sparse attention forward with Q, K and V in fp8 (OCP e4m3 bytes, torch.float8_e4m3fn)
// on v_mfma_f32_16x16x32_fp8_fp8 (include/mispmm_attn_fp8.h): scores, row softmax and the product with V in ONE launch for
// all heads, per-head scales of Q, K and V applied in fp32.
//
// WORK SPLIT.  That of the bf16 forward (fused/attn_bsr_tiles.hpp, THE WORK UNIT): one wave owns 16 query rows of one head
// and walks its block row 32 keys a step, 4 waves to a workgroup, (head, unit) in XCD order; no LDS, no atomics.  Lane
// l = (i = l & 15, g = l >> 4).  What is written for this element type is everything a lane reads and feeds the MFMAs.
//
// SCORES, transposed: the step's 16 keys are the A operand, the wave's 16 query rows the B operand, and register r of the
// result is the score of query i with key 4g + r (the operand bytes as bsr_fp8/spmm_bsr_fp8.hip proves them: lane (c, g)
// holds A[c][8g .. 8g+7] and B[8g .. 8g+7][c], byte e = k slot 8g + e).  k is only a summation index, so the slots are NAMED
// to suit the reads: lane (i, g) reads the 16 consecutive bytes 64 s + 16 g .. + 15 of its K row in ONE buffer_load_dwordx4
// and feeds the low 8 to one MFMA and the high 8 to the next; Q's fragments are read once with the same naming.  The two
// MFMAs of a 64-column step of D then sum columns {64 s + 16 g + e} and {64 s + 16 g + 8 + e}, e < 8, g < 4: all 64, each
// once.  Half the K-fragment reads of an 8-byte scheme, and the reason D is a multiple of 16: a read is inside D or dropped.
//
// WEIGHTS.  w = exp(z - mu) in fp32 by the online softmax of the bf16 kernel (running maximum, mu, alpha, the -Inf and NaN
// handling, tile_exp, settle).  They enter the second MFMA as e4m3 of fl(256 w), by v_cvt_pk_fp8_f32: w in (0, 1] lands in
// (0, 256], inside e4m3's range (256 is exact), and the flush threshold moves from 2^-10 to 2^-18.  The divisor l sums the
// ROUNDED, scaled weights as the converter wrote them (read back by v_cvt_pk_f32_fp8), the numbers the product multiplies
// by: out is a convex combination of V's rows and the 2^8 cancels.  lx sums the unrounded, unscaled weights for lse.
// A lane's 8 weights of a step are its 8 k slots of the B operand of O^T += V^T P^T (slot 8g + j is key 4g + j of the first
// tile, 8g + 4 + j the same key of the second): two packed converts into each of two dwords, no lane move.
// A weight that is +Inf or NaN must poison the whole row whatever the converter makes of it: (tx - tx) is added to the
// step's sum of rounded weights, +0 while the unrounded sum tx is finite and NaN otherwise.
//
// V IN THE V LAYOUT.  Accumulator tile t of lane column c is output column TPL c + t.  The lane reads the TPL consecutive
// bytes from column TPL i of each of its 8 key rows (rows 4g .. 4g+3 of both tiles; T8: a dwordx2 per row, T4: a dword) and
// regroups them with v_perm_b32 byte transposes (transpose4, as in bsr_fp8/) into one 64-bit A operand per tile.  Lane
// (i, g) ends with acc[t][k] = O[i][TPL (4g + k) + t]: the store is a run of TPL consecutive columns for every k.
//
// LOADS go through buffer descriptors of each head's exact span; an absent tile (a block column at or past K / bS, the
// missing half of a half step, a step past the end) and columns at or past the width take the dropped-load offset.  The
// next step's loads are issued one step ahead into the other of two named stages, the block columns one step further ahead
// by scalar loads.  The scales are read by scalar loads once per wave.
// The unit lies outside csrc/ and fused/: the census tests hold those directories and their libraries to their records.
#include "../fused/attn_bsr_tiles.hpp"
#include "mispmm_attn_fp8.h"

namespace mispmm {

namespace {

struct Fp8Params {
    uint32_t units, wgs_per_head, total, xcd_chunk;  // units: 16-row work units of one head; total: workgroups of all heads
    uint32_t Kb, D, Dv, rows;                        // rows = numBlockRows * bS
    uint32_t ldq, ldk, ldv, ldo;                     // row strides in elements; for Q, K and V those are bytes
    uint32_t q_bytes, k_bytes, v_bytes;              // one head's span: (rows - 1) * ld + width
    float scale;
    uint64_t q_head, k_head, v_head, o_head;         // elements
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

// the two 8-byte operands of a 16-byte read: slots named so that the low half goes to one MFMA, the high half to the next
__device__ __forceinline__ long low8(u32x4_t v) { return __builtin_bit_cast(long, u32x2_t{v[0], v[1]}); }
__device__ __forceinline__ long high8(u32x4_t v) { return __builtin_bit_cast(long, u32x2_t{v[2], v[3]}); }

__device__ __forceinline__ f32x4_t mfma8(long a, long b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0); }

// BS: block size.  DS: 64-column steps of D held (D <= 64 DS).  TPL: accumulator tiles = consecutive V bytes per lane
// (Dv <= 16 TPL).  The arrays are kernel arguments of their own, `const __restrict__`: block columns and scales come by
// scalar loads.
template <int BS, int DS, int TPL, bool MASK, bool OUT_BF16>
__global__ void __launch_bounds__(64 * kTileWaves)
    attn_bsr_fp8_kernel(const Fp8Params p, const uint32_t *__restrict__ blockRowPtrs, const uint32_t *__restrict__ blockColIdxs,
                        const uint8_t *__restrict__ Q, const uint8_t *__restrict__ K, const uint8_t *__restrict__ V,
                        const float *__restrict__ q_scale, const float *__restrict__ k_scale, const float *__restrict__ v_scale,
                        const float *__restrict__ mask, void *__restrict__ out, float *__restrict__ lse_out) {
    static_assert((BS == 16 || BS == 32) && (DS == 1 || DS == 2) && (TPL == 4 || TPL == 8), "the instances of the header");
    using W = Walk<BS>;
    constexpr int VW = TPL / 4;  // dwords of one V row read
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t item = xcd_block(blockIdx.x, p.xcd_chunk);
    if (item >= p.total) return;
    const uint32_t h = item / p.wgs_per_head;
    const uint32_t unit = (item - h * p.wgs_per_head) * kTileWaves + wave;
    if (unit >= p.units) return;
    const uint32_t R = unit / W::T, sub = unit % W::T;
    const uint32_t i = lane & 15, g = lane >> 4;
    const uint32_t row = unit * 16u + i;  // < rows
    const uint32_t bs = blockRowPtrs[R], be = blockRowPtrs[R + 1];
    const float ninf = -__builtin_huge_valf();

    f32x4_t acc[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // out = fl(fl(O * inv) * vs), two multiplies; by_v false: the first alone.  For every k a run of TPL consecutive columns
    auto store = [&](float inv, bool by_v, float vs, float lse) {
        const size_t base = static_cast<size_t>(h) * p.o_head + static_cast<size_t>(row) * p.ldo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t col = TPL * (4u * g + k);
            if (col >= p.Dv) continue;
            float v[TPL];
#pragma unroll
            for (int t = 0; t < TPL; ++t) {
                v[t] = acc[t][k] * inv;
                const float scaled_v = v[t] * vs;
                v[t] = by_v ? scaled_v : v[t];
            }
            if constexpr (OUT_BF16) {
                uint32_t o[TPL / 2];
#pragma unroll
                for (int w = 0; w < TPL / 2; ++w)
                    o[w] = __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(v[2 * w]), static_cast<__bf16>(v[2 * w + 1])});
                uint16_t *dst = static_cast<uint16_t *>(out) + base + col;
                if constexpr (TPL == 8) *reinterpret_cast<u32x4_t *>(dst) = u32x4_t{o[0], o[1], o[2], o[3]};
                else *reinterpret_cast<u32x2_t *>(dst) = u32x2_t{o[0], o[1]};
            } else {
                float *dst = static_cast<float *>(out) + base + col;
#pragma unroll
                for (int w = 0; w < TPL / 4; ++w)
                    *reinterpret_cast<f32x4_t *>(dst + 4 * w) = f32x4_t{v[4 * w], v[4 * w + 1], v[4 * w + 2], v[4 * w + 3]};
            }
        }
        if (lse_out && g == 0) lse_out[static_cast<size_t>(h) * p.rows + row] = lse;
    };
    if (be <= bs) {  // an empty block row: +0 whatever the scales hold, lse = log 0
        store(1.f, false, 1.f, ninf);
        return;
    }

    // c_h = fl(fl(scale * q_scale[h]) * k_scale[h]), once per wave; a NULL scale is no multiply
    float c_h = p.scale;
    if (q_scale) c_h = c_h * q_scale[h];
    if (k_scale) c_h = c_h * k_scale[h];
    const bool by_v = v_scale != nullptr;
    const float vs = by_v ? v_scale[h] : 1.f;

    auto settle_acc = [&] { settle<TPL>(acc); };

    const rsrc_t qr = make_rsrc(Q + h * p.q_head, p.q_bytes), kr = make_rsrc(K + h * p.k_head, p.k_bytes), vr = make_rsrc(V + h * p.v_head, p.v_bytes);
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

    // the block columns behind the two 16-key tiles of the step that starts at block e (bS = 32: one block); past the row's end: none
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
    constexpr uint32_t kSecond = W::kSecond, EPS = W::EPS;
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
        if constexpr (MASK) {  // a step past the row's end re-reads the row's last block: valid memory, never used
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

    auto step = [&](const Stage &use, Stage &fill) {
        const Cols after = cols_at(e + 2 * EPS);
        load_stage(nxt, e + EPS, fill);
        const bool second = BS == 32 || e + 1 < be;  // wave-uniform: a half step has no second tile
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
            const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(d, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(d, true);
            t = t + lo[0];
            t = t + lo[1];
            t = t + hi[0];
            t = t + hi[1];
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
            uint32_t lo[4], hi[4];
            transpose4(use.v[0][w], use.v[1][w], use.v[2][w], use.v[3][w], lo);
            transpose4(use.v[4][w], use.v[5][w], use.v[6][w], use.v[7][w], hi);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * w + j] = mfma8(__builtin_bit_cast(long, u32x2_t{lo[j], hi[j]}), pfrag, acc[4 * w + j]);
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
    store(1.f / l, by_v, vs, mu + __builtin_logf(lx));
}

struct Fp8Call {
    hipStream_t stream;
    uint32_t H, Mb;
    Fp8Params p;
    const uint32_t *blockRowPtrs, *blockColIdxs;
    const uint8_t *Q, *K, *V;
    const float *q_scale, *k_scale, *v_scale, *mask;
    void *out;
    float *lse;
};

template <int BS, int DS, int TPL, bool MASK, bool OUT_BF16>
void launch_attn_fp8(const Fp8Call &c) {
    Fp8Params p = c.p;
    const uint32_t grid = finish_grid(p, c.Mb * (BS / 16), c.H);
    note_kernel("attn_bsr_fp8<b%d,%s,%s,D%d,T%d>", BS, OUT_BF16 ? "bf16" : "f32", MASK ? "mask" : "nomask", DS, TPL);
    hipLaunchKernelGGL((attn_bsr_fp8_kernel<BS, DS, TPL, MASK, OUT_BF16>), dim3(grid), dim3(64 * kTileWaves), 0, c.stream, p, c.blockRowPtrs,
                       c.blockColIdxs, c.Q, c.K, c.V, c.q_scale, c.k_scale, c.v_scale, c.mask, c.out, c.lse);
}

bool aligned4(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 3u) == 0; }

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_attn_bsr_fp8(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                                   const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint8_t *Q, uint32_t ldq, uint64_t q_head,
                                   const uint8_t *Kmat, uint32_t ldk, uint64_t k_head, const uint8_t *V, uint32_t ldv, uint64_t v_head,
                                   uint32_t D, uint32_t Dv, const float *mask, float scale, const float *q_scale, const float *k_scale,
                                   const float *v_scale, void *out, uint32_t ldo, uint64_t o_head, int out_bf16, float *lse) {
    constexpr const char *fn = "attn_bsr_fp8";
    if (const int refused = refuse_shape(fn, bS, scale, D, Dv, K)) return refused;
    if (D % 16 != 0)  // a lane reads 16 bytes of a row of Q or K: wholly inside D or wholly dropped
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: D must be a multiple of 16 from 16 to 128 (got D=%u)", fn, D);
    if (H == 0 || numBlockRows == 0) return MISPMM_OK;
    if (!blockRowPtrs || !Q || !Kmat || !V || !out || (numBlocks != 0 && !blockColIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: blockRowPtrs, blockColIdxs, Q, K, V or out is null", fn);
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)", fn, D, ldq,
                    ldk, Dv, ldv, ldo);
    // a lane reads 16 bytes of Q and K, 8 (T4: 4) of V and 16 of the mask, and writes 16 (a 64-column bf16 out: 8)
    const uint32_t oq = out_bf16 ? 8u : 4u;  // elements of out to 16 bytes
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
    if (rows > 0x7FFFFFFFull || ceil_div64(rows / 16, kTileWaves) * H > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: %llu rows x %u heads are more work units than one launch takes", fn,
                    static_cast<unsigned long long>(rows), H);
    Fp8Call c{};
    c.stream = as_stream(stream);
    c.H = H;
    c.Mb = numBlockRows;
    c.blockRowPtrs = blockRowPtrs, c.blockColIdxs = blockColIdxs;
    c.Q = Q, c.K = Kmat, c.V = V;
    c.q_scale = q_scale, c.k_scale = k_scale, c.v_scale = v_scale;
    c.mask = mask, c.out = out, c.lse = lse;
    Fp8Params &p = c.p;
    p.Kb = K / bS, p.D = D, p.Dv = Dv, p.rows = static_cast<uint32_t>(rows);
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo;
    p.q_bytes = static_cast<uint32_t>(qs), p.k_bytes = static_cast<uint32_t>(ks), p.v_bytes = static_cast<uint32_t>(vs);
    p.q_head = q_head, p.k_head = k_head, p.v_head = v_head, p.o_head = o_head;
    p.scale = scale;
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_const<1, 2>(D <= 64 ? 1 : 2, [&](auto ds) {
            with_const<4, 8>(Dv <= 64 ? 4 : 8, [&](auto tpl) {
                with_flag(mask != nullptr, [&](auto mk) {
                    with_flag(out_bf16 != 0, [&](auto ob) {
                        launch_attn_fp8<decltype(bs)::value, decltype(ds)::value, decltype(tpl)::value, decltype(mk)::value, decltype(ob)::value>(c);
                    });
                });
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
