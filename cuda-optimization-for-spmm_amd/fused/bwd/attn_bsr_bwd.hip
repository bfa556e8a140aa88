// Fused block-sparse attention backward in bf16 (mispmm_attn_bwd.h): dQ, dK and dV of mispmm_attn_bsr_bf16 for all heads in
// two launches.  Neither S, P, dP nor dS is written: a pass recomputes the scores of the blocks it walks from Q and K and
// turns them into weights with the forward's per-row log-sum-exp.
//   z[r][key]  = fl32(scale * <Q[r], K[key]> + mask)      the forward's z: the same MFMA, the same fma
//   P          = exp(z - lse[r])                          v_exp_f32 of fl(t * log2 e), as the forward
//   dP         = <dO[r, :Dv], V[key, :Dv]>                MFMA, fp32
//   dS         = fl(fl(P * fl(dP - delta[r])) * scale)    delta[r] = sum_c dO[r][c] * O[r][c]
//   dQ[r]      = sum_key bf16(dS) K[key]      dK[key] = sum_r bf16(dS) Q[r]      dV[key] = sum_r bf16(P) dO[r]
//
// Work unit, lane layout of the transposed products, the V layout, loads and settle(): ../attn_bsr_tiles.hpp.
//
// THE ROW PASS.  One wave owns 16 query rows of one head and walks its block row 32 keys at a step.  Q's and dO's fragments
// stay in registers; K rows resp. V rows are the A operands of the two score products, so lane (i, g) holds query i x keys
// 4g .. 4g + 3 of both 16-key tiles for S AND dP: lse[i] and delta[i] are lane-local and dS needs no cross-lane move.
// dQ^T += K^T dS^T: K is read a second time in the V layout.  Before the walk the wave forms delta of its 16 rows from the dO
// fragments it holds and the same columns of O (a lane sum by fma, columns ascending, then (g0 + g1) + (g2 + g3) by two xor
// moves) and writes it to the caller's workspace.  Without dQ the pass stops there.
//
// THE COLUMN PASS is its mirror on A^T's pattern.  One wave owns 16 keys of one head, holds their K and V fragments as the B
// operands (the lane then holds key i x queries 4g .. 4g + 3) and walks the block column 32 queries at a step: Q and dO rows
// as A operands for S and dP, lse and delta of the lane's 8 queries (two 16-byte loads each), the mask through perm, and Q
// and dO a second time in the V layout for dK^T += Q^T dS and dV^T += dO^T P.  It follows the row pass on the same stream: it
// reads delta.
//
// One register stage: a step's loads are issued together at its top and the MFMAs wait for them; the latency is left to the
// other waves of the SIMD (two stages do not fit at D = Dv = 128).  The accumulators are only
// ever touched by MFMAs inside the loop, so the XDL-write to VALU-read wait settle() spells out is needed
// once: on the edge out of the loop, before the store.  No LDS, no barrier, no atomics; every sum has a fixed order.
#include "../attn_bsr_tiles.hpp"
#include "mispmm_attn_bwd.h"

namespace mispmm {

namespace {

struct BwdParams {
    uint32_t units, wgs_per_head, total, xcd_chunk;  // units: 16-row (16-key) work units of one head
    uint32_t Mb, Kb, D, Dv, rows;                    // rows = Mb * bS queries; Kb * bS keys
    uint32_t ldq2, ldk2, ldv2, ldg2;                 // row strides in bytes
    uint32_t q_bytes, k_bytes, v_bytes, g_bytes;     // one head's span
    uint32_t ldo, lddq, lddk, lddv;                  // elements
    uint32_t out_bf16, grads_bf16, want_dq, want_dk, want_dv;
    float scale;
    uint64_t q_head, k_head, v_head, g_head, o_head, dq_head, dk_head, dv_head;  // elements
};

// the weights and dS of the lane's 8 elements of a step, as the two bf16 B operands.  ls / dl: lse and delta of the
// element's query; a tile that is not there contributes +0.
__device__ __forceinline__ void weights(const float (&z)[8], const float (&dp)[8], const float (&ls)[8], const float (&dl)[8], float scale, bool first,
                                        bool second, bf16x8_t &pfrag, bf16x8_t &dsfrag) {
    u32x4_t pw, dw;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        float pv[2], dv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = 2 * w + u;
            const bool there = j < 4 ? first : second;  // wave-uniform
            const float pj = tile_exp(z[j] - ls[j]);
            const float t = dp[j] - dl[j];
            pv[u] = there ? pj : 0.f;
            dv[u] = there ? (pj * t) * scale : 0.f;
        }
        pw[w] = __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(pv[0]), static_cast<__bf16>(pv[1])});
        dw[w] = __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(dv[0]), static_cast<__bf16>(dv[1])});
    }
    pfrag = __builtin_bit_cast(bf16x8_t, pw);
    dsfrag = __builtin_bit_cast(bf16x8_t, dw);
}

// BS: block size.  DS / DSV: 32-column steps of D / Dv held (D <= 32 DS, Dv <= 32 DSV); dQ has 2 DS accumulator tiles.
template <int BS, int DS, int DSV, bool MASK>
__global__ void __launch_bounds__(64 * kTileWaves)
    attn_bwd_rows_kernel(const BwdParams p, const uint32_t *__restrict__ blockRowPtrs, const uint32_t *__restrict__ blockColIdxs,
                         const uint16_t *__restrict__ Q, const uint16_t *__restrict__ K, const uint16_t *__restrict__ V, const uint16_t *__restrict__ G,
                         const void *__restrict__ O, const float *__restrict__ lse, const float *__restrict__ mask, float *__restrict__ delta,
                         void *__restrict__ dQ) {
    using W = Walk<BS>;
    constexpr uint32_t EPS = W::EPS, kSecond = W::kSecond;
    constexpr int TPL = 2 * DS;
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
    const uint32_t kcol = g * 8u;         // the lane's 8 columns of a 32-column step

    const rsrc_t gr = make_rsrc(G + h * p.g_head, p.g_bytes);
    bf16x8_t gf[DSV];
#pragma unroll
    for (int s = 0; s < DSV; ++s) gf[s] = load_frag(gr, row * p.ldg2, s * 32u + kcol, p.Dv);

    // delta: the lane's columns ascending by fma, then the four lanes of the row
    float dl = 0.f;
    {
        const size_t obase = static_cast<size_t>(h) * p.o_head + static_cast<size_t>(row) * p.ldo;
#pragma unroll
        for (int s = 0; s < DSV; ++s) {
            const uint32_t col = s * 32u + kcol;
            if (col >= p.Dv) continue;
            float o[8];
            if (p.out_bf16) {
                const u32x4_t raw = *reinterpret_cast<const u32x4_t *>(static_cast<const uint16_t *>(O) + obase + col);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    o[2 * w] = __uint_as_float(raw[w] << 16);
                    o[2 * w + 1] = __uint_as_float(raw[w] & 0xFFFF0000u);
                }
            } else {
                const f32x4_t lo = *reinterpret_cast<const f32x4_t *>(static_cast<const float *>(O) + obase + col);
                const f32x4_t hi = *reinterpret_cast<const f32x4_t *>(static_cast<const float *>(O) + obase + col + 4);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    o[w] = lo[w];
                    o[4 + w] = hi[w];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                dl = __builtin_fmaf(__uint_as_float(static_cast<uint32_t>(static_cast<uint16_t>(gf[s][j])) << 16), o[j], dl);
        }
        dl = dl + lane_xor<16>(dl);
        dl = dl + lane_xor<32>(dl);
        if (g == 0) delta[static_cast<size_t>(h) * p.rows + row] = dl;
    }
    if (!p.want_dq) return;

    f32x4_t acc[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const size_t dq_at = static_cast<size_t>(h) * p.dq_head + static_cast<size_t>(row) * p.lddq;
    const uint32_t bs = blockRowPtrs[R], be = blockRowPtrs[R + 1];
    if (be <= bs) {  // an empty block row: +0 rows
        store_tiles<TPL>(acc, dQ, dq_at, g, p.D, 1.f, p.grads_bf16 != 0);
        return;
    }

    const rsrc_t qr = make_rsrc(Q + h * p.q_head, p.q_bytes), kr = make_rsrc(K + h * p.k_head, p.k_bytes), vr = make_rsrc(V + h * p.v_head, p.v_bytes);
    bf16x8_t qf[DS];
#pragma unroll
    for (int s = 0; s < DS; ++s) qf[s] = load_frag(qr, row * p.ldq2, s * 32u + kcol, p.D);
    const float ls = lse[static_cast<size_t>(h) * p.rows + row];

    // the lane's share of a load's offset (attn_bsr_tiles.hpp, LOADS): row i of a 16-key tile and the lane's columns for the A operands of
    // the two score products, rows 4g + j and columns TPL * i .. for K in the V layout
    uint32_t koff[DS], voff[DSV], ktoff[4];
#pragma unroll
    for (int s = 0; s < DS; ++s) koff[s] = s * 32u + kcol < p.D ? i * p.ldk2 + (s * 32u + kcol) * 2u : kDropLoad;
#pragma unroll
    for (int s = 0; s < DSV; ++s) voff[s] = s * 32u + kcol < p.Dv ? i * p.ldv2 + (s * 32u + kcol) * 2u : kDropLoad;
    const uint32_t tcol = i * TPL;
#pragma unroll
    for (int j = 0; j < 4; ++j) ktoff[j] = tcol < p.D ? (4u * g + j) * p.ldk2 + tcol * 2u : kDropLoad;
    const size_t mask_at = static_cast<size_t>(sub * 16u + i) * BS + 4u * g;
    const uint32_t last = be - 1;
    float lsv[8], dlv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) lsv[j] = ls, dlv[j] = dl;

    for (uint32_t e = bs; e < be; e += EPS) {
        const bool second = BS == 32 || e + 1 < be;  // wave-uniform: a half step has no second tile
        const uint32_t ca = blockColIdxs[e], cb = BS == 32 ? ca : blockColIdxs[min(e + 1, last)];
        const bool va = ca < p.Kb, vb = second && cb < p.Kb;  // a block column at or past K / bS reads zeros
        const uint32_t ra = va ? ca * BS : 0u, rb = vb ? cb * BS + kSecond : 0u;
        bf16x8_t ka[2][DS], vv[2][DSV];
#pragma unroll
        for (int s = 0; s < DS; ++s) {
            ka[0][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(kr, va ? koff[s] : kDropLoad, ra * p.ldk2, 0));
            ka[1][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(kr, vb ? koff[s] : kDropLoad, rb * p.ldk2, 0));
        }
#pragma unroll
        for (int s = 0; s < DSV; ++s) {
            vv[0][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(vr, va ? voff[s] : kDropLoad, ra * p.ldv2, 0));
            vv[1][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(vr, vb ? voff[s] : kDropLoad, rb * p.ldv2, 0));
        }
        f32x4_t ma{0.f, 0.f, 0.f, 0.f}, mb{0.f, 0.f, 0.f, 0.f};
        if constexpr (MASK) {
            const size_t ea = static_cast<size_t>(e) * (BS * BS);
            const size_t eb = BS == 32 ? ea + 16u : static_cast<size_t>(min(e + 1, last)) * (BS * BS);
            ma = *reinterpret_cast<const f32x4_t *>(mask + ea + mask_at);
            mb = *reinterpret_cast<const f32x4_t *>(mask + eb + mask_at);
        }
        TRows<TPL> kt;
        load_trows<TPL>(kt, kr, ktoff, va, vb, ra * p.ldk2, rb * p.ldk2);

        f32x4_t sa{0.f, 0.f, 0.f, 0.f}, sb{0.f, 0.f, 0.f, 0.f}, da{0.f, 0.f, 0.f, 0.f}, db{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DS; ++s) sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[0][s], qf[s], sa, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < DS; ++s) sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[1][s], qf[s], sb, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < DSV; ++s) da = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vv[0][s], gf[s], da, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < DSV; ++s) db = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vv[1][s], gf[s], db, 0, 0, 0);
        float z[8], dp[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            z[j] = scaled<MASK>(p.scale, sa[j], ma, j);
            z[4 + j] = scaled<MASK>(p.scale, sb[j], mb, j);
            dp[j] = da[j];
            dp[4 + j] = db[j];
        }
        bf16x8_t pfrag, dsfrag;
        weights(z, dp, lsv, dlv, p.scale, true, second, pfrag, dsfrag);
        mfma_trows<TPL>(acc, kt, dsfrag);
    }
    settle<TPL>(acc);
    store_tiles<TPL>(acc, dQ, dq_at, g, p.D, 1.f, p.grads_bf16 != 0);
}

// the mirror on A^T's pattern: one wave owns 16 keys; dK has 2 DS accumulator tiles, dV 2 DSV
template <int BS, int DS, int DSV, bool MASK>
__global__ void __launch_bounds__(64 * kTileWaves)
    attn_bwd_cols_kernel(const BwdParams p, const uint32_t *__restrict__ tRowPtrs, const uint32_t *__restrict__ tColIdxs,
                         const uint32_t *__restrict__ perm, const uint16_t *__restrict__ Q, const uint16_t *__restrict__ K,
                         const uint16_t *__restrict__ V, const uint16_t *__restrict__ G, const float *__restrict__ lse, const float *__restrict__ delta,
                         const float *__restrict__ mask, void *__restrict__ dK, void *__restrict__ dV) {
    using W = Walk<BS>;
    constexpr uint32_t EPS = W::EPS, kSecond = W::kSecond;
    constexpr int TK = 2 * DS, TV = 2 * DSV;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t item = xcd_block(blockIdx.x, p.xcd_chunk);
    if (item >= p.total) return;
    const uint32_t h = item / p.wgs_per_head;
    const uint32_t unit = (item - h * p.wgs_per_head) * kTileWaves + wave;
    if (unit >= p.units) return;
    const uint32_t C = unit / W::T, sub = unit % W::T;
    const uint32_t i = lane & 15, g = lane >> 4;
    const uint32_t key = unit * 16u + i;  // < Kb * bS
    const uint32_t kcol = g * 8u;
    const bool want_dk = p.want_dk != 0, want_dv = p.want_dv != 0;  // wave-uniform

    f32x4_t acck[TK], accv[TV];
#pragma unroll
    for (int t = 0; t < TK; ++t) acck[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TV; ++t) accv[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const size_t dk_at = static_cast<size_t>(h) * p.dk_head + static_cast<size_t>(key) * p.lddk;
    const size_t dv_at = static_cast<size_t>(h) * p.dv_head + static_cast<size_t>(key) * p.lddv;
    const uint32_t bs = tRowPtrs[C], be = tRowPtrs[C + 1];
    if (be > bs) {
        const rsrc_t qr = make_rsrc(Q + h * p.q_head, p.q_bytes), kr = make_rsrc(K + h * p.k_head, p.k_bytes);
        const rsrc_t vr = make_rsrc(V + h * p.v_head, p.v_bytes), gr = make_rsrc(G + h * p.g_head, p.g_bytes);
        bf16x8_t kf[DS], vf[DSV];
#pragma unroll
        for (int s = 0; s < DS; ++s) kf[s] = load_frag(kr, key * p.ldk2, s * 32u + kcol, p.D);
#pragma unroll
        for (int s = 0; s < DSV; ++s) vf[s] = load_frag(vr, key * p.ldv2, s * 32u + kcol, p.Dv);
        uint32_t qoff[DS], goff[DSV], qtoff[4], gtoff[4];
#pragma unroll
        for (int s = 0; s < DS; ++s) qoff[s] = s * 32u + kcol < p.D ? i * p.ldq2 + (s * 32u + kcol) * 2u : kDropLoad;
#pragma unroll
        for (int s = 0; s < DSV; ++s) goff[s] = s * 32u + kcol < p.Dv ? i * p.ldg2 + (s * 32u + kcol) * 2u : kDropLoad;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            qtoff[j] = i * TK < p.D ? (4u * g + j) * p.ldq2 + i * TK * 2u : kDropLoad;
            gtoff[j] = i * TV < p.Dv ? (4u * g + j) * p.ldg2 + i * TV * 2u : kDropLoad;
        }
            const uint32_t last = be - 1;
        const float *lse_h = lse + static_cast<size_t>(h) * p.rows + 4u * g;
        const float *delta_h = delta + static_cast<size_t>(h) * p.rows + 4u * g;
        const size_t mask_at = static_cast<size_t>(4u * g) * BS + sub * 16u + i;  // query 4g, key i of the wave's half

        for (uint32_t e = bs; e < be; e += EPS) {
            const bool second = BS == 32 || e + 1 < be;
            const uint32_t ea = e, eb = BS == 32 ? e : min(e + 1, last);
            const uint32_t ca = tColIdxs[ea], cb = BS == 32 ? ca : tColIdxs[eb];
            const bool va = ca < p.Mb, vb = second && cb < p.Mb;  // a block row of A that is not there: nothing
            // first query of each tile.  A tile that is not there takes query 0: its Q and dO loads are dropped (zeros) and its
            // lse, delta and mask loads read valid memory of row 0 / the block column's last block, never used -- weights()
            // selects +0 for the tile's P and dS
            const uint32_t ra = va ? ca * BS : 0u, rb = vb ? cb * BS + kSecond : 0u;
            bf16x8_t qa[2][DS], ga[2][DSV];
#pragma unroll
            for (int s = 0; s < DS; ++s) {
                qa[0][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(qr, va ? qoff[s] : kDropLoad, ra * p.ldq2, 0));
                qa[1][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(qr, vb ? qoff[s] : kDropLoad, rb * p.ldq2, 0));
            }
            float z[8], dp[8], lsv[8], dlv[8];
            {
                const f32x4_t la = *reinterpret_cast<const f32x4_t *>(lse_h + ra), lb = *reinterpret_cast<const f32x4_t *>(lse_h + rb);
#pragma unroll
                for (int j = 0; j < 4; ++j) lsv[j] = la[j], lsv[4 + j] = lb[j];
            }
            float mk[8];
            if constexpr (MASK) {
                const size_t pa = static_cast<size_t>(perm[ea]) * (BS * BS), pb = static_cast<size_t>(perm[eb]) * (BS * BS) + kSecond * BS;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    mk[j] = mask[pa + mask_at + j * BS];
                    mk[4 + j] = mask[pb + mask_at + j * BS];
                }
            }
            TRows<TK> qt;
            TRows<TV> gt;
            if (want_dk) {
#pragma unroll
                for (int s = 0; s < DSV; ++s) {
                    ga[0][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(gr, va ? goff[s] : kDropLoad, ra * p.ldg2, 0));
                    ga[1][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(gr, vb ? goff[s] : kDropLoad, rb * p.ldg2, 0));
                }
                const f32x4_t xa = *reinterpret_cast<const f32x4_t *>(delta_h + ra), xb = *reinterpret_cast<const f32x4_t *>(delta_h + rb);
#pragma unroll
                for (int j = 0; j < 4; ++j) dlv[j] = xa[j], dlv[4 + j] = xb[j];
                load_trows<TK>(qt, qr, qtoff, va, vb, ra * p.ldq2, rb * p.ldq2);
            }
            if (want_dv) load_trows<TV>(gt, gr, gtoff, va, vb, ra * p.ldg2, rb * p.ldg2);

            f32x4_t sa{0.f, 0.f, 0.f, 0.f}, sb{0.f, 0.f, 0.f, 0.f}, da{0.f, 0.f, 0.f, 0.f}, db{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < DS; ++s) sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[0][s], kf[s], sa, 0, 0, 0);
#pragma unroll
            for (int s = 0; s < DS; ++s) sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[1][s], kf[s], sb, 0, 0, 0);
            if (want_dk) {
#pragma unroll
                for (int s = 0; s < DSV; ++s) da = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[0][s], vf[s], da, 0, 0, 0);
#pragma unroll
                for (int s = 0; s < DSV; ++s) db = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[1][s], vf[s], db, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                z[j] = scaled<MASK>(p.scale, sa[j], mk, j);
                z[4 + j] = scaled<MASK>(p.scale, sb[j], mk, 4 + j);
                dp[j] = da[j];
                dp[4 + j] = db[j];
                if (!want_dk) dlv[j] = 0.f, dlv[4 + j] = 0.f;
            }
            bf16x8_t pfrag, dsfrag;
            weights(z, dp, lsv, dlv, p.scale, va, vb, pfrag, dsfrag);
            if (want_dv) mfma_trows<TV>(accv, gt, pfrag);
            if (want_dk) mfma_trows<TK>(acck, qt, dsfrag);
        }
        if (want_dk) settle<TK>(acck);
        if (want_dv) settle<TV>(accv);
    }
    // an empty block column: +0 rows
    if (want_dk) store_tiles<TK>(acck, dK, dk_at, g, p.D, 1.f, p.grads_bf16 != 0);
    if (want_dv) store_tiles<TV>(accv, dV, dv_at, g, p.Dv, 1.f, p.grads_bf16 != 0);
}

struct BwdCall {
    hipStream_t stream;
    uint32_t H;
    BwdParams p;
    const uint32_t *rowPtrs, *colIdxs, *tRowPtrs, *tColIdxs, *perm;
    const uint16_t *Q, *K, *V, *G;
    const void *O;
    const float *lse, *mask;
    float *delta;
    void *dQ, *dK, *dV;
};

template <int BS, int DS, int DSV, bool MASK>
void launch_rows(const BwdCall &c) {
    BwdParams p = c.p;
    const uint32_t grid = finish_grid(p, p.Mb * (BS / 16), c.H);
    hipLaunchKernelGGL((attn_bwd_rows_kernel<BS, DS, DSV, MASK>), dim3(grid), dim3(64 * kTileWaves), 0, c.stream, p, c.rowPtrs, c.colIdxs, c.Q, c.K,
                       c.V, c.G, c.O, c.lse, c.mask, c.delta, c.dQ);
}

template <int BS, int DS, int DSV, bool MASK>
void launch_cols(const BwdCall &c) {
    BwdParams p = c.p;
    const uint32_t grid = finish_grid(p, p.Kb * (BS / 16), c.H);
    hipLaunchKernelGGL((attn_bwd_cols_kernel<BS, DS, DSV, MASK>), dim3(grid), dim3(64 * kTileWaves), 0, c.stream, p, c.tRowPtrs, c.tColIdxs, c.perm,
                       c.Q, c.K, c.V, c.G, c.lse, c.delta, c.mask, c.dK, c.dV);
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_attn_bsr_bwd_bf16(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                                        const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint32_t *tBlockRowPtrs,
                                        const uint32_t *tBlockColIdxs, const uint32_t *perm, const uint16_t *Q, uint32_t ldq, uint64_t q_head,
                                        const uint16_t *Kmat, uint32_t ldk, uint64_t k_head, const uint16_t *V, uint32_t ldv, uint64_t v_head,
                                        const uint16_t *dO, uint32_t ldg, uint64_t g_head, const void *out, uint32_t ldo, uint64_t o_head,
                                        int out_bf16, const float *lse, float *delta, uint32_t D, uint32_t Dv, const float *mask, float scale,
                                        void *dQ, uint32_t lddq, uint64_t dq_head, void *dK, uint32_t lddk, uint64_t dk_head, void *dV,
                                        uint32_t lddv, uint64_t dv_head, int grads_bf16) {
    if (const int refused = refuse_shape("attn_bsr_bwd_bf16", bS, scale, D, Dv, K)) return refused;
    if (H == 0 || numBlockRows == 0 || (!dQ && !dK && !dV)) return MISPMM_OK;
    const bool rows_pass = dQ || dK, cols_pass = (dK || dV) && K != 0;
    if (!blockRowPtrs || !Q || !Kmat || !V || !dO || !lse || (numBlocks != 0 && !blockColIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_bwd_bf16: blockRowPtrs, blockColIdxs, Q, K, V, dO or lse is null");
    if ((dK || dV) && (!tBlockRowPtrs || (numBlocks != 0 && !tBlockColIdxs)))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_bwd_bf16: tBlockRowPtrs or tBlockColIdxs is null and dK or dV is asked for");
    if ((dK || dV) && mask && numBlocks != 0 && !perm)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_bwd_bf16: perm is null and dK or dV is asked for with a mask");
    if (rows_pass && (!out || !delta)) return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_bwd_bf16: out or delta is null and dQ or dK is asked for");
    if (ldq < D || ldk < D || ldv < Dv || ldg < Dv || (rows_pass && ldo < Dv) || (dQ && lddq < D) || (dK && lddk < D) || (dV && lddv < Dv))
        return fail(MISPMM_ERR_INVALID_ARG,
                    "attn_bsr_bwd_bf16: leading dimension smaller than the width (D=%u ldq=%u ldk=%u lddq=%u lddk=%u, Dv=%u ldv=%u ldg=%u ldo=%u "
                    "lddv=%u)",
                    D, ldq, ldk, lddq, lddk, Dv, ldv, ldg, ldo, lddv);
    // every lane reads and writes 16-byte (a 64-column bf16 gradient: 8-byte) vectors
    const uint32_t oq = out_bf16 ? 8u : 4u, gq = grads_bf16 ? 8u : 4u;  // elements to 16 bytes
    if (!aligned16(Q) || !aligned16(Kmat) || !aligned16(V) || !aligned16(dO) || !aligned16(lse) || (mask && !aligned16(mask)) ||
        (rows_pass && (!aligned16(out) || !aligned16(delta) || ldo % oq || o_head % oq)) || ldq % 8 || ldk % 8 || ldv % 8 || ldg % 8 || q_head % 8 ||
        k_head % 8 || v_head % 8 || g_head % 8 || (dQ && (!aligned16(dQ) || lddq % gq || dq_head % gq)) ||
        (dK && (!aligned16(dK) || lddk % gq || dk_head % gq)) || (dV && (!aligned16(dV) || lddv % gq || dv_head % gq)))
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "attn_bsr_bwd_bf16: Q, K, V, dO, out, lse, delta, mask, dQ, dK and dV must be 16-byte aligned, and so every row and head "
                    "stride (ldq=%u ldk=%u ldv=%u ldg=%u ldo=%u lddq=%u lddk=%u lddv=%u)",
                    ldq, ldk, ldv, ldg, ldo, lddq, lddk, lddv);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load; the outputs keep the limit
    const uint64_t rows = static_cast<uint64_t>(numBlockRows) * bS;
    const uint64_t qs = span(rows, ldq, D) * 2u, ks = span(K, ldk, D) * 2u, vs = span(K, ldv, Dv) * 2u, gs = span(rows, ldg, Dv) * 2u;
    const uint64_t os = rows_pass ? span(rows, ldo, Dv) * (out_bf16 ? 2u : 4u) : 0, ge = grads_bf16 ? 2u : 4u;
    const uint64_t dqs = dQ ? span(rows, lddq, D) * ge : 0, dks = dK ? span(K, lddk, D) * ge : 0, dvs = dV ? span(K, lddv, Dv) * ge : 0;
    for (const uint64_t s : {qs, ks, vs, gs, os, dqs, dks, dvs})
        if (s > 0x7FFFFFFFull)
            return fail(MISPMM_ERR_UNSUPPORTED,
                        "attn_bsr_bwd_bf16: an operand of one head spans 2 GiB or more (Q %llu, K %llu, V %llu, dO %llu, out %llu, dQ %llu, dK %llu, "
                        "dV %llu bytes)",
                        static_cast<unsigned long long>(qs), static_cast<unsigned long long>(ks), static_cast<unsigned long long>(vs),
                        static_cast<unsigned long long>(gs), static_cast<unsigned long long>(os), static_cast<unsigned long long>(dqs),
                        static_cast<unsigned long long>(dks), static_cast<unsigned long long>(dvs));
    if (rows > 0x7FFFFFFFull || ceil_div64(rows / 16, kTileWaves) * H > 0x7FFFFFFFull || ceil_div64(K / 16, kTileWaves) * H > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "attn_bsr_bwd_bf16: %llu rows or %u keys x %u heads are more work units than one launch takes",
                    static_cast<unsigned long long>(rows), K, H);
    BwdCall c{};
    c.stream = as_stream(stream);
    c.H = H;
    c.rowPtrs = blockRowPtrs, c.colIdxs = blockColIdxs, c.tRowPtrs = tBlockRowPtrs, c.tColIdxs = tBlockColIdxs, c.perm = perm;
    c.Q = Q, c.K = Kmat, c.V = V, c.G = dO, c.O = out;
    c.lse = lse, c.mask = mask, c.delta = delta;
    c.dQ = dQ, c.dK = dK, c.dV = dV;
    BwdParams &p = c.p;
    p.Mb = numBlockRows, p.Kb = K / bS, p.D = D, p.Dv = Dv, p.rows = static_cast<uint32_t>(rows);
    p.ldq2 = ldq * 2u, p.ldk2 = ldk * 2u, p.ldv2 = ldv * 2u, p.ldg2 = ldg * 2u;
    p.q_bytes = static_cast<uint32_t>(qs), p.k_bytes = static_cast<uint32_t>(ks), p.v_bytes = static_cast<uint32_t>(vs);
    p.g_bytes = static_cast<uint32_t>(gs);
    p.ldo = ldo, p.lddq = lddq, p.lddk = lddk, p.lddv = lddv;
    p.out_bf16 = out_bf16 != 0, p.grads_bf16 = grads_bf16 != 0;
    p.want_dq = dQ != nullptr, p.want_dk = dK != nullptr, p.want_dv = dV != nullptr;
    p.scale = scale;
    p.q_head = q_head, p.k_head = k_head, p.v_head = v_head, p.g_head = g_head, p.o_head = o_head;
    p.dq_head = dq_head, p.dk_head = dk_head, p.dv_head = dv_head;
    const int ds = D <= 64 ? 2 : 4, dsv = Dv <= 64 ? 2 : 4;
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_const<2, 4>(ds, [&](auto d) {
            with_const<2, 4>(dsv, [&](auto dv) {
                with_flag(mask != nullptr, [&](auto mk) {
                    if (rows_pass) launch_rows<decltype(bs)::value, decltype(d)::value, decltype(dv)::value, decltype(mk)::value>(c);
                    if (cols_pass) launch_cols<decltype(bs)::value, decltype(d)::value, decltype(dv)::value, decltype(mk)::value>(c);
                });
            });
        });
    });
    char shape[48];
    snprintf(shape, sizeof(shape), "<b%u,%s,D%d,V%d>", bS, mask ? "mask" : "nomask", ds, dsv);
    if (rows_pass && cols_pass) note_kernel("attn_bsr_bwd_rows%s + attn_bsr_bwd_cols%s", shape, shape);
    else note_kernel("%s%s", rows_pass ? "attn_bsr_bwd_rows" : "attn_bsr_bwd_cols", shape);
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
