// libmispmm_bsrc_fp8.so: C = (A @ B) scaled per row and per column, A column-compacted in 16-row strips and fixed step
// slots, A's values and B in OCP e4m3 bytes, on v_mfma_f32_16x16x32_fp8_fp8 (include/mispmm_bsrc_fp8.h): the layout and the
// work split of bsrc_slots_mfma_bf16 (csrc/bsr_slots.hpp) with the operands of bsr_mfma_fp8
// (bsr_fp8/spmm_bsr_fp8.hip).  The fp8 instruction's K step is 32 slots = one [16][32] tile of the layout: ONE instruction per
// tile and step where the bf16 kernel issues two.
//
// THE LANE LAYOUT is bsr_mfma_fp8's.  Lane l = (c = l & 15, g = l >> 4) holds A[i = c][k = 8g .. 8g+7] as ONE 8-byte read of
// tiles[s][c][8g ..], byte e of the 64-bit operand = k slot 8g + e, and B[k = 8g .. 8g+7][j = c] in the same byte order;
// register r of a result tile is D[row 4g + r][col c].
//
// COLUMN LIST.  The step index is wave-uniform, so its 32 column indices come through the scalar cache (two s_load_dwordx16)
// and lane group g takes indices 8g .. 8g+7 by and/or with four masks: no branch, no vector load in front of the B reads.
//
// B ROWS.  A work item covers 128 output columns; tile t of lane column c is output column ncol + t, ncol = 128 st + 8c.  For
// each of its 8 gathered rows the lane reads its 8 consecutive BYTES through a buffer descriptor of B's exact size: eight
// different rows, 16 VGPRs in flight where the bf16 kernel holds 32.  A padding index (0xFFFFFFFF) takes the dropped-load
// offset as the WHOLE offset, a lane at or past N as its column part (K * ldb < 2^31, so the sum keeps bit 31): zeros, nothing
// fetched.  All eight reads and the A read are issued before the first v_perm_b32 (the sched_barrier behind them); then two
// 4 x 4 byte transposes per dword column (transpose4) make the operands of tiles 4w .. 4w+3, and each tile is ONE MFMA into a
// fresh accumulator (addend 0): no accumulator is live while the reads are in flight.
//
// REDUCE AND STORE are bsr_slots.hpp's: waves 1..3 park their tile in LDS (24 KiB), extra steps go to waves 1..3, which add
// them into their parked tile, and wave 0 adds the three parked tiles in wave order and stores 16 rows (`w0`); or, where C is
// fp32 and no strip has extra steps, every wave parks the three row quads it does not own and wave q adds and stores rows
// 4q .. 4q+3 (`share`).  The scales of the rows and columns a lane stores are read before the barrier and applied behind the
// sum as two separate multiplies (-ffp-contract=off); the stores are non-temporal.
// The unit lies outside csrc/ and bsr_fp8/: the census tests hold those directories and their libraries to their records.
#include <algorithm>
#include <vector>

#include "mispmm_bsrc_fp8.h"
#include "bsr_mfma_tiles.hpp"
#include "spmm_common.hpp"

namespace mispmm {

namespace {

constexpr uint32_t kSlots = 4;            // fixed step slots per strip = waves per workgroup
constexpr uint32_t kPad = 0xFFFFFFFFu;    // a padding column index

// rows r0 .. r3 hold byte j = tile j; out[j] holds byte i = row i of tile j (as bsr_fp8/spmm_bsr_fp8.hip)
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

template <bool C_BF16, bool SCALES, bool SHARE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 8))) void bsrc_slots_mfma_fp8(
    uint32_t Ms, uint32_t nST, const uint32_t *__restrict__ extraPtrs, const uint32_t *__restrict__ cols, const uint8_t *__restrict__ tiles,
    const uint8_t *__restrict__ B, uint32_t b_bytes, uint32_t N, uint32_t ldb, const float *__restrict__ rowScale,
    const float *__restrict__ colScale, void *__restrict__ Cv, uint32_t ldc, uint32_t xcd_chunk) {
    static_assert(!(SHARE && C_BF16), "the shared reduce is the fp32 C's (bsr_slots.hpp measured it slower with a bf16 C)");
    constexpr int TPL = 8;
    // [wave - 1][row of the strip][128 columns], or with SHARE [wave][quad slot 0..2][row of the quad][128 columns]: 24 KiB
    __shared__ float parked[kSlots - 1][16][128];

    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t item = xcd_block(blockIdx.x, xcd_chunk);
    if (item >= Ms * nST) return;  // workgroup-uniform, before any barrier
    const uint32_t R = item / nST, st = item - R * nST;
    const uint32_t c = lane & 15, g = lane >> 4;
    const uint32_t ncol = st * (16 * TPL) + c * TPL;  // first of this lane's 8 output columns
    const rsrc_t rsrc = make_rsrc(B, b_bytes);
    const uint32_t lane_off = ncol < N ? ncol : kDropLoad;

    // this lane's 8 B-row indices of step s: lane group g multiplies k = 8g .. 8g+7
    struct Idx {
        uint32_t v[8];
    };
    auto load_idx = [&](uint32_t s, Idx &ix) {
        using u32x16_t = uint32_t __attribute__((ext_vector_type(16)));
        const u32x16_t *p = reinterpret_cast<const u32x16_t *>(cols + static_cast<size_t>(__builtin_amdgcn_readfirstlane(s)) * 32u);
        const u32x16_t lo = p[0], hi = p[1];  // whole-vector loads, then a branch-free deal
        const uint32_t m0 = g == 0 ? ~0u : 0u, m1 = g == 1 ? ~0u : 0u, m2 = g == 2 ? ~0u : 0u, m3 = g == 3 ? ~0u : 0u;
#pragma unroll
        for (int e = 0; e < 8; ++e) ix.v[e] = (lo[e] & m0) | (lo[8 + e] & m1) | (hi[e] & m2) | (hi[8 + e] & m3);
        return lo[0];
    };
    // one MFMA K step (32 occupied columns) into fresh accumulators
    auto step_tile = [&](uint32_t s, const Idx &ix, f32x4_t (&t)[TPL]) {
        u32x2_t braw[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t col = ix.v[e];
            braw[e] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, col == kPad ? kDropLoad : col * ldb + lane_off, 0, 0);
        }
        const u32x2_t araw = *reinterpret_cast<const u32x2_t *>(tiles + static_cast<size_t>(s) * 512u + c * 32u + g * 8u);
        // all nine reads are on their way before the first v_perm
        __builtin_amdgcn_sched_barrier(0);
        const long a = __builtin_bit_cast(long, araw);
        const f32x4_t zero{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            uint32_t lo[4], hi[4];
            transpose4(braw[0][w], braw[1][w], braw[2][w], braw[3][w], lo);
            transpose4(braw[4][w], braw[5][w], braw[6][w], braw[7][w], hi);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                t[4 * w + j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, __builtin_bit_cast(long, u32x2_t{lo[j], hi[j]}), zero, 0, 0, 0);
        }
    };

    // hop 1: this wave's slot (column list) and the extent of the strip's extra steps
    Idx ix;
    // a slot past the strip's step count is all padding; a used slot starts with a real column (padding only ever trails)
    const uint32_t first = load_idx(R * kSlots + wave, ix);
    auto slot_tile = [&](f32x4_t (&t)[TPL]) {
        if (first != kPad) {
            step_tile(R * kSlots + wave, ix, t);  // hop 2
        } else {
#pragma unroll
            for (int i = 0; i < TPL; ++i) t[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
    };

    // the scales of the rows and columns this lane stores, read ahead of the barrier.  A NULL scale or an empty strip (slot 0
    // is all padding) multiplies nothing: the selects in store_row keep the sum's bits
    const uint32_t srow = R * 16u + (SHARE ? wave : g) * 4u;  // the first row this lane stores
    bool by_row = false, by_col = false;                      // workgroup-uniform
    float rs[4] = {}, cs[TPL] = {};
    if constexpr (SCALES) {
        const bool scaled = cols[static_cast<size_t>(R) * (kSlots * 32u)] != kPad;
        by_row = scaled && rowScale;
        by_col = scaled && colScale;
        if (by_row && (SHARE || wave == 0)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) rs[r] = rowScale[srow + r];
        }
        if (by_col && ncol < N && (SHARE || wave == 0)) {
#pragma unroll
            for (int t = 0; t < TPL; ++t) cs[t] = colScale[ncol + t];
        }
    }
    // one row of the result, r = 0 .. 3 of the lane's rows: scale, round, store this lane's 8 columns
    auto store_row = [&](int r, f32x4_t s0, f32x4_t s1) {
        if constexpr (SCALES) {
            const f32x4_t r0 = s0 * rs[r], r1 = s1 * rs[r];
            s0 = by_row ? r0 : s0;
            s1 = by_row ? r1 : s1;
            const f32x4_t c0 = s0 * f32x4_t{cs[0], cs[1], cs[2], cs[3]}, c1 = s1 * f32x4_t{cs[4], cs[5], cs[6], cs[7]};
            s0 = by_col ? c0 : s0;
            s1 = by_col ? c1 : s1;
        }
        const size_t crow = static_cast<size_t>(srow + r) * ldc + ncol;
        if constexpr (C_BF16) {
            const u32x4_t o{pack_bf2(s0[0], s0[1]), pack_bf2(s0[2], s0[3]), pack_bf2(s1[0], s1[1]), pack_bf2(s1[2], s1[3])};
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4_t *>(static_cast<uint16_t *>(Cv) + crow));
        } else {
            float *dst = static_cast<float *>(Cv) + crow;
            __builtin_nontemporal_store(s0, reinterpret_cast<f32x4_t *>(dst));
            __builtin_nontemporal_store(s1, reinterpret_cast<f32x4_t *>(dst + 4));
        }
    };

    if constexpr (SHARE) {
        f32x4_t t[TPL];
        slot_tile(t);  // zeros for an unused slot: parked like any other
        float *quads = &parked[0][0][0];
        if (g != wave) {
            // lane (c, g) holds rows 4g .. 4g+3 = quad g, which wave g owns; quad slot = g with this wave's own quad left out
            float *dst = quads + ((wave * (kSlots - 1) + (g - (g > wave ? 1u : 0u))) * 4u) * 128u + c * 8u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                *reinterpret_cast<f32x4_t *>(dst + r * 128) = f32x4_t{t[0][r], t[1][r], t[2][r], t[3][r]};
                *reinterpret_cast<f32x4_t *>(dst + r * 128 + 4) = f32x4_t{t[4][r], t[5][r], t[6][r], t[7][r]};
            }
        }
        __syncthreads();
        // one straight-line body per owner wave: the place of the wave's own tile in the sum is then a constant
        auto reduce_quad = [&](auto owner) {
            constexpr uint32_t Q = decltype(owner)::value;
            if (g != Q || ncol >= N) return;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                f32x4_t p0[kSlots], p1[kSlots];
#pragma unroll
                for (uint32_t w = 0; w < kSlots; ++w) {
                    if (w == Q) {
                        p0[w] = f32x4_t{t[0][r], t[1][r], t[2][r], t[3][r]};
                        p1[w] = f32x4_t{t[4][r], t[5][r], t[6][r], t[7][r]};
                    } else {
                        const float *src = quads + ((w * (kSlots - 1) + (Q - (Q > w ? 1u : 0u))) * 4u + r) * 128u + c * 8u;
                        p0[w] = *reinterpret_cast<const f32x4_t *>(src);
                        p1[w] = *reinterpret_cast<const f32x4_t *>(src + 4);
                    }
                }
                store_row(r, ((p0[0] + p0[1]) + p0[2]) + p0[3], ((p1[0] + p1[1]) + p1[2]) + p1[3]);
            }
        };
        if (wave == 0) reduce_quad(std::integral_constant<uint32_t, 0>{});
        else if (wave == 1) reduce_quad(std::integral_constant<uint32_t, 1>{});
        else if (wave == 2) reduce_quad(std::integral_constant<uint32_t, 2>{});
        else reduce_quad(std::integral_constant<uint32_t, 3>{});
    } else if (wave != 0) {
        const uint32_t ex0 = extraPtrs[R], ex1 = extraPtrs[R + 1];
        {
            f32x4_t t[TPL];
            slot_tile(t);
            // park the tile: lane (c, g) holds rows 4g .. 4g+3, columns 8c .. 8c+7
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float *dst = &parked[wave - 1][g * 4 + r][c * 8];
                *reinterpret_cast<f32x4_t *>(dst) = f32x4_t{t[0][r], t[1][r], t[2][r], t[3][r]};
                *reinterpret_cast<f32x4_t *>(dst + 4) = f32x4_t{t[4][r], t[5][r], t[6][r], t[7][r]};
            }
        }
        // strips of more than 4 steps (more than 128 occupied columns): extra step i goes to wave 1 + i % 3
        for (uint32_t e = ex0 + (wave - 1); e < ex1; e += kSlots - 1) {
            const uint32_t s = Ms * kSlots + e;
            load_idx(s, ix);
            f32x4_t t[TPL];
            step_tile(s, ix, t);
            // the parked tile lives in LDS between two extra steps, not in 32 registers across the B reads; a lane re-reads
            // exactly the words it wrote, so this needs no barrier
            asm volatile("" ::: "memory");
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float *dst = &parked[wave - 1][g * 4 + r][c * 8];
                f32x4_t a = *reinterpret_cast<f32x4_t *>(dst), b = *reinterpret_cast<f32x4_t *>(dst + 4);
                a += f32x4_t{t[0][r], t[1][r], t[2][r], t[3][r]};
                b += f32x4_t{t[4][r], t[5][r], t[6][r], t[7][r]};
                *reinterpret_cast<f32x4_t *>(dst) = a;
                *reinterpret_cast<f32x4_t *>(dst + 4) = b;
            }
            asm volatile("" ::: "memory");
        }
        __syncthreads();
    } else {
        f32x4_t acc[TPL];
        slot_tile(acc);
        __syncthreads();
        if (ncol < N) {
            // wave 0 adds the parked tiles in wave order and stores the strip's 16 x 128 result
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                f32x4_t s0{acc[0][r], acc[1][r], acc[2][r], acc[3][r]}, s1{acc[4][r], acc[5][r], acc[6][r], acc[7][r]};
#pragma unroll
                for (uint32_t p = 0; p < kSlots - 1; ++p) {
                    s0 += *reinterpret_cast<const f32x4_t *>(&parked[p][g * 4 + r][c * 8]);
                    s1 += *reinterpret_cast<const f32x4_t *>(&parked[p][g * 4 + r][c * 8 + 4]);
                }
                store_row(r, s0, s1);
            }
        }
    }
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_bsr_compact_slots_fp8_host(uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                                                 const uint32_t *blockRowPtrs_host, const uint32_t *blockColIdxs_host, const uint8_t *blocks_host,
                                                 uint32_t *nSteps_out, uint32_t *nUsedSteps_out, uint32_t *extraPtrs_out_host,
                                                 uint32_t *cols_out_host, uint8_t *tiles_out_host) {
    constexpr const char *name = "bsr compact slots fp8";
    if (!nSteps_out) return fail(MISPMM_ERR_INVALID_ARG, "%s: nSteps_out is null", name);
    if (bS != 16 && bS != 32) return fail(MISPMM_ERR_UNSUPPORTED, "%s: only 16x16 or 32x32 blocks (got %ux%u)", name, bS, bS);
    const bool fill = extraPtrs_out_host && cols_out_host && tiles_out_host;
    if (!fill && (extraPtrs_out_host || cols_out_host || tiles_out_host))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: give all three outputs or none (size query)", name);
    const uint64_t M = static_cast<uint64_t>(numBlockRows) * bS;
    if (M > 0xFFFFFFFFull) return fail(MISPMM_ERR_UNSUPPORTED, "%s: %u block rows of %u exceed 2^32 - 1 rows", name, numBlockRows, bS);
    if (int st = mispmm_bsr_check_host(static_cast<uint32_t>(M), K, bS, bS, numBlocks, blockRowPtrs_host, static_cast<uint64_t>(numBlockRows) + 1,
                                       blockColIdxs_host, numBlocks, static_cast<uint64_t>(numBlocks) * bS * bS))
        return st;
    if (numBlocks != 0 && !blocks_host) return fail(MISPMM_ERR_INVALID_ARG, "%s: blocks is null", name);
    const uint32_t halves = bS / 16;
    const uint64_t strips = static_cast<uint64_t>(numBlockRows) * halves, fixed = strips * kSlots;
    uint64_t extra = 0, used = 0;
    struct Col {
        uint32_t col, block, j;
    };
    std::vector<Col> occ;
    for (uint64_t R = 0; R < strips; ++R) {
        const uint32_t br = static_cast<uint32_t>(R / halves), h = static_cast<uint32_t>(R % halves);
        // the strip's occupied columns: some row holds a byte that is not +-0 (a NaN byte is occupied)
        occ.clear();
        for (uint32_t b = blockRowPtrs_host[br]; b < blockRowPtrs_host[br + 1]; ++b) {
            const uint8_t *rows = blocks_host + (static_cast<size_t>(b) * bS + h * 16u) * bS;
            for (uint32_t j = 0; j < bS; ++j) {
                bool any = false;
                for (uint32_t i = 0; i < 16 && !any; ++i) any = (rows[static_cast<size_t>(i) * bS + j] & 0x7Fu) != 0;
                if (any) occ.push_back(Col{blockColIdxs_host[b] * bS + j, b, j});
            }
        }
        // ascending; a block column stored twice keeps its storage order
        std::stable_sort(occ.begin(), occ.end(), [](const Col &x, const Col &y) { return x.col < y.col; });
        const uint32_t nsteps = static_cast<uint32_t>((occ.size() + 31) / 32);
        if (fill) {
            extraPtrs_out_host[R] = static_cast<uint32_t>(extra);
            for (uint32_t s = 0; s < std::max(nsteps, kSlots); ++s) {
                const uint64_t at = s < kSlots ? R * kSlots + s : fixed + extra + (s - kSlots);
                uint32_t *cdst = cols_out_host + at * 32;
                uint8_t *tdst = tiles_out_host + at * 512;
                for (uint32_t k = 0; k < 32; ++k) {
                    const size_t e = static_cast<size_t>(s) * 32 + k;
                    const bool live = e < occ.size();
                    cdst[k] = live ? occ[e].col : kPad;
                    const uint8_t *src = live ? blocks_host + (static_cast<size_t>(occ[e].block) * bS + h * 16u) * bS + occ[e].j : nullptr;
                    for (uint32_t i = 0; i < 16; ++i) tdst[i * 32 + k] = live ? src[static_cast<size_t>(i) * bS] : 0;
                }
            }
        }
        used += nsteps;
        if (nsteps > kSlots) extra += nsteps - kSlots;
    }
    if (fixed + extra > 0x03FFFFFFull) return fail(MISPMM_ERR_UNSUPPORTED, "%s: too many K steps", name);
    if (fill) extraPtrs_out_host[strips] = static_cast<uint32_t>(extra);
    *nSteps_out = static_cast<uint32_t>(fixed + extra);
    if (nUsedSteps_out) *nUsedSteps_out = static_cast<uint32_t>(used);
    return MISPMM_OK;
}

extern "C" int mispmm_bsrc_slots_fp8(mispmm_stream_t stream, uint32_t numStrips, uint32_t K, uint32_t nSteps, const uint32_t *extraPtrs,
                                     const uint32_t *cols, const uint8_t *tiles, const uint8_t *B, uint32_t N, uint32_t ldb, const float *rowScale,
                                     const float *colScale, void *C, uint32_t ldc, int c_bf16) {
    constexpr const char *name = "bsrc_slots_fp8";
    auto off4 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (!extraPtrs || !cols || !tiles || !B || !C) return fail(MISPMM_ERR_INVALID_ARG, "%s: null pointer", name);
    if (N % 8 != 0 || ldb % 8 != 0 || ldc % 8 != 0)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: N, ldb and ldc must be multiples of 8 (N=%u ldb=%u ldc=%u)", name, N, ldb, ldc);
    if (ldb < N || ldc < N) return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than N (N=%u ldb=%u ldc=%u)", name, N, ldb, ldc);
    if (!aligned8(tiles) || !aligned8(B) || !aligned16(C) || off4(extraPtrs) || off4(cols) || off4(rowScale) || off4(colScale))
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: tiles and B must be 8-byte aligned, C 16-byte, extraPtrs, cols and the scales 4-byte", name);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    if (!fits_buffer(K, ldb, 1)) return fail(MISPMM_ERR_UNSUPPORTED, "%s: B spans 2 GiB or more (K=%u ldb=%u)", name, K, ldb);
    const uint32_t nST = ceil_div(N, 128u);
    // the kernel indexes rows and work items with 32 bits: one workgroup per (strip, 128 columns)
    if (numStrips > 0x0FFFFFFFu || static_cast<uint64_t>(numStrips) * nST > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: %u strips x %u columns exceed the grid of this kernel", name, numStrips, N);
    const uint64_t slot_steps = static_cast<uint64_t>(numStrips) * kSlots;
    if (nSteps < slot_steps) return fail(MISPMM_ERR_INVALID_ARG, "%s: nSteps %u is less than %u slots per strip", name, nSteps, kSlots);
    if (numStrips == 0 || N == 0) return MISPMM_OK;
    const XcdGrid xg = xcd_grid(numStrips * nST);
    // B's exact extent: the gap columns of its last row are not part of it
    const uint32_t b_bytes = K == 0 ? 0u : static_cast<uint32_t>(static_cast<uint64_t>(K - 1) * ldb + N);
    const bool scales = rowScale || colScale;
    // nSteps == 4 * numStrips leaves no room for extra steps: by the layout's contract extraPtrs then describes none, and the
    // shared reduce does not read it.  With a bf16 C wave 0 reduces: what csrc/bsr_slots.hpp measured for either C type
    const bool share = nSteps == slot_steps && !c_bf16;
    note_kernel("bsrc_slots_mfma_fp8<T8,%s,%s,%s>", c_bf16 ? "c16" : "c32", scales ? "scales" : "plain", share ? "share" : "w0");
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(xg.grid), dim3(256), 0, as_stream(stream), numStrips, nST, extraPtrs, cols, tiles, B, b_bytes, N, ldb, rowScale,
                           colScale, C, ldc, xg.chunk);
    };
    with_flag(scales, [&](auto sc) {
        constexpr bool SC = decltype(sc)::value;
        if (c_bf16) launch(bsrc_slots_mfma_fp8<true, SC, false>);
        else if (share) launch(bsrc_slots_mfma_fp8<false, SC, true>);
        else launch(bsrc_slots_mfma_fp8<false, SC, false>);
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
