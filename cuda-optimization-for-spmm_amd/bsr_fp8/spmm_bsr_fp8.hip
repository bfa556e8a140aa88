// libmispmm_bsr_fp8.so: C = (A @ B) scaled per row and per column, A block-sparse (16 x 16 or 32 x 32 blocks) and B dense,
// both in OCP e4m3 bytes (torch.float8_e4m3fn), on v_mfma_f32_16x16x32_fp8_fp8 (include/mispmm_bsr_fp8.h).
//
// THE LANE LAYOUT.  Lane l = (c = l & 15, g = l >> 4).  One MFMA multiplies 16 rows x 32 k slots of A by 32 k slots x 16
// columns of B.  Lane (c, g) holds A[i = c][k = 8g .. 8g+7] as ONE 8-byte read, byte e of the 64-bit operand = k slot
// 8g + e, and B[k = 8g .. 8g+7][j = c] as one 64-bit operand in the same byte order; register r of a result tile is
// D[row 4g + r][col c].  tests/test_gpu_bsr_fp8.py proves this with one-hot operands, slot by slot.
// The 32 k slots of a step: the 16 + 16 columns of a pair of 16 x 16 blocks (lane groups 0, 1 the first block, 2, 3 the
// second; the missing half of an odd pair is zeros), or the 32 columns of one 32 x 32 block, whose two 16-row halves are two
// A operands against the same B operand.
//
// B ROWS.  A work item covers a super-tile of 16 * TPL output columns, interleaved as in csrc/bsr_mfma_tiles.hpp: tile t of
// lane column c is output column ncol + t, ncol = 16 * TPL * st + TPL * c.  For each of its 8 k rows the lane reads its TPL
// consecutive BYTES through a buffer descriptor of B's exact size: 8 bytes at TPL = 8 (the 16 lanes of a k row then read one
// 128-byte line), 16 at TPL = 16.  Dword w of a row holds the bytes of tiles 4w .. 4w+3, so the operand of a tile is a 4 x 4
// byte transpose over four k rows, twice (k rows 0-3 the low dword, 4-7 the high one): transpose4 below, two stages of
// v_perm_b32, in registers.  No LDS staging of B (DESIGN.md section 5.2 measured that route slower for bf16).  The missing
// half of an odd pair, and a lane whose columns lie at N or past it, take the dropped-load offset (spmm_common.hpp): zeros,
// nothing fetched.  All eight reads and the A reads are issued before the first v_perm (the sched_barrier behind them).
//
// WORK SPLIT.  One workgroup of 4 waves per (block row, super-tile); K step s goes to wave s % 4, which accumulates its
// steps in place in VGPRs (-mllvm -amdgpu-mfma-vgpr-form=true).  The four partial tiles are added through LDS in wave order,
// ((w0 + w1) + w2) + w3, the same bits run to run.  With an fp32 C wave q adds and stores rows 4q .. 4q+3 of each 16-row
// half (every wave parks the three row quads it does not own); with a bf16 C waves 1..3 park their tiles and wave 0 adds and
// stores all 16 rows -- the split csrc/bsr_slots.hpp measured faster for each C type.  A 32 x 32 block row goes through the
// same LDS twice, one 16-row half at a time.
//
// EPILOGUE.  rowScale and colScale are read once per owned row and column and applied as two separate fp32 multiplies
// (-ffp-contract=off), a NULL scale is no multiply; an empty block row is +0 whatever the scales.  The store is
// store_crow's: fp32 as 16-byte runs, bf16 packed by v_cvt_pk_bf16_f32.
// The unit lies outside csrc/: the census tests hold that directory and libmispmm.so to their records.
#include "mispmm_bsr_fp8.h"
#include "bsr_mfma_tiles.hpp"
#include "spmm_common.hpp"

namespace mispmm {

namespace {

// rows r0 .. r3 hold byte j = tile j; out[j] holds byte i = row i of tile j
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

// one B row: the lane's TPL interleaved byte columns at byte offset voff
template <int TPL>
__device__ __forceinline__ void load_brow8(rsrc_t rsrc, uint32_t voff, uint32_t (&row)[TPL / 4]) {
    if constexpr (TPL == 16) {
        const auto r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0);
#pragma unroll
        for (int w = 0; w < 4; ++w) row[w] = r[w];
    } else {
        const auto r = __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, 0, 0);
        row[0] = r[0];
        row[1] = r[1];
    }
}

// row r of the lane's TPL columns to C at element index row * ldc + ncol, as store_crow writes it
template <int TPL, bool C_BF16>
__device__ __forceinline__ void store_row(void *Cv, uint32_t row, uint32_t ldc, uint32_t ncol, const float (&v)[TPL]) {
    if constexpr (C_BF16) {
        uint16_t *dst = static_cast<uint16_t *>(Cv) + (static_cast<size_t>(row) * ldc + ncol);
#pragma unroll
        for (int w = 0; w < TPL / 8; ++w)
            *reinterpret_cast<u32x4_t *>(dst + 8 * w) = u32x4_t{pack_bf2(v[8 * w], v[8 * w + 1]), pack_bf2(v[8 * w + 2], v[8 * w + 3]),
                                                                pack_bf2(v[8 * w + 4], v[8 * w + 5]), pack_bf2(v[8 * w + 6], v[8 * w + 7])};
    } else {
        float *dst = static_cast<float *>(Cv) + (static_cast<size_t>(row) * ldc + ncol);
#pragma unroll
        for (int w = 0; w < TPL / 4; ++w) *reinterpret_cast<f32x4_t *>(dst + 4 * w) = f32x4_t{v[4 * w], v[4 * w + 1], v[4 * w + 2], v[4 * w + 3]};
    }
}

template <int BS, int TPL, bool C_BF16, bool SCALES>
__global__ __launch_bounds__(256) void bsr_mfma_fp8(uint32_t Mb, uint32_t nST, const uint32_t *__restrict__ blockRowPtrs,
                                                    const uint32_t *__restrict__ blockColIdxs, const uint8_t *__restrict__ blocks,
                                                    const uint8_t *__restrict__ B, uint32_t b_bytes, uint32_t N, uint32_t ldb,
                                                    const float *__restrict__ rowScale, const float *__restrict__ colScale,
                                                    void *__restrict__ Cv, uint32_t ldc, uint32_t xcd_chunk) {
    static_assert((BS == 16 || BS == 32) && (TPL == 8 || TPL == 16), "the instances of the header");
    constexpr int NA = BS / 16;        // A operands per step: the 16-row halves of a block
    constexpr bool SHARE = !C_BF16;    // the reduce and the store dealt over the four waves
    // one 16-row half at a time.  SHARE: [wave][quad slot 0..2][tile][lane column]; else [wave - 1][tile][lane]
    __shared__ f32x4_t parked[3 * TPL * 64];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t item = xcd_block(blockIdx.x, xcd_chunk);
    if (item >= Mb * nST) return;  // workgroup-uniform, before any barrier
    const uint32_t R = item / nST, st = item - R * nST;
    const uint32_t c = lane & 15, g = lane >> 4;
    const uint32_t ncol = st * (16 * TPL) + c * TPL;  // first of this lane's TPL interleaved output columns
    const rsrc_t rsrc = make_rsrc(B, b_bytes);
    const uint32_t lane_off = ncol < N ? ncol : kDropLoad;
    // this lane's 8 k slots: which block of the step, and which of its columns
    const uint32_t second = BS == 16 ? g >> 1 : 0u;
    const uint32_t kfirst = BS == 16 ? (g & 1) * 8u : g * 8u;

    f32x4_t acc[NA][TPL];
#pragma unroll
    for (int h = 0; h < NA; ++h)
#pragma unroll
        for (int t = 0; t < TPL; ++t) acc[h][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const uint32_t bs = blockRowPtrs[R], be = blockRowPtrs[R + 1];
    const uint32_t nsteps = BS == 16 ? (be - bs + 1) / 2 : be - bs;
    if (wave < nsteps) {
        const uint32_t last = be - 1;
        auto block_of = [&](uint32_t s) { return bs + (BS == 16 ? 2 * s + second : s); };
        uint32_t col_cur = blockColIdxs[min(block_of(wave), last)];
        for (uint32_t s = wave; s < nsteps; s += 4) {
            const uint32_t col_next = blockColIdxs[min(block_of(s + 4), last)];
            const uint32_t b = block_of(s);
            const bool have = b <= last;  // false for the missing half of an odd pair
            const uint8_t *ablk = blocks + static_cast<size_t>(min(b, last)) * (BS * BS) + c * BS + kfirst;
            u32x2_t araw[NA];
#pragma unroll
            for (int h = 0; h < NA; ++h) araw[h] = *reinterpret_cast<const u32x2_t *>(ablk + h * 16 * BS);
            // the block column differs between the two halves of the wave at BS = 16: the whole row offset is per lane
            const uint32_t voff = have ? lane_off + (col_cur * BS + kfirst) * ldb : kDropLoad;
            uint32_t braw[8][TPL / 4];
#pragma unroll
            for (int e = 0; e < 8; ++e) load_brow8<TPL>(rsrc, voff + e * ldb, braw[e]);
            // every read is on its way before the first v_perm: without this fence the regrouping is interleaved with the
            // loads and waits for them a few at a time
            __builtin_amdgcn_sched_barrier(0);
            long a[NA];
#pragma unroll
            for (int h = 0; h < NA; ++h) a[h] = __builtin_bit_cast(long, have ? araw[h] : u32x2_t{0u, 0u});
#pragma unroll
            for (int w = 0; w < TPL / 4; ++w) {
                uint32_t lo[4], hi[4];
                transpose4(braw[0][w], braw[1][w], braw[2][w], braw[3][w], lo);
                transpose4(braw[4][w], braw[5][w], braw[6][w], braw[7][w], hi);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const long bop = __builtin_bit_cast(long, u32x2_t{lo[j], hi[j]});
#pragma unroll
                    for (int h = 0; h < NA; ++h)
                        acc[h][4 * w + j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a[h], bop, acc[h][4 * w + j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            col_cur = col_next;
        }
    }

    // the scales of the rows and columns this lane stores, read once and ahead of the reduction (their latency passes behind
    // the barrier).  A scale that is NULL (or an empty block row) multiplies nothing: the selects in finish keep the sum's bits
    const bool scaled = SCALES && bs != be;  // an empty block row is +0 whatever the scales
    const bool by_row = scaled && rowScale, by_col = scaled && colScale;  // workgroup-uniform
    const uint32_t srow = R * BS + (SHARE ? wave : g) * 4u;  // the first row this lane stores of half 0
    float rs[NA][4] = {}, cs[TPL] = {};
    if constexpr (SCALES) {
        if (by_row) {
#pragma unroll
            for (int h = 0; h < NA; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) rs[h][r] = rowScale[srow + h * 16 + r];
        }
        if (by_col && ncol < N) {
#pragma unroll
            for (int t = 0; t < TPL; ++t) cs[t] = colScale[ncol + t];
        }
    }
    // rows 4g .. 4g+3 of half h, this lane's TPL columns, summed over the waves: scale, round, store
    auto finish = [&](int h, const f32x4_t (&sum)[TPL]) {
        const uint32_t row0 = srow + h * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v[TPL];
#pragma unroll
            for (int t = 0; t < TPL; ++t) {
                v[t] = sum[t][r];
                if constexpr (SCALES) {
                    const float byr = v[t] * rs[h][r];
                    v[t] = by_row ? byr : v[t];
                    const float byc = v[t] * cs[t];
                    v[t] = by_col ? byc : v[t];
                }
            }
            store_row<TPL, C_BF16>(Cv, row0 + r, ldc, ncol, v);
        }
    };

#pragma unroll
    for (int h = 0; h < NA; ++h) {
        if (h != 0) __syncthreads();  // the reads of the first half are done
        if constexpr (SHARE) {
            // lane (c, g) holds quad g, which wave g owns; quad slot = g with this wave's own quad left out
            if (g != wave) {
                f32x4_t *dst = parked + ((wave * 3u + (g - (g > wave ? 1u : 0u))) * TPL) * 16u + c;
#pragma unroll
                for (int t = 0; t < TPL; ++t) dst[t * 16] = acc[h][t];
            }
            __syncthreads();
            // one straight-line body per owner wave: the place of the wave's own tile in the sum is then a constant
            auto reduce_quad = [&](auto owner) {
                constexpr uint32_t Q = decltype(owner)::value;
                if (g != Q || ncol >= N) return;
                f32x4_t sum[TPL];
#pragma unroll
                for (int t = 0; t < TPL; ++t) {
                    f32x4_t p[4];
#pragma unroll
                    for (uint32_t w = 0; w < 4; ++w)
                        p[w] = w == Q ? acc[h][t] : parked[((w * 3u + (Q - (Q > w ? 1u : 0u))) * TPL + t) * 16u + c];
                    sum[t] = ((p[0] + p[1]) + p[2]) + p[3];
                    if (t % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // two tiles' reads in flight, not all: see below
                }
                finish(h, sum);
            };
            if (wave == 0) reduce_quad(std::integral_constant<uint32_t, 0>{});
            else if (wave == 1) reduce_quad(std::integral_constant<uint32_t, 1>{});
            else if (wave == 2) reduce_quad(std::integral_constant<uint32_t, 2>{});
            else reduce_quad(std::integral_constant<uint32_t, 3>{});
        } else {
            if (wave != 0) {
#pragma unroll
                for (int t = 0; t < TPL; ++t) parked[((wave - 1) * TPL + t) * 64u + lane] = acc[h][t];
            }
            __syncthreads();
            if (wave == 0 && ncol < N) {
                f32x4_t sum[TPL];
#pragma unroll
                for (int t = 0; t < TPL; ++t) {
                    sum[t] = acc[h][t];
#pragma unroll
                    for (uint32_t w = 0; w < 3; ++w) sum[t] += parked[(w * TPL + t) * 64u + lane];
                    // the reads of two tiles in flight at a time: left alone, the instances with scales issue all 3 * TPL
                    // reads ahead of the scale loads, 96 or 192 VGPRs that cost the main loop half its resident waves
                    if (t % 2 == 1) __builtin_amdgcn_sched_barrier(0);
                }
                finish(h, sum);
            }
        }
    }
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_bsr_fp8(mispmm_stream_t stream, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                              const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint8_t *blocks, const uint8_t *B, uint32_t N,
                              uint32_t ldb, const float *rowScale, const float *colScale, void *C, uint32_t ldc, int c_bf16) {
    constexpr const char *name = "bsr_fp8";
    if (!blockRowPtrs || !B || !C) return fail(MISPMM_ERR_INVALID_ARG, "%s: blockRowPtrs, B or C is null", name);
    if (numBlocks != 0 && (!blockColIdxs || !blocks)) return fail(MISPMM_ERR_INVALID_ARG, "%s: blockColIdxs or blocks is null", name);
    if (bS != 16 && bS != 32) return fail(MISPMM_ERR_UNSUPPORTED, "%s: only 16x16 or 32x32 blocks (got %ux%u)", name, bS, bS);
    if (N % 8 != 0 || ldb % 8 != 0 || ldc % 8 != 0)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: N, ldb and ldc must be multiples of 8 (N=%u ldb=%u ldc=%u)", name, N, ldb, ldc);
    if (ldb < N || ldc < N) return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than N (N=%u ldb=%u ldc=%u)", name, N, ldb, ldc);
    if (!aligned8(blocks) || !aligned8(B) || !aligned16(C) || (reinterpret_cast<uintptr_t>(rowScale) & 3u) || (reinterpret_cast<uintptr_t>(colScale) & 3u))
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: blocks and B must be 8-byte aligned, C 16-byte, the scales 4-byte", name);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    if (!fits_buffer(K, ldb, 1)) return fail(MISPMM_ERR_UNSUPPORTED, "%s: B spans 2 GiB or more (K=%u ldb=%u)", name, K, ldb);
    if (numBlockRows == 0 || N == 0) return MISPMM_OK;
    // 16 tiles per lane (256-column super-tiles, 16-byte B reads) once N fills one and 16-byte reads line up; else 8 tiles
    // (128 columns, 8-byte reads).  All four (bS, TPL) forms are free of scratch
    const bool wide = N >= 256 && N % 16 == 0 && ldb % 16 == 0 && aligned16(B);
    const uint32_t nST = ceil_div(N, wide ? 256u : 128u);
    if (static_cast<uint64_t>(numBlockRows) * nST > 0x7FFFFFFFull)   // one workgroup per (block row, super-tile)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: %u block rows x %u columns exceed the grid of this kernel", name, numBlockRows, N);
    const XcdGrid xg = xcd_grid(numBlockRows * nST);
    // B's exact extent: the gap columns of its last row are not part of it
    const uint32_t b_bytes = K == 0 ? 0u : static_cast<uint32_t>(static_cast<uint64_t>(K - 1) * ldb + N);
    const bool scales = rowScale || colScale;
    note_kernel("bsr_mfma_fp8<b%u,T%d,%s,%s>", bS, wide ? 16 : 8, c_bf16 ? "c16" : "c32", scales ? "scales" : "plain");
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_const<16, 8>(wide ? 16 : 8, [&](auto tpl) {
            with_flag(c_bf16 != 0, [&](auto cb) {
                with_flag(scales, [&](auto sc) {
                    hipLaunchKernelGGL((bsr_mfma_fp8<decltype(bs)::value, decltype(tpl)::value, decltype(cb)::value, decltype(sc)::value>), dim3(xg.grid),
                                       dim3(256), 0, as_stream(stream), numBlockRows, nST, blockRowPtrs, blockColIdxs, blocks, B, b_bytes, N, ldb, rowScale,
                                       colScale, C, ldc, xg.chunk);
                });
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
