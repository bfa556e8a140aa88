// SDDMM on a BSR pattern in bf16: out[e][i][j] = <X[R * bS + i, :], Y[c * bS + j, :]> for every stored block e of block row R
// with block column c = blockColIdxs[e] (A's values are not read).  The backward of C = A * B with respect to A's blocks is
// this product with X = dC, Y = B.
//
// Arithmetic: v_mfma_f32_16x16x32_bf16, one instruction per 16 x 16 output tile and 32 columns of N, columns ascending, fp32
// accumulation.  The instruction's operand maps (lane l: A[row l & 15][k = 8 (l >> 4) + 0..7], B[k = 8 (l >> 4) + 0..7][col l & 15])
// are both "row l & 15 of a row-major operand, 8 consecutive columns": a fragment is one 16-byte row read per lane, no permute,
// no LDS.  Y is the A operand and X the B operand, so the result tile arrives TRANSPOSED -- D[row = j][col = i], lane l holds
// i = l & 15 and j = 4 (l >> 4) + 0..3 in its four accumulator registers -- which are four CONSECUTIVE elements of a row of the
// out block: a lane stores one 16-byte (bf16 out: 8-byte) vector and a wave instruction one whole 16 x 16 tile.  (With X as the
// A operand a register would scatter over four rows.)  The sums are the same either way: the products commute and the
// order over n is the instruction's.
// Shape: one workgroup of 4 waves per block row, the row's blocks dealt to the waves in turn; a 32 x 32 block is 2 x 2 tiles
// of one wave.  N <= 32 * NS (NS = 4, and 8 with 16-byte lanes): the wave's X fragments stay in registers for the whole row and
// the Y fragments of its next block are fetched before the products of the current one.  Wider N: a chunk loop of 32 * NS
// columns that re-reads X (from L1 / L2: the four waves share it).  A wave without a block leaves at once; nothing crosses
// waves: no LDS, no barrier.
// Loads go through buffer descriptors: a column at or past N and a block column at or past K / bS become the dropped-load
// offset (spmm_common.hpp), so they read zeros and fetch nothing.  Fixed order: run to run identical.
#include "spmm_common.hpp"

namespace mispmm {

namespace {

using bf16x8_t = short __attribute__((ext_vector_type(8)));
using sbf32x4_t = float __attribute__((ext_vector_type(4)));
// `out` is only as aligned as its element type: global vector stores take any address
using out_f32x4_t = float __attribute__((ext_vector_type(4), aligned(4)));
using out_u16x4_t = uint16_t __attribute__((ext_vector_type(4), aligned(2)));

constexpr int kSbWaves = 4;

// 8 consecutive bf16 of one row: columns col .. col + 7 at byte offset row_off (kDropLoad: no such row) + 2 col.  WIDE: N is a
// multiple of 8, so the 8 columns are inside N or past it together.  Narrow: element by element, any N and any alignment.
// Neither offset sum can wrap: row_off + 2 col stays below 2^31 for a row in range, and kDropLoad + 2 col keeps bit 31.
template <bool WIDE>
__device__ __forceinline__ bf16x8_t load_frag(rsrc_t rsrc, uint32_t row_off, uint32_t col, uint32_t N) {
    if constexpr (WIDE) {
        const uint32_t off = col < N ? row_off + col * 2u : kDropLoad;
        return __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
    } else {
        bf16x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t off = col + j < N ? row_off + (col + j) * 2u : kDropLoad;
            v[j] = static_cast<short>(__builtin_amdgcn_raw_buffer_load_b16(rsrc, off, 0, 0));
        }
        return v;
    }
}

// BS: block size (16, 32).  NS: 32-column steps held at once.  HOLD: N <= 32 * NS, X read once per wave; else the chunk loop.
template <int BS, bool WIDE, bool OUT_BF16, int NS, bool HOLD>
__global__ void __launch_bounds__(64 * kSbWaves) sddmm_bsr_kernel(uint32_t Mb, uint32_t Kb, uint32_t N, uint32_t xcd_chunk, uint32_t ldx2,
                                                                  uint32_t ldy2, const uint32_t *__restrict__ blockRowPtrs,
                                                                  const uint32_t *__restrict__ blockColIdxs,
                                                                  const uint16_t *__restrict__ X, uint32_t x_bytes,
                                                                  const uint16_t *__restrict__ Y, uint32_t y_bytes, void *__restrict__ outv) {
    constexpr int T = BS / 16;  // tiles per block side
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t R = xcd_block(blockIdx.x, xcd_chunk);
    if (R >= Mb) return;
    const uint32_t bs = blockRowPtrs[R], be = blockRowPtrs[R + 1];
    if (be <= bs || be - bs <= wave) return;  // an empty block row, or fewer blocks than waves
    const uint32_t r = lane & 15, g = lane >> 4;
    const uint32_t kcol = g * 8u;  // the lane's 8 columns of a 32-column step
    const rsrc_t xr = make_rsrc(X, x_bytes), yr = make_rsrc(Y, y_bytes);

    uint32_t xrow[T];  // < 2 GiB: the host declines anything larger
#pragma unroll
    for (int t = 0; t < T; ++t) xrow[t] = (R * BS + t * 16u + r) * ldx2;

    struct Frags {
        bf16x8_t f[NS][T];
    };
    auto load_x = [&](uint32_t n0, Frags &x) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int t = 0; t < T; ++t) x.f[s][t] = load_frag<WIDE>(xr, xrow[t], n0 + s * 32u + kcol, N);
    };
    // a block column at or past K / bS names no row of Y: zeros, nothing fetched
    auto load_y = [&](uint32_t c, uint32_t n0, Frags &y) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t yrow = c < Kb ? (c * BS + t * 16u + r) * ldy2 : kDropLoad;
#pragma unroll
            for (int s = 0; s < NS; ++s) y.f[s][t] = load_frag<WIDE>(yr, yrow, n0 + s * 32u + kcol, N);
        }
    };
    sbf32x4_t acc[T][T];
    auto clear = [&] {
#pragma unroll
        for (int ti = 0; ti < T; ++ti)
#pragma unroll
            for (int tj = 0; tj < T; ++tj) acc[ti][tj] = sbf32x4_t{0.f, 0.f, 0.f, 0.f};
    };
    auto multiply = [&](const Frags &x, const Frags &y) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int ti = 0; ti < T; ++ti)
#pragma unroll
                for (int tj = 0; tj < T; ++tj)
                    acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y.f[s][tj], x.f[s][ti], acc[ti][tj], 0, 0, 0);
    };
    // lane (r, g) holds out[e][ti * 16 + r][tj * 16 + 4 g + 0..3]
    auto store = [&](uint32_t e) {
        // Hazard: the result registers of an MFMA may not be read by a VALU or memory instruction until the instruction has
        // gone through its passes -- the ISA's XDL-write to VALU-read rule asks for the pass count plus 3 wait states, 11 for
        // this 8-pass shape and 19 at most for any shape -- and the hardware does not interlock it.  hipcc pads the hazard
        // inside a basic block (the HOLD bodies: `s_nop` ahead of the store) but not on the edge out of the chunk loop, where
        // the first accumulator read of the store directly follows the loop's last MFMA.  So the chunk loop spells the wait
        // out, 32 idle cycles per tile, with the accumulators passing through the statement so that every read follows it.
        if constexpr (!HOLD) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ti = 0; ti < T; ++ti)
#pragma unroll
                for (int tj = 0; tj < T; ++tj) asm volatile("s_nop 15\n\ts_nop 15" : "+a"(acc[ti][tj]));
            __builtin_amdgcn_sched_barrier(0);
        }
        const size_t base = static_cast<size_t>(e) * (BS * BS);
#pragma unroll
        for (int ti = 0; ti < T; ++ti)
#pragma unroll
            for (int tj = 0; tj < T; ++tj) {
                const size_t at = base + (ti * 16u + r) * BS + tj * 16u + g * 4u;
                const sbf32x4_t v = acc[ti][tj];
                if constexpr (OUT_BF16) {
                    out_u16x4_t o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = __builtin_bit_cast(uint16_t, static_cast<__bf16>(v[k]));  // v_cvt_pk_bf16_f32, as mispmm_f32_to_bf16: RNE, a NaN stays a NaN
                    *reinterpret_cast<out_u16x4_t *>(static_cast<uint16_t *>(outv) + at) = o;
                } else {
                    *reinterpret_cast<out_f32x4_t *>(static_cast<float *>(outv) + at) = out_f32x4_t{v[0], v[1], v[2], v[3]};
                }
            }
    };

    if constexpr (HOLD) {
        // two fragment sets in turn (a copy `cur = nxt` would wait for the loads it is meant to hide); the block column of
        // a fetch is itself read one block ahead.  Past the row's end: an out-of-range block column, so the loads are dropped.
        auto col_of = [&](uint32_t e) { return e < be ? blockColIdxs[e] : 0xFFFFFFFFu; };
        Frags x, y0, y1;
        uint32_t e = bs + wave;
        load_x(0, x);
        load_y(blockColIdxs[e], 0, y0);
        uint32_t c1 = col_of(e + kSbWaves);
        for (;;) {
            const uint32_t c2 = col_of(e + 2 * kSbWaves);
            load_y(c1, 0, y1);
            clear();
            multiply(x, y0);
            store(e);
            e += kSbWaves;
            if (e >= be) break;
            c1 = col_of(e + 2 * kSbWaves);
            load_y(c2, 0, y0);
            clear();
            multiply(x, y1);
            store(e);
            e += kSbWaves;
            if (e >= be) break;
        }
    } else {
        for (uint32_t e = bs + wave; e < be; e += kSbWaves) {
            const uint32_t c = blockColIdxs[e];
            clear();
            for (uint32_t n0 = 0; n0 < N; n0 += 32u * NS) {
                Frags x, y;
                load_x(n0, x);
                load_y(c, n0, y);
                multiply(x, y);
            }
            store(e);
        }
    }
}

struct SbArgs {
    hipStream_t stream;
    uint32_t Mb, Kb, N;
    const uint32_t *blockRowPtrs, *blockColIdxs;
    const uint16_t *X;
    uint32_t ldx;
    const uint16_t *Y;
    uint32_t ldy;
    void *out;
};

template <int BS, bool WIDE, bool OUT_BF16, int NS, bool HOLD>
void launch_sddmm_bsr(const SbArgs &a) {
    const XcdGrid xg = xcd_grid(a.Mb);
    note_kernel("sddmm_bsr<b%d,%s,%s,%s%d>", BS, WIDE ? "wide" : "narrow", OUT_BF16 ? "bf16" : "f32", HOLD ? "hold" : "loop", NS);
    hipLaunchKernelGGL((sddmm_bsr_kernel<BS, WIDE, OUT_BF16, NS, HOLD>), dim3(xg.grid), dim3(64 * kSbWaves), 0, a.stream, a.Mb, a.Kb, a.N,
                       xg.chunk, a.ldx * 2u, a.ldy * 2u, a.blockRowPtrs, a.blockColIdxs, a.X,
                       static_cast<uint32_t>(static_cast<uint64_t>(a.Mb) * BS * a.ldx * 2u), a.Y,
                       static_cast<uint32_t>(static_cast<uint64_t>(a.Kb) * BS * a.ldy * 2u), a.out);
}

template <int BS, bool WIDE, bool OUT_BF16>
void launch_sddmm_bsr_width(const SbArgs &a) {
    if (a.N <= 128) return launch_sddmm_bsr<BS, WIDE, OUT_BF16, 4, true>(a);
    if constexpr (WIDE) {
        if (a.N <= 256) return launch_sddmm_bsr<BS, WIDE, OUT_BF16, 8, true>(a);
        launch_sddmm_bsr<BS, WIDE, OUT_BF16, 8, false>(a);
    } else {
        // an element-wise fragment passes through 8 registers before it is packed into 4: half the steps at once
        launch_sddmm_bsr<BS, WIDE, OUT_BF16, 4, false>(a);
    }
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_sddmm_bsr_bf16(mispmm_stream_t stream, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                                     const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint16_t *X, uint32_t ldx,
                                     const uint16_t *Y, uint32_t ldy, uint32_t N, void *out, int out_bf16) {
    if (bS != 16 && bS != 32) return fail(MISPMM_ERR_UNSUPPORTED, "sddmm_bsr_bf16: only 16x16 or 32x32 blocks (got bS=%u)", bS);
    if (numBlockRows == 0 || numBlocks == 0) return MISPMM_OK;
    if (!blockRowPtrs || !blockColIdxs || !out) return fail(MISPMM_ERR_INVALID_ARG, "sddmm_bsr_bf16: blockRowPtrs, blockColIdxs or out is null");
    if (ldx < N || ldy < N)
        return fail(MISPMM_ERR_INVALID_ARG, "sddmm_bsr_bf16: leading dimension smaller than N (N=%u ldx=%u ldy=%u)", N, ldx, ldy);
    if (K % bS != 0) return fail(MISPMM_ERR_INVALID_ARG, "sddmm_bsr_bf16: K=%u is not a multiple of the block size %u", K, bS);
    if (N == 0) {  // empty sums: +0
        note_kernel("sddmm_bsr<zero>");
        MISPMM_HIP_TRY(hipMemsetAsync(out, 0, static_cast<size_t>(numBlocks) * bS * bS * (out_bf16 ? 2u : 4u), as_stream(stream)));
        return MISPMM_OK;
    }
    if (!X || !Y) return fail(MISPMM_ERR_INVALID_ARG, "sddmm_bsr_bf16: X or Y is null");
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    const auto spans_2gib = [](uint64_t rows, uint32_t ld) { return ld != 0 && rows > 0x3FFFFFFFull / ld; };  // rows * ld * 2 bytes
    if (spans_2gib(static_cast<uint64_t>(numBlockRows) * bS, ldx) || spans_2gib(K, ldy))
        return fail(MISPMM_ERR_UNSUPPORTED, "sddmm_bsr_bf16: X or Y spans 2 GiB or more (rows=%llu ldx=%u K=%u ldy=%u)",
                    static_cast<unsigned long long>(numBlockRows) * bS, ldx, K, ldy);
    const SbArgs a{as_stream(stream), numBlockRows, K / bS, N, blockRowPtrs, blockColIdxs, X, ldx, Y, ldy, out};
    const bool wide = N % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && aligned16(X) && aligned16(Y);
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_flag(wide, [&](auto w) {
            with_flag(out_bf16 != 0, [&](auto o) { launch_sddmm_bsr_width<decltype(bs)::value, decltype(w)::value, decltype(o)::value>(a); });
        });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
