// The tile pieces of fused bf16 attention on a BSR block pattern, written once for the forward (attn_bsr.hip) and the two
// passes of the backward (bwd/attn_bsr_bwd.hip).  No kernel and no tag stands here: each unit keeps its parameter block, its
// kernels, its launchers and its entry point, and walks its stages its own way.
//
// THE WORK UNIT.  One WAVE owns 16 rows of one head -- query rows in the forward and in the backward's row pass, keys in its
// column pass: a block row (column) at bS = 16, half of one at bS = 32 -- and walks it 32 rows of the other side at a step:
// two blocks at bS = 16 (an odd leftover is a half step), one block at bS = 32 (Walk<BS>).  kTileWaves waves to a
// workgroup, consecutive units of one head; nothing crosses waves: no LDS, no barrier, no atomics.  Every kernel decodes its
// unit the same way at its top: xcd_block() of the workgroup, then the head h, then the unit (both early returns: a
// workgroup, a wave past the end), then the block row R and the 16-row part `sub` of it, then the lane as i = l & 15,
// g = l >> 4; finish_grid() fills what that reads.
//
// THE TRANSPOSED PRODUCTS.  Every product is computed transposed, so that what belongs to one of the wave's 16 rows stays
// in one lane.  A score product takes the step's rows (K rows in the forward) as the A operand and the wave's own rows (Q
// rows; their fragments stay in registers for the whole walk, load_frag) as the B operand: lane (i, g) holds row i of the
// wave x rows 4g .. 4g + 3 of each of the step's two 16-row tiles.  An accumulating product acc^T += X^T * W^T (O^T += V^T P^T,
// dQ^T += K^T dS^T, ...) takes W^T as the B operand: lane (i, g) supplies W[i][its 8 k slots].  k is only a summation index,
// so slot 8g + j is NAMED row 4g + j of the first tile and slot 8g + 4 + j row 4g + j of the second: the 8 weights a lane
// already holds, no lane move.  The A operand is X^T in the V LAYOUT (TRows): the lane reads, for the same 8 rows, the TPL
// consecutive bf16 of columns TPL * i .. and regroups them per tile with v_perm_b32, exactly as bsr_mfma_bf16 (spmm_bsr.hip)
// does for its B.  Lane (i, g) then holds acc[i][4 TPL g .. 4 TPL g + 4 TPL - 1]: whatever scales row i is lane-local and the
// final store is a run of consecutive elements of the row (store_tiles).
//
// MFMA HAZARD.  An accumulator that an MFMA wrote and VALU reads over a loop edge -- the forward's rescale in the next
// iteration, every kernel's store after the loop -- is not covered by the wait hipcc pads inside a block (the `store`
// comment of sddmm_bsr.hip).  settle() spells the XDL-write to VALU-read wait out for all tiles together: 16 idle cycles,
// the accumulators passing through the statement so that every read follows it.
//
// LOADS go through buffer descriptors (one per operand and head).  The lane's share of a load's offset does not change
// along the walk: `row * ld2 + col * 2` with row i and columns 32 s + 8 g .. for a fragment, row 4g + j and columns TPL * i ..
// in the V layout, or the dropped-load mark kDropLoad for columns at or past the width.  The tile's first row comes as the
// wave-uniform scalar offset.  A tile that is not there -- a block at or past the operand's end, the missing half of a half
// step, a step past the walk's end -- takes the mark as the whole vector offset and a scalar offset of 0 (two marks added
// would wrap): zeros, nothing fetched.
//
// The SHAPE of each helper is the one that leaves the ISA of all 64 kernel instances as it was (DESIGN.md section 9 item
// 25): a helper that takes a whole array the kernel also writes elsewhere, or that forms an address from kernel arguments,
// moved instructions; so the forward calls the per-run, per-slot and per-pair helpers from its own loops and lambdas,
// and the unit decode and the lane offsets above are described here and spelled in the kernels.
#pragma once
#include "lane_moves.hpp"

namespace mispmm {

namespace {

using bf16x8_t = short __attribute__((ext_vector_type(8)));
using f32x4_t = float __attribute__((ext_vector_type(4)));
using u32x2_t = uint32_t __attribute__((ext_vector_type(2)));
using u32x4_t = uint32_t __attribute__((ext_vector_type(4)));
using bf2 = __bf16 __attribute__((ext_vector_type(2)));

constexpr int kTileWaves = 4;  // waves to a workgroup, in every kernel of both units

__device__ __forceinline__ float tile_exp(float t) { return __builtin_amdgcn_exp2f(t * 1.44269504088896340736f); }  // as softmax_bsr.hip

// what follows from the block size BS
template <int BS>
struct Walk {
    static constexpr uint32_t T = BS / 16;                    // work units per block row
    static constexpr uint32_t EPS = BS == 16 ? 2 : 1;         // blocks per 32-row step
    static constexpr uint32_t kSecond = BS == 32 ? 16u : 0u;  // first row of a step's second tile inside its block
};

// 8 consecutive bf16 of one of the wave's own rows; the 8 columns are inside N or past it together (N is a multiple of 8)
__device__ __forceinline__ bf16x8_t load_frag(rsrc_t rsrc, uint32_t row_off, uint32_t col, uint32_t N) {
    const uint32_t off = col < N ? row_off + col * 2u : kDropLoad;
    return __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
}

// the accumulators, settled: every read after this statement follows the MFMAs that wrote them by 16 cycles
template <int TPL>
__device__ __forceinline__ void settle(f32x4_t (&acc)[TPL]) {
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (TPL == 8)
        asm volatile("s_nop 15" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7]));
    else
        asm volatile("s_nop 15" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
    __builtin_amdgcn_sched_barrier(0);
}

// lane (i, g) holds X[row][TPL (4g + k) + t] in acc[t][k]: for every k a run of TPL consecutive columns, inside `width` or
// past it together (a multiple of 8).  Stored times inv: fp32, or bf16 by v_cvt_pk_bf16_f32 (as mispmm_f32_to_bf16: RNE, a
// NaN stays a NaN).
template <int TPL>
__device__ __forceinline__ void store_run(const f32x4_t (&acc)[TPL], int k, float inv, void *out, size_t base, uint32_t col, bool as_bf16) {
    float v[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) v[t] = acc[t][k] * inv;
    if (as_bf16) {
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
        for (int w = 0; w < TPL / 4; ++w) *reinterpret_cast<f32x4_t *>(dst + 4 * w) = f32x4_t{v[4 * w], v[4 * w + 1], v[4 * w + 2], v[4 * w + 3]};
    }
}
template <int TPL>
__device__ __forceinline__ void store_tiles(const f32x4_t (&acc)[TPL], void *out, size_t base, uint32_t g, uint32_t width, float inv,
                                            bool as_bf16) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t col = TPL * (4u * g + k);
        if (col < width) store_run<TPL>(acc, k, inv, out, base, col, as_bf16);
    }
}

// the lane's rows of an operand in the V layout: slot j < 4 row 4g + j of the step's first 16-row tile, slot 4 + j the same
// row of the second; of each the TPL consecutive bf16 from column TPL * i.  off: the lane's four V-layout offsets; va / vb: the tile is there
// (wave-uniform); sa / sb: the tile's first row times the row stride
template <int TPL>
struct TRows {
    uint32_t v[8][TPL / 2];
};
template <int TPL>
__device__ __forceinline__ void load_trow(TRows<TPL> &t, int j, rsrc_t rsrc, uint32_t vo, uint32_t so) {
    if constexpr (TPL == 8) {
        const auto r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo, so, 0);
#pragma unroll
        for (int w = 0; w < 4; ++w) t.v[j][w] = r[w];
    } else {
        const auto r = __builtin_amdgcn_raw_buffer_load_b64(rsrc, vo, so, 0);
        t.v[j][0] = r[0];
        t.v[j][1] = r[1];
    }
}
template <int TPL>
__device__ __forceinline__ void load_trows(TRows<TPL> &t, rsrc_t rsrc, const uint32_t (&off)[4], bool va, bool vb, uint32_t sa, uint32_t sb) {
#pragma unroll
    for (int j = 0; j < 8; ++j) load_trow<TPL>(t, j, rsrc, (j < 4 ? va : vb) ? off[j & 3] : kDropLoad, j < 4 ? sa : sb);
}
// acc^T += X^T * W^T: tiles 2w and 2w + 1 take the low and high bf16 of dword w of every row's columns
template <int TPL>
__device__ __forceinline__ void mfma_trow_pair(f32x4_t &a0, f32x4_t &a1, const TRows<TPL> &t, int w, bf16x8_t w8) {
    u32x4_t even, odd;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t lo = t.v[2 * q][w], hi = t.v[2 * q + 1][w];
        even[q] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);  // {hi.h0, lo.h0}
        odd[q] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);   // {hi.h1, lo.h1}
    }
    a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, even), w8, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, odd), w8, a1, 0, 0, 0);
}
template <int TPL>
__device__ __forceinline__ void mfma_trows(f32x4_t (&acc)[TPL], const TRows<TPL> &t, bf16x8_t w8) {
#pragma unroll
    for (int w = 0; w < TPL / 2; ++w) mfma_trow_pair<TPL>(acc[2 * w], acc[2 * w + 1], t, w, w8);
}

// z = fl32(scale * s + mask) of one score, one fma; no mask: the product (as softmax_bsr.hip).  m[j]: the score's mask element
template <bool MASK, class M>
__device__ __forceinline__ float scaled(float scale, float s, const M &m, int j) {
    if constexpr (MASK) return __builtin_fmaf(scale, s, m[j]);
    else return scale * s;
}

// elements one head's rows span: the last row ends with its last column, not with its stride
uint64_t span(uint64_t rows, uint32_t ld, uint32_t width) { return rows == 0 ? 0 : (rows - 1) * ld + width; }

// what both entry points refuse first, in this order; fn: the entry point's name as its messages begin
int refuse_shape(const char *fn, uint32_t bS, float scale, uint32_t D, uint32_t Dv, uint32_t K) {
    if (bS != 16 && bS != 32) return fail(MISPMM_ERR_UNSUPPORTED, "%s: only 16x16 or 32x32 blocks (got bS=%u)", fn, bS);
    if (!(scale > 0.f) || scale == __builtin_huge_valf())
        return fail(MISPMM_ERR_INVALID_ARG, "%s: scale must be finite and > 0 (got %g)", fn, static_cast<double>(scale));
    if (D == 0 || Dv == 0 || D % 8 != 0 || Dv % 8 != 0 || D > 128 || Dv > 128)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: D and Dv must be multiples of 8 from 8 to 128 (got D=%u Dv=%u)", fn, D, Dv);
    if (K % bS != 0) return fail(MISPMM_ERR_INVALID_ARG, "%s: K=%u is not a multiple of the block size %u", fn, K, bS);
    return MISPMM_OK;
}

// a launch over `units` work units of each of H heads: fills what the kernels' unit decode reads and returns the workgroups to launch
template <class P>
uint32_t finish_grid(P &p, uint32_t units, uint32_t H) {
    p.units = units;
    p.wgs_per_head = ceil_div(units, kTileWaves);
    p.total = p.wgs_per_head * H;
    const XcdGrid xg = xcd_grid(p.total);
    p.xcd_chunk = xg.chunk;
    return xg.grid;
}

}  // namespace

}  // namespace mispmm
