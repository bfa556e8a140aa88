// The tile pieces of the bf16 block-sparse products on v_mfma_f32_16x16x32_bf16, written once for the register-staged
// kernels of spmm_bsr.hip (bsr_mfma_bf16, bsrc_mfma_bf16, bsr_mfma_bf16_b32), bsrc_slots_mfma_bf16 (bsr_slots.hpp) and, for
// the vector types alone, bsr_bf16_lds (bsr_bf16_lds.hpp).  No kernel and no tag stands here.
//
// THE LANE LAYOUT.  Lane l = (c = l & 15, g = l >> 4).  One MFMA multiplies 16 rows x 32 k slots of A by 32 k slots x 16
// columns of B: lane (c, g) holds A[i = c][k = 8g .. 8g+7] (one 16-byte read, `araw`) and B[k = 8g .. 8g+7][j = c];
// register r of a result tile is D[row 4g + r][col c].  Which B rows the 32 k slots are is the kernel's business (the 16 + 16
// columns of a block pair, the 32 columns of a 32 x 32 block, 32 occupied columns of a compacted block row).
// A work item covers a super-tile of 16 * TPL output columns, interleaved over TPL accumulator tiles: tile t of lane column
// c is output column ncol + t, ncol = 16 * TPL * st + TPL * c.  So for each of its 8 k rows the lane reads the TPL
// CONSECUTIVE bf16 of columns ncol .. ncol + TPL - 1 (load_brow: 16 bytes at TPL = 8, 8 at TPL = 4), regroups the 8 rows per
// tile with v_perm_b32 (regroup_pair: the transpose B needs, done in registers), and writes row 4g + r of the result as
// one run of TPL consecutive elements (store_crow).
//
// DROPPED LOADS.  B is read through a buffer descriptor of its exact size.  The lane's share of every offset is
// lane_off = ncol * 2, or kDropLoad for ncol >= N (N is a multiple of TPL where these kernels run, so a lane's columns are
// inside N or past it together); a B row that is not there -- the missing half of an odd block pair, a block past the row's
// end, a padding column 0xFFFFFFFF -- takes kDropLoad as the WHOLE offset.  Either way the read returns zeros and fetches
// nothing; the coefficients that meet them are zero as well.  The row offset is per lane and rides in voffset with soffset
// 0: a non-uniform soffset costs a waterfall loop.
//
// The SHAPE of each helper is the one that leaves the ISA of the kernels as it was; what
// could not be shared under that rule -- the cross-wave reduction, the work-item prologue -- is described there and
// spelled in the kernels.
#pragma once
#include "spmm_common.hpp"

namespace mispmm {

using f32x4_t = float __attribute__((ext_vector_type(4)));
using bf16x8_t = short __attribute__((ext_vector_type(8)));
using u32x2_t = uint32_t __attribute__((ext_vector_type(2)));
using u32x4_t = uint32_t __attribute__((ext_vector_type(4)));

// what a lane holds of one MFMA K step: NA A operands (two for the 16-row halves of a 32 x 32 block) and its 8 B rows
template <int TPL, int NA = 1>
struct Frag {
    u32x4_t araw[NA];
    uint32_t braw[8][TPL / 2];
};

// one B row: the lane's TPL interleaved bf16 columns at byte offset voff
template <int TPL>
__device__ __forceinline__ void load_brow(rsrc_t rsrc, uint32_t voff, uint32_t (&row)[TPL / 2]) {
    if constexpr (TPL == 8) {
        const auto r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0);
#pragma unroll
        for (int w = 0; w < 4; ++w) row[w] = r[w];
    } else {
        const auto r = __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, 0, 0);
        row[0] = r[0];
        row[1] = r[1];
    }
}

// the B operands of tiles 2w and 2w+1: the low and high bf16 of dword w of every k row.  Once both are packed the eight raw
// dwords are dead, so the regrouped operands never coexist with more than one dword column
template <int TPL>
__device__ __forceinline__ void regroup_pair(const uint32_t (&braw)[8][TPL / 2], int w, u32x4_t &even, u32x4_t &odd) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t lo = braw[2 * p][w], hi = braw[2 * p + 1][w];
        even[p] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);  // {hi.h0, lo.h0}
        odd[p] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);   // {hi.h1, lo.h1}
    }
}

// two fp32 to one dword of bf16 (v_cvt_pk_bf16_f32: RNE, a NaN stays a NaN), `lo` in the low half
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
    using bf2 = __bf16 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(lo), static_cast<__bf16>(hi)});
}

// row r of the lane's TPL tiles to C at element index crow: fp32 as 16-byte runs, or bf16 by v_cvt_pk_bf16_f32 in one store
template <int TPL, bool C_BF16>
__device__ __forceinline__ void store_crow(void *Cv, uint32_t row, uint32_t ldc, uint32_t ncol, const f32x4_t (&acc)[TPL], int r) {
    if constexpr (C_BF16) {
        uint32_t o[TPL / 2];
#pragma unroll
        for (int w = 0; w < TPL / 2; ++w) o[w] = pack_bf2(acc[2 * w][r], acc[2 * w + 1][r]);
        uint16_t *dst = static_cast<uint16_t *>(Cv) + (static_cast<size_t>(row) * ldc + ncol);
        if constexpr (TPL == 8) *reinterpret_cast<u32x4_t *>(dst) = u32x4_t{o[0], o[1], o[2], o[3]};
        else *reinterpret_cast<u32x2_t *>(dst) = u32x2_t{o[0], o[1]};
    } else {
        float *dst = static_cast<float *>(Cv) + (static_cast<size_t>(row) * ldc + ncol);
#pragma unroll
        for (int w = 0; w < TPL / 4; ++w)
            *reinterpret_cast<f32x4_t *>(dst + 4 * w) = f32x4_t{acc[4 * w][r], acc[4 * w + 1][r], acc[4 * w + 2][r], acc[4 * w + 3][r]};
    }
}

}  // namespace mispmm
