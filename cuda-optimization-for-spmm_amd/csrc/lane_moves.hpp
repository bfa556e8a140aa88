// Cross-lane moves inside a lane group of a wave, shared by the kernels that reduce over a row's lanes (sddmm.hip,
// softmax_csr.hip).  A move reads only lanes of the reader's own group of MASK * 2 lanes, so a group whose lanes branch
// together never reads a lane that has left.
#pragma once
#include "spmm_common.hpp"

namespace mispmm {

// the value lane ^ MASK holds.  1, 2: quad_perm [1,0,3,2] / [2,3,0,1]; 8: row_ror:8 (a rotation by half a 16-lane row is the
// exchange of its halves); 4, 16: ds_swizzle bit mode (and 0x1f, or 0, xor MASK; inside 32 lanes); 32: ds_bpermute.
template <int MASK>
__device__ __forceinline__ uint32_t lane_xor_u32(uint32_t x) {
    const int v = static_cast<int>(x);
    if constexpr (MASK == 1) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true));
    else if constexpr (MASK == 2) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true));
    else if constexpr (MASK == 8) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, true));
    else if constexpr (MASK == 4 || MASK == 16) return static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(v, (MASK << 10) | 0x1F));
    else return static_cast<uint32_t>(__shfl_xor(v, MASK, kWave));
}
template <int MASK> __device__ __forceinline__ float lane_xor(float x) { return __uint_as_float(lane_xor_u32<MASK>(__float_as_uint(x))); }
template <int MASK> __device__ __forceinline__ double lane_xor(double x) {
    using u2 = uint32_t __attribute__((ext_vector_type(2)));
    u2 b = __builtin_bit_cast(u2, x);
    b[0] = lane_xor_u32<MASK>(b[0]);
    b[1] = lane_xor_u32<MASK>(b[1]);
    return __builtin_bit_cast(double, b);
}

// f over the values of all G lanes of a group, in every lane of it: a butterfly of log2(G) moves.  f must be commutative
// to the bit (fp add and max are), so both partners of a step hold the same value and the order is fixed.
template <int G, class A, class F>
__device__ __forceinline__ A group_all_reduce(A v, F f) {
    static_assert(G >= 1 && (G & (G - 1)) == 0 && G <= kWave, "a group is a power of two of lanes inside a wave");
    if constexpr (G >= 2) v = f(v, lane_xor<1>(v));
    if constexpr (G >= 4) v = f(v, lane_xor<2>(v));
    if constexpr (G >= 8) v = f(v, lane_xor<4>(v));
    if constexpr (G >= 16) v = f(v, lane_xor<8>(v));
    if constexpr (G >= 32) v = f(v, lane_xor<16>(v));
    if constexpr (G >= 64) v = f(v, lane_xor<32>(v));
    return v;
}

}  // namespace mispmm
