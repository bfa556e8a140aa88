// A lane's slice of a bf16 row as raw bits: how it is loaded and how one element is taken out of it.  Shared by the units that
// read bf16 operands themselves (rows_bf16/spmm_rows_bf16.hip, sddmm_bf16/sddmm_csr_bf16.hip, ElemBf16 of attn_csr/elem.hpp).
#pragma once
#include "spmm_common.hpp"

namespace mispmm {

namespace {

using u32x2 = uint32_t __attribute__((ext_vector_type(2)));
using u32x4 = uint32_t __attribute__((ext_vector_type(4)));

// V bf16 elements as they are loaded: element 2i in the low half of dword i, element 2i + 1 in the high half
template <int V> struct RawOf;
template <> struct RawOf<1> { using type = uint32_t; };
template <> struct RawOf<4> { using type = u32x2; };
template <> struct RawOf<8> { using type = u32x4; };

template <int V>
__device__ __forceinline__ typename RawOf<V>::type buffer_load_bf16(rsrc_t rsrc, uint32_t voffset) {
    if constexpr (V == 1) return __builtin_amdgcn_raw_buffer_load_b16(rsrc, voffset, 0, 0);
    else if constexpr (V == 4) return __builtin_amdgcn_raw_buffer_load_b64(rsrc, voffset, 0, 0);
    else return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, 0, 0);
}

// element i widened to fp32 exactly: the bits moved to the upper half, nothing flushed or quieted
template <int V>
__device__ __forceinline__ float widen(const typename RawOf<V>::type &raw, int i) {
    if constexpr (V == 1) return __uint_as_float(raw << 16);
    else return __uint_as_float((i & 1) ? (raw[i >> 1] & 0xFFFF0000u) : (raw[i >> 1] << 16));
}

}  // namespace

}  // namespace mispmm
