// The element policy of the fused attention on a CSR pattern: what differs between operands in fp32 and operands in bf16,
// written once for the kernels of attn_csr_fwd.hpp and attn_csr_bwd.hpp and the four libraries built from them.
// A policy gives, for a lane width VEC:
//   kBytes, kWide        bytes per element; the wide lane width (16 bytes of a row: 4 or 8 columns); the other width is 1
//   in_t, out_t          what a pointer to an operand and to a result points at (a bf16 result is fp32 or bf16: void)
//   raw_t<VEC>           a lane's slice of a row as it is loaded
//   load<VEC>            ... through a raw buffer descriptor; the dropped-load mark gives zeros
//   at<VEC>(raw, i)      column i of the slice as a float: vec_get, or the exact widening
//   kWidens, held_t,     the slice of the group's OWN row as it is kept over the whole walk: the loaded vector, or (kWidens)
//   held(x, i)           VEC floats widened once, which the kernel fills from at(); column i of either
//   lane_off<G, VEC>     byte offset of the lane's columns of chunk c, or the dropped-load mark past the width
//   gather<VEC, NCH>     the lane's slices of a batch's 8 x NCH rows of one operand
//   row_t, row_of, ptr   where row `row` of head h of a result begins (head stride and ld in elements) and a pointer into it: a
//                        float pointer formed once per row, or an element index that meets the base at the store, where the
//                        result's type (fp32 or bf16) is known
//   fits<G, VEC, NCH>    the instances the static_asserts allow;  with_instance: the one list of those that exist
// Beside the policies: store_f32 / store_bf16 (a lane's VEC results as fp32, or rounded once through bf16_pair), the backward's
// weight(), and for the entry points aligned2 and Extent / extent / meet (the overlap check, element size as an argument).
// They take and return values: that kind leaves the kernels' ISA alone (lane_group.hpp's header, DESIGN.md section 9
// items 17, 18 and 22).  bf16: element 2i of a dword is its low half, 2i + 1 its high half, each widened by moving its bits to
// the upper half of an fp32 (exact, nothing flushed or quieted); V8 is 8 consecutive columns as one 16-byte buffer load (the
// register cost of an fp32 V4 slice), V1 one buffer_load_ushort per column.
#pragma once
#include "bf16_lanes.hpp"
#include "lane_group.hpp"

namespace mispmm {

namespace {

// one rounding to nearest even, a NaN stays a NaN: v_cvt_pk_bf16_f32, as rows_bf16/ and mispmm_f32_to_bf16
__device__ __forceinline__ uint32_t bf16_bits(float x) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(x)); }
__device__ __forceinline__ uint32_t bf16_pair(float lo, float hi) { return bf16_bits(lo) | (bf16_bits(hi) << 16); }

// the lane's VEC results to the lane's columns of a row of an fp32 result ...
template <int VEC>
__device__ __forceinline__ void store_f32(float *to, const float *r) {
    if constexpr (VEC == 8) {
        store_vec<4>(to, f32x4{r[0], r[1], r[2], r[3]});
        store_vec<4>(to + 4, f32x4{r[4], r[5], r[6], r[7]});
    } else {
        typename VecOf<VEC>::type x;
#pragma unroll
        for (int v = 0; v < VEC; ++v) vec_set<VEC>(x, v, r[v]);
        store_vec<VEC>(to, x);
    }
}
// ... or of a bf16 one: the same values rounded once
template <int VEC>
__device__ __forceinline__ void store_bf16(uint16_t *to, const float *r) {
    if constexpr (VEC == 1) *to = static_cast<uint16_t>(bf16_bits(r[0]));
    else *reinterpret_cast<u32x4 *>(to) = u32x4{bf16_pair(r[0], r[1]), bf16_pair(r[2], r[3]), bf16_pair(r[4], r[5]), bf16_pair(r[6], r[7])};
}

// what both policies spell alike, over the policy's own kBytes, raw_t and load
template <class Elem>
struct ElemCommon {
    // byte offset of the lane's columns of chunk c in a row of `width` columns; past the width: the dropped-load mark
    template <int G, int VEC>
    static __device__ __forceinline__ uint32_t lane_off(uint32_t lane, int c, uint32_t width) {
        const uint32_t col = c * (G * VEC) + lane * VEC;
        return col < width ? col * Elem::kBytes : kDropLoad;
    }

    // the lane's slices of the batch's 8 rows of one operand; key: byte offset of the row of entry `sub`, or the mark
    template <int VEC, int NCH, class Raw>
    static __device__ __forceinline__ void gather(uint32_t key, rsrc_t r, const uint32_t (&off)[NCH], Raw (&rows)[kLgBatch][NCH]) {
        static_for<0, kLgBatch>([&](auto j_tag) {
            constexpr int j = decltype(j_tag)::value;
            const uint32_t kj = group_bcast<8, j>(key);
#pragma unroll
            for (int c = 0; c < NCH; ++c) rows[j][c] = Elem::template load<VEC>(r, join_off(kj, off[c]));
        });
    }

    // f(G, VEC, NCH) as constants -- lanes of a row, elements of a lane, chunks of G * VEC columns: the one list of the
    // instances that exist.  Wide lanes: 64 x 4 or 32 x 8 covers 256; element lanes: a whole wave takes 1, 2 or 4 chunks
    template <class F>
    static void with_instance(int vec, int g, uint32_t width, F &&f) {
        using std::integral_constant;
        using wide = integral_constant<int, Elem::kWide>;
        if (vec == Elem::kWide) {
            if constexpr (Elem::kWide == 4) with_group(g, [&](auto gr) { f(gr, wide{}, integral_constant<int, 1>{}); });
            else with_const<8, 16, 32>(g, [&](auto gr) { f(gr, wide{}, integral_constant<int, 1>{}); });
        } else if (!try_const<8, 16, 32>(g, [&](auto gr) { f(gr, integral_constant<int, 1>{}, integral_constant<int, 1>{}); })) {
            const uint32_t chunks = ceil_div(width, static_cast<uint32_t>(kWave));
            with_const<1, 2, 4>(chunks <= 1 ? 1 : chunks == 2 ? 2 : 4,
                                [&](auto ch) { f(integral_constant<int, 64>{}, integral_constant<int, 1>{}, ch); });
        }
    }
};

struct ElemF32 : ElemCommon<ElemF32> {
    using in_t = float;
    using out_t = float;
    static constexpr uint32_t kBytes = 4;
    static constexpr int kWide = 4;
    static constexpr bool kWidens = false;
    template <int VEC> using raw_t = typename VecOf<VEC>::type;
    template <int VEC> using held_t = raw_t<VEC>;
    using row_t = float *;

    template <int VEC>
    static __device__ __forceinline__ raw_t<VEC> load(rsrc_t r, uint32_t off) { return buffer_load_vec<VEC>(r, off, 0); }
    template <int VEC>
    static __device__ __forceinline__ float at(const raw_t<VEC> &raw, int i) { return vec_get<VEC>(raw, i); }
    template <int VEC>
    static __device__ __forceinline__ float held(const held_t<VEC> &x, int i) { return vec_get<VEC>(x, i); }

    static __device__ __forceinline__ row_t row_of(float *out, uint32_t h, uint64_t head, uint32_t row, uint32_t ld) {
        return out + static_cast<size_t>(h) * head + static_cast<size_t>(row) * ld;
    }
    template <class T>
    static __device__ __forceinline__ T *ptr(float *, row_t at) { return reinterpret_cast<T *>(at); }  // T is float wherever this runs

    // more than one chunk only where a whole wave owns the row
    template <int G, int VEC, int NCH>
    static constexpr bool fits = (VEC == 4 || VEC == 1) && (NCH == 1 || G == kWave);
};

struct ElemBf16 : ElemCommon<ElemBf16> {
    using in_t = uint16_t;
    using out_t = void;
    static constexpr uint32_t kBytes = 2;
    static constexpr int kWide = 8;
    static constexpr bool kWidens = true;
    template <int VEC> using raw_t = typename RawOf<VEC>::type;
    template <int VEC> using held_t = float[VEC];
    using row_t = size_t;

    template <int VEC>
    static __device__ __forceinline__ raw_t<VEC> load(rsrc_t r, uint32_t off) { return buffer_load_bf16<VEC>(r, off); }
    // element i widened to fp32 exactly: the bits moved to the upper half
    template <int VEC>
    static __device__ __forceinline__ float at(const raw_t<VEC> &raw, int i) { return widen<VEC>(raw, i); }
    template <int VEC>
    static __device__ __forceinline__ float held(const held_t<VEC> &h, int i) { return h[i]; }
    static __device__ __forceinline__ row_t row_of(void *, uint32_t h, uint64_t head, uint32_t row, uint32_t ld) {
        return static_cast<size_t>(h) * head + static_cast<size_t>(row) * ld;
    }
    template <class T>
    static __device__ __forceinline__ T *ptr(void *out, row_t at) { return static_cast<T *>(out) + at; }

    // 16-byte lanes or element lanes, there is no 8-byte form; more than one chunk only where a whole wave of element lanes
    // owns the row
    template <int G, int VEC, int NCH>
    static constexpr bool fits = (VEC == 8 || VEC == 1) && (NCH == 1 || (G == kWave && VEC == 1));
};

// P of one entry of the backward: exp(z - lse) with one rounding of the difference; a row whose lse is not finite is NaN
// throughout, as a softmax over a +Inf, a NaN or nothing but -Inf is (z - (+Inf) alone would give +0)
__device__ __forceinline__ float weight(float z, float lse) {
    return __builtin_fabsf(lse) < __builtin_huge_valf() ? lg_exp(z - lse) : __builtin_nanf("");
}

inline bool aligned2(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 1u) == 0; }

struct Extent {
    const char *lo, *hi;
};
// bytes H heads of an operand of `elem`-byte elements cover (a head stride of 0: one head's); strides and span in elements
inline Extent extent(const void *base, uint32_t H, uint64_t head_stride, uint64_t head_span, uint64_t elem) {
    const char *lo = static_cast<const char *>(base);
    return {lo, base && head_span ? lo + ((H - 1) * head_stride + head_span) * elem : lo};
}
inline bool meet(const Extent &x, const Extent &y) { return x.lo < y.hi && y.lo < x.hi; }

}  // namespace

}  // namespace mispmm
