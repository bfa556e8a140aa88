// libmispmm_sddmm_bf16.so: SDDMM on a CSR pattern with X and Y in bf16 (include/mispmm_sddmm_bf16.h):
// out[e] = <X[row(e), :], Y[col(e), :]> for every stored entry e of A, A's values unread.  The backward of C = A * B with
// respect to A's values is this product with X = dC, Y = B, both as the bf16 product keeps them.
//
// The kernel body, its shape (G lanes own one row of A, a lane owns V consecutive columns of each column chunk of G * V, batches
// of 8 entries, the transposing butterfly) and the launch ladder are csrc/sddmm_csr.hpp's, shared with csrc/sddmm.hip; here:
// the element policy (V8: one 16-byte buffer load per operand row and chunk, V1: one 2-byte load per column; a lane's slice
// stays raw bf16 bits and every element is widened exactly at its use, bits << 16), the two arithmetics, the kernel with its
// parameter list and its store (the out type is a wave-uniform branch there), the launch and the entry point.
// Fixed order throughout: run to run identical.  No LDS, no scratch, no atomics.
// The unit lies outside csrc/ and rows_bf16/: the census tests hold those directories' libraries to their records.
#include "mispmm_sddmm_bf16.h"
#include "bf16_lanes.hpp"
#include "sddmm_csr.hpp"

namespace mispmm {

namespace {

// the element policy of sddmm_csr.hpp: a lane's slice is raw bits, an element of it a float
struct SdBf16 {
    using in_t = uint16_t;
    static constexpr uint32_t kBytes = 2;
    template <int V> using raw_t = typename RawOf<V>::type;
    template <int V>
    static __device__ __forceinline__ raw_t<V> load(rsrc_t rsrc, uint32_t voffset) { return buffer_load_bf16<V>(rsrc, voffset); }
    template <int V>
    static __device__ __forceinline__ float at(const raw_t<V> &raw, int i) { return widen<V>(raw, i); }
};

// one rounding to nearest even, a NaN stays a NaN: v_cvt_pk_bf16_f32, the instruction of mispmm_f32_to_bf16
__device__ __forceinline__ uint16_t bf16_bits(float x) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(x)); }

// The two arithmetics (mispmm_sddmm_bf16.h, NUMERICS).  A: type of a partial sum.  No packed dot instruction: v_dot2_f32_bf16
// does not state its rounding.
struct SdRef {  // the bf16 x bf16 product is exact in fp64 (and in fp32): the fused form rounds once, at the add
    using A = double;
    static constexpr const char *tag = "ref64";
    static __device__ __forceinline__ void mac(A &acc, float x, float y) { acc = __builtin_fma(static_cast<double>(x), static_cast<double>(y), acc); }
    static __device__ __forceinline__ float finish(A acc) { return static_cast<float>(acc); }
};
struct SdFast {
    using A = float;
    static constexpr const char *tag = "fast";
    static __device__ __forceinline__ void mac(A &acc, float x, float y) { acc = __builtin_fmaf(x, y, acc); }
    static __device__ __forceinline__ float finish(A acc) { return acc; }
};

// the store: entry e of `out` in its type
struct SdStore {
    void *out;
    uint32_t out_bf16;
    __device__ __forceinline__ void operator()(size_t at, float res) const {
        if (out_bf16) static_cast<uint16_t *>(out)[at] = bf16_bits(res);  // wave-uniform
        else static_cast<float *>(out)[at] = res;
    }
};

template <class P, int G, int V, int NCH>
__global__ void __launch_bounds__(kSdBlock) sddmm_csr_bf16_kernel(uint32_t M, uint32_t N, uint32_t xcd_chunk, uint32_t ldx, uint32_t ldy,
                                                                  uint32_t out_bf16, const uint32_t *__restrict__ rowPtrs,
                                                                  const uint32_t *__restrict__ colIdxs, const uint16_t *__restrict__ X,
                                                                  uint32_t x_bytes, const uint16_t *__restrict__ Y, uint32_t y_bytes,
                                                                  void *__restrict__ out) {
    sddmm_csr_body<SdBf16, P, G, V, NCH>(M, N, xcd_chunk, ldx, ldy, rowPtrs, colIdxs, X, x_bytes, Y, y_bytes, SdStore{out, out_bf16});
}

struct SdArgs {
    hipStream_t stream;
    uint32_t M, K, N;
    const uint32_t *rowPtrs, *colIdxs;
    const uint16_t *X;
    uint32_t ldx;
    const uint16_t *Y;
    uint32_t ldy;
    void *out;
    bool out_bf16;
};

inline bool aligned_to(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// bytes from the first element of a [rows][ld] bf16 operand to the end of its last row's `width` columns
uint32_t span_bytes(uint64_t rows, uint32_t ld, uint32_t width) { return rows == 0 ? 0u : static_cast<uint32_t>(((rows - 1) * ld + width) * 2u); }

template <class P, int G, int V, int NCH>
void launch_sddmm(const SdArgs &a) {
    const XcdGrid xg = xcd_grid(ceil_div(a.M, static_cast<uint32_t>(kSdBlock / G)));
    note_kernel("sddmm_csr_bf16<%s,G%d,V%d,C%d> %s", P::tag, G, V, NCH, a.out_bf16 ? "bf16" : "f32");
    // both spans below 2 GiB (checked by the caller)
    hipLaunchKernelGGL((sddmm_csr_bf16_kernel<P, G, V, NCH>), dim3(xg.grid), dim3(kSdBlock), 0, a.stream, a.M, a.N, xg.chunk, a.ldx, a.ldy,
                       a.out_bf16 ? 1u : 0u, a.rowPtrs, a.colIdxs, a.X, span_bytes(a.M, a.ldx, a.N), a.Y, span_bytes(a.K, a.ldy, a.N), a.out);
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_sddmm_csr_bf16(mispmm_stream_t stream, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                     const uint32_t *colIdxs, const uint16_t *X, uint32_t ldx, const uint16_t *Y, uint32_t ldy, uint32_t N,
                                     void *out, int out_bf16, int acc_mode) {
    constexpr const char *name = "sddmm_csr_bf16";
    if (int s = check_acc_mode(name, acc_mode)) return s;
    if (ldx < N || ldy < N)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than N (N=%u ldx=%u ldy=%u)", name, N, ldx, ldy);
    if (M == 0 || nnz == 0) return MISPMM_OK;
    if (!rowPtrs || !colIdxs || !out) return fail(MISPMM_ERR_INVALID_ARG, "%s: rowPtrs, colIdxs or out is null", name);
    const uint32_t out_elem = out_bf16 ? 2u : 4u;
    if (!aligned_to(out, out_elem)) return fail(MISPMM_ERR_INVALID_ARG, "%s: out must be %u-byte aligned", name, out_elem);
    if (N == 0) {  // empty sums: +0, in either out type
        note_kernel("sddmm_csr_bf16<zero>");
        MISPMM_HIP_TRY(hipMemsetAsync(out, 0, static_cast<size_t>(nnz) * out_elem, as_stream(stream)));
        return MISPMM_OK;
    }
    if (!X || !Y) return fail(MISPMM_ERR_INVALID_ARG, "%s: X or Y is null", name);
    if (!aligned_to(X, 2) || !aligned_to(Y, 2)) return fail(MISPMM_ERR_INVALID_ARG, "%s: X and Y must be 2-byte aligned", name);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    if (!fits_buffer(M, ldx, 2) || !fits_buffer(K, ldy, 2))
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: X or Y spans 2 GiB or more (M=%u ldx=%u K=%u ldy=%u); there is no wide body", name, M, ldx, K, ldy);
    const SdArgs a{as_stream(stream), M, K, N, rowPtrs, colIdxs, X, ldx, Y, ldy, out, out_bf16 != 0};
    const bool wide = N % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && aligned16(X) && aligned16(Y);
    with_acc<SdRef, SdFast>(acc_mode, [&](auto acc) {
        with_const<8, 1>(wide ? 8 : 1, [&](auto v) {
            launch_sddmm_shape<decltype(v)::value>(N, [&](auto g, auto c) {
                launch_sddmm<typename decltype(acc)::type, decltype(g)::value, decltype(v)::value, decltype(c)::value>(a);
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
