// SDDMM on a CSR pattern in fp32 and fp64: out[e] = <X[row(e), :], Y[col(e), :]> for every stored entry e of A (A's values are
// not read).  The backward of C = A * B with respect to A's values is this product with X = dC, Y = B.
// The kernel body, its shape and the launch ladder are sddmm_csr.hpp's; here: the element policy over T, the four arithmetics,
// the kernel with its parameter list and its store, the launch and the entry points.
#include "sddmm_csr.hpp"

namespace mispmm {

namespace {

template <class T, int VEC> struct SdVec;
template <> struct SdVec<float, 1> { using type = float; };
template <> struct SdVec<float, 4> { using type = f32x4; };
template <> struct SdVec<double, 1> { using type = double; };
template <> struct SdVec<double, 2> { using type = double __attribute__((ext_vector_type(2))); };

// the element policy of sddmm_csr.hpp: a lane's slice is a T or a 16-byte vector of T
template <class T>
struct SdElem {
    using in_t = T;
    static constexpr uint32_t kBytes = sizeof(T);
    template <int VEC> using raw_t = typename SdVec<T, VEC>::type;
    template <int VEC>
    static __device__ __forceinline__ raw_t<VEC> load(rsrc_t rsrc, uint32_t voffset) {
        if constexpr (sizeof(raw_t<VEC>) == 4) return __builtin_bit_cast(raw_t<VEC>, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voffset, 0, 0));
        else if constexpr (sizeof(raw_t<VEC>) == 8) return __builtin_bit_cast(raw_t<VEC>, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voffset, 0, 0));
        else return __builtin_bit_cast(raw_t<VEC>, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, 0, 0));
    }
    template <int VEC>
    static __device__ __forceinline__ T at(const raw_t<VEC> &v, int i) {
        if constexpr (VEC == 1) return v; else return v[i];
    }
};

// The four arithmetics (mispmm.h, section SDDMM).  T: operand type, A: type of a partial sum.
struct SdF32Ref {  // the fp32 x fp32 product is exact in fp64, so the fused form rounds exactly where mul + add would: once, at the add
    using T = float; using A = double;
    static constexpr const char *tag = "f32,ref64";
    static __device__ __forceinline__ void mac(A &acc, T x, T y) { acc = __builtin_fma(static_cast<double>(x), static_cast<double>(y), acc); }
    static __device__ __forceinline__ T finish(A acc) { return static_cast<float>(acc); }
};
struct SdF32Fast {
    using T = float; using A = float;
    static constexpr const char *tag = "f32,fast";
    static __device__ __forceinline__ void mac(A &acc, T x, T y) { acc = __builtin_fmaf(x, y, acc); }
    static __device__ __forceinline__ T finish(A acc) { return acc; }
};
struct SdF64Ref {  // -ffp-contract=off keeps the product and the add apart
    using T = double; using A = double;
    static constexpr const char *tag = "f64,ref";
    static __device__ __forceinline__ void mac(A &acc, T x, T y) {
        const double p = x * y;
        acc = acc + p;
    }
    static __device__ __forceinline__ T finish(A acc) { return acc; }
};
struct SdF64Fast {
    using T = double; using A = double;
    static constexpr const char *tag = "f64,fast";
    static __device__ __forceinline__ void mac(A &acc, T x, T y) { acc = __builtin_fma(x, y, acc); }
    static __device__ __forceinline__ T finish(A acc) { return acc; }
};

// the store: entry e of `out`
template <class T>
struct SdStore {
    T *out;
    __device__ __forceinline__ void operator()(size_t e, T r) const { out[e] = r; }
};

template <class P, int G, int VEC, int NCH>
__global__ void __launch_bounds__(kSdBlock) sddmm_csr_kernel(uint32_t M, uint32_t N, uint32_t xcd_chunk, uint32_t ldx, uint32_t ldy,
                                                             const uint32_t *__restrict__ rowPtrs, const uint32_t *__restrict__ colIdxs,
                                                             const typename P::T *__restrict__ X, uint32_t x_bytes,
                                                             const typename P::T *__restrict__ Y, uint32_t y_bytes,
                                                             typename P::T *__restrict__ out) {
    using T = typename P::T;
    sddmm_csr_body<SdElem<T>, P, G, VEC, NCH>(M, N, xcd_chunk, ldx, ldy, rowPtrs, colIdxs, X, x_bytes, Y, y_bytes, SdStore<T>{out});
}

template <class T>
struct SdArgs {
    hipStream_t stream;
    uint32_t M, K, N;
    const uint32_t *rowPtrs, *colIdxs;
    const T *X;
    uint32_t ldx;
    const T *Y;
    uint32_t ldy;
    T *out;
};

template <class P, int G, int VEC, int NCH>
void launch_sddmm(const SdArgs<typename P::T> &a) {
    constexpr uint32_t ES = sizeof(typename P::T);
    const XcdGrid xg = xcd_grid(ceil_div(a.M, static_cast<uint32_t>(kSdBlock / G)));
    note_kernel("sddmm_csr<%s,G%d,V%d,C%d>", P::tag, G, VEC, NCH);
    hipLaunchKernelGGL((sddmm_csr_kernel<P, G, VEC, NCH>), dim3(xg.grid), dim3(kSdBlock), 0, a.stream, a.M, a.N, xg.chunk, a.ldx, a.ldy,
                       a.rowPtrs, a.colIdxs, a.X, static_cast<uint32_t>(static_cast<uint64_t>(a.M) * a.ldx * ES), a.Y,
                       static_cast<uint32_t>(static_cast<uint64_t>(a.K) * a.ldy * ES), a.out);
}

template <class PRef, class PFast>
int sddmm_csr(const char *name, mispmm_stream_t stream, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
              const uint32_t *colIdxs, const typename PRef::T *X, uint32_t ldx, const typename PRef::T *Y, uint32_t ldy, uint32_t N,
              typename PRef::T *out, int acc_mode) {
    using T = typename PRef::T;
    constexpr int WIDE = 16 / sizeof(T);  // elements of a 16-byte lane
    if (int s = check_acc_mode(name, acc_mode)) return s;
    if (M == 0 || nnz == 0) return MISPMM_OK;
    if (!rowPtrs || !colIdxs || !out) return fail(MISPMM_ERR_INVALID_ARG, "%s: rowPtrs, colIdxs or out is null", name);
    if (ldx < N || ldy < N)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than N (N=%u ldx=%u ldy=%u)", name, N, ldx, ldy);
    if (N == 0) {  // empty sums: +0
        note_kernel("sddmm_csr<zero>");
        MISPMM_HIP_TRY(hipMemsetAsync(out, 0, static_cast<size_t>(nnz) * sizeof(T), as_stream(stream)));
        return MISPMM_OK;
    }
    if (!X || !Y) return fail(MISPMM_ERR_INVALID_ARG, "%s: X or Y is null", name);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    if (!fits_buffer(M, ldx, sizeof(T)) || !fits_buffer(K, ldy, sizeof(T)))
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: X or Y spans 2 GiB or more (M=%u ldx=%u K=%u ldy=%u)", name, M, ldx, K, ldy);
    const SdArgs<T> a{as_stream(stream), M, K, N, rowPtrs, colIdxs, X, ldx, Y, ldy, out};
    const bool wide = N % WIDE == 0 && ldx % WIDE == 0 && ldy % WIDE == 0 && aligned16(X) && aligned16(Y);
    with_acc<PRef, PFast>(acc_mode, [&](auto acc) {
        with_const<WIDE, 1>(wide ? WIDE : 1, [&](auto v) {
            launch_sddmm_shape<decltype(v)::value>(N, [&](auto g, auto c) {
                launch_sddmm<typename decltype(acc)::type, decltype(g)::value, decltype(v)::value, decltype(c)::value>(a);
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_sddmm_csr_f32(mispmm_stream_t stream, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                    const uint32_t *colIdxs, const float *X, uint32_t ldx, const float *Y, uint32_t ldy, uint32_t N,
                                    float *out, int acc_mode) {
    return sddmm_csr<SdF32Ref, SdF32Fast>("sddmm_csr_f32", stream, M, K, nnz, rowPtrs, colIdxs, X, ldx, Y, ldy, N, out, acc_mode);
}

extern "C" int mispmm_sddmm_csr_f64(mispmm_stream_t stream, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                    const uint32_t *colIdxs, const double *X, uint32_t ldx, const double *Y, uint32_t ldy, uint32_t N,
                                    double *out, int acc_mode) {
    return sddmm_csr<SdF64Ref, SdF64Fast>("sddmm_csr_f64", stream, M, K, nnz, rowPtrs, colIdxs, X, ldx, Y, ldy, N, out, acc_mode);
}
