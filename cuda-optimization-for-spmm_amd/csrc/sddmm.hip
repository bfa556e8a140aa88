// SDDMM on a CSR pattern: out[e] = <X[row(e), :], Y[col(e), :]> for every stored entry e of A (A's values are not read).
// The backward of C = A * B with respect to A's values is this product with X = dC, Y = B.
//
// Shape: the row-gather kernel's (row_gather.hpp) -- G lanes own one row of A, a lane owns VEC consecutive columns of each
// column chunk of G * VEC.  The group keeps its slice of X[row] in registers (up to 4 chunks; wider
// rows re-read X per batch, from L1), walks the row's entries in batches of 8 with the 8 x NCH Y-row reads of a batch
// independent of each other, and sums every lane's 8 partial dot products across the group with a TRANSPOSING butterfly:
// in step k a lane keeps the half of its values whose entry number has bit k equal to its own lane bit k and hands the other
// half to lane ^ (1 << k), so 8 values cross the group in 4 + 2 + 1 moves (then one per further doubling of G) instead of
// 8 * log2(G), and lane i of the group ends up with the result of entry i of the batch: lanes 0..7 store 8 consecutive
// elements of `out`.  The moves (lane_moves.hpp) are DPP (quad_perm, row_ror) or ds_swizzle; lane ^ 32 goes through ds_bpermute.
// A batch's column keys reach the group by DPP row_newbcast: per key two moves (lane j and lane 8 + j of the 16-lane row) and
// a select on the lane's own half, 16 moves per batch; with G >= 16 one move would do (both halves hold the same keys).
// Fixed order throughout: run to run identical.  No LDS, no scratch.
#include "lane_moves.hpp"

namespace mispmm {

namespace {

constexpr int kSdBlock = 256;  // threads per workgroup
constexpr int kSdBatch = 8;    // entries of a row summed at once: lane i < 8 of a group stores the i-th

template <class T, int VEC> struct SdVec;
template <> struct SdVec<float, 1> { using type = float; };
template <> struct SdVec<float, 4> { using type = f32x4; };
template <> struct SdVec<double, 1> { using type = double; };
template <> struct SdVec<double, 2> { using type = double __attribute__((ext_vector_type(2))); };

template <class T, int VEC>
__device__ __forceinline__ typename SdVec<T, VEC>::type sd_load(rsrc_t rsrc, uint32_t voffset) {
    using vec_t = typename SdVec<T, VEC>::type;
    if constexpr (sizeof(vec_t) == 4) return __builtin_bit_cast(vec_t, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voffset, 0, 0));
    else if constexpr (sizeof(vec_t) == 8) return __builtin_bit_cast(vec_t, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voffset, 0, 0));
    else return __builtin_bit_cast(vec_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, 0, 0));
}
template <class T, int VEC>
__device__ __forceinline__ T sd_get(const typename SdVec<T, VEC>::type &v, int i) {
    if constexpr (VEC == 1) return v; else return v[i];
}

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

// one step of the transposing butterfly: 2 * H values in, H out; the lane whose bit MASK is clear keeps the even ones
template <int MASK, int H, class A>
__device__ __forceinline__ void fold(const A *in, A *out, bool odd) {
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const A keep = odd ? in[2 * j + 1] : in[2 * j];
        const A send = odd ? in[2 * j] : in[2 * j + 1];
        out[j] = keep + lane_xor<MASK>(send);
    }
}

// NCH > 0: the group's slice of X[row] -- NCH chunks of G * VEC columns -- lives in registers; NCH == 0 (G = 64 only): any N,
// X re-read chunk by chunk for every batch of entries.
template <class P, int G, int VEC, int NCH>
__global__ void __launch_bounds__(kSdBlock) sddmm_csr_kernel(uint32_t M, uint32_t N, uint32_t xcd_chunk, uint32_t ldx, uint32_t ldy,
                                                             const uint32_t *__restrict__ rowPtrs, const uint32_t *__restrict__ colIdxs,
                                                             const typename P::T *__restrict__ X, uint32_t x_bytes,
                                                             const typename P::T *__restrict__ Y, uint32_t y_bytes,
                                                             typename P::T *__restrict__ out) {
    using T = typename P::T;
    using A = typename P::A;
    using vec_t = typename SdVec<T, VEC>::type;
    static_assert(G >= kSdBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's results sit in the first lanes of a group");
    static_assert(NCH > 0 || G == kWave, "the chunk loop is for rows wider than a wave");
    constexpr int GROUPS = kSdBlock / G, E = kSdBatch;
    constexpr uint32_t ES = sizeof(T), CHUNK = G * VEC;
    const uint32_t lane = threadIdx.x % G, sub = lane & (E - 1);
    const uint64_t row64 = static_cast<uint64_t>(xcd_block(blockIdx.x, xcd_chunk)) * GROUPS + threadIdx.x / G;
    const bool row_ok = row64 < M;
    const uint32_t row = static_cast<uint32_t>(row64);
    uint32_t base = 0, len = 0;
    if (row_ok) {
        base = rowPtrs[row];
        len = rowPtrs[row + 1] - base;
    }
    if (len == 0) return;  // the lanes a move reads from are all in the lane's own group, which leaves as one

    const rsrc_t xr = make_rsrc(X, x_bytes), yr = make_rsrc(Y, y_bytes);
    const uint32_t x_row = row * ldx * ES;  // < 2 GiB: the host declines anything larger
    const uint32_t ldy_bytes = ldy * ES;
    // byte offset of the lane's columns in chunk c, kDropLoad past N: such a load returns zeros, so a masked lane adds
    // 0 * 0 = +0 to every live slot (neither the gap columns of a strided operand nor anything behind it is ever read)
    auto col_off = [&](uint32_t c0) {
        const uint32_t col = c0 + lane * VEC;
        return col < N ? col * ES : kDropLoad;
    };
    // A Y read's offset is key + column offset and either part may be kDropLoad.  Both at once -- a slot past the row end
    // in a lane past N -- wrap to offset 0: that lane really reads Y[0][0..VEC).  It is an in-range read that changes no
    // result: the lane's X is zero, the product (0 * y, a NaN if y is not finite) lands only in the sum of a slot past the
    // row end, the butterfly keeps the slots apart and the store is guarded.
    uint32_t off[NCH > 0 ? NCH : 1];
    vec_t xv[NCH > 0 ? NCH : 1];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            off[c] = col_off(c * CHUNK);
            xv[c] = sd_load<T, VEC>(xr, x_row + off[c]);
        }
    }
    // entry c0 + sub of the row: every 8-lane segment of the group holds the batch's 8 columns
    auto fetch = [&](uint32_t c0) {
        const uint32_t idx = c0 + sub;
        return colIdxs[static_cast<size_t>(base) + (idx < len ? idx : 0u)];
    };
    uint32_t nxt = fetch(0);
    for (uint32_t s0 = 0; s0 < len; s0 += E) {
        // a slot past the row end gets key kDropLoad: zeros, and a result nobody stores
        const uint32_t key = s0 + sub < len ? nxt * ldy_bytes : kDropLoad;
        nxt = fetch(s0 + E);  // on its way while this batch is gathered
        A acc[E];
#pragma unroll
        for (int j = 0; j < E; ++j) acc[j] = A(0);
        if constexpr (NCH > 0) {
            static_for<0, E>([&](auto j_tag) {
                constexpr int j = decltype(j_tag)::value;
                const uint32_t kj = group_bcast<8, j>(key);
                vec_t yv[NCH];
#pragma unroll
                for (int c = 0; c < NCH; ++c) yv[c] = sd_load<T, VEC>(yr, kj + off[c]);
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) P::mac(acc[j], sd_get<T, VEC>(xv[c], v), sd_get<T, VEC>(yv[c], v));
            });
        } else {
            uint32_t kj[E];
            static_for<0, E>([&](auto j_tag) { kj[decltype(j_tag)::value] = group_bcast<8, decltype(j_tag)::value>(key); });
            for (uint32_t c0 = 0; c0 < N; c0 += CHUNK) {
                const uint32_t o = col_off(c0);
                const vec_t x = sd_load<T, VEC>(xr, x_row + o);
                vec_t yv[E];
#pragma unroll
                for (int j = 0; j < E; ++j) yv[j] = sd_load<T, VEC>(yr, kj[j] + o);
#pragma unroll
                for (int j = 0; j < E; ++j)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) P::mac(acc[j], sd_get<T, VEC>(x, v), sd_get<T, VEC>(yv[j], v));
            }
        }
        A w[4], u[2], z[1];
        fold<1, 4>(acc, w, (lane & 1u) != 0);
        fold<2, 2>(w, u, (lane & 2u) != 0);
        fold<4, 1>(u, z, (lane & 4u) != 0);
        A r = z[0];
        if constexpr (G >= 16) r = r + lane_xor<8>(r);
        if constexpr (G >= 32) r = r + lane_xor<16>(r);
        if constexpr (G >= 64) r = r + lane_xor<32>(r);
        if (lane < E && s0 + lane < len) out[static_cast<size_t>(base) + s0 + lane] = P::finish(r);
    }
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

template <class P, int VEC>
void launch_sddmm_shape(const SdArgs<typename P::T> &a) {
    if (try_const<8, 16, 32>(pick_group(a.N, VEC), [&](auto g) { launch_sddmm<P, decltype(g)::value, VEC, 1>(a); })) return;
    // a whole wave per row: 1, 2 or 4 chunks of 64 lanes held in registers, 0 = a loop over any number
    const uint32_t chunks = ceil_div(a.N, static_cast<uint32_t>(kWave * VEC));
    with_const<1, 2, 4, 0>(chunks <= 1 ? 1 : chunks == 2 ? 2 : chunks <= 4 ? 4 : 0, [&](auto c) { launch_sddmm<P, 64, VEC, decltype(c)::value>(a); });
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
        with_const<WIDE, 1>(wide ? WIDE : 1, [&](auto v) { launch_sddmm_shape<typename decltype(acc)::type, decltype(v)::value>(a); });
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
