// libmispmm_sddmm_bf16.so: SDDMM on a CSR pattern with X and Y in bf16 (include/mispmm_sddmm_bf16.h):
// out[e] = <X[row(e), :], Y[col(e), :]> for every stored entry e of A, A's values unread.  The backward of C = A * B with
// respect to A's values is this product with X = dC, Y = B, both as the bf16 product keeps them.
//
// The shape is csrc/sddmm.hip's, COPIED for another element width rather than templated there (the census tests hold that
// unit's instances to their record): G lanes own one row of A, a lane owns V consecutive columns of each column chunk of
// G * V (V8: one 16-byte buffer load per operand row and chunk, V1: one 2-byte load per column).  The group keeps its slice
// of X[row] in registers as raw bf16 bits (up to 4 chunks; wider rows re-read X per batch, from L1), walks the row's entries
// in batches of 8 with the 8 x NCH Y-row reads of a batch independent of each other, widens every element exactly at its
// use (bits << 16), and sums every lane's 8 partial dot products across the group with the TRANSPOSING butterfly of
// sddmm.hip: in step k a lane keeps the half of its values whose entry number has bit k equal to its own lane bit k and
// hands the other half to lane ^ (1 << k), so lane i of the group ends up with the result of entry i of the batch and lanes
// 0..7 store 8 consecutive elements of `out`.  The out type is a wave-uniform branch at that store.
// Fixed order throughout: run to run identical.  No LDS, no scratch, no atomics.
// The sources lie outside csrc/ and rows_bf16/: the census tests hold those directories and their libraries to their records.
#include "mispmm_sddmm_bf16.h"
#include "lane_moves.hpp"

namespace mispmm {

namespace {

constexpr int kSdBlock = 256;  // threads per workgroup
constexpr int kSdBatch = 8;    // entries of a row summed at once: lane i < 8 of a group stores the i-th

using u32x4 = uint32_t __attribute__((ext_vector_type(4)));

// V bf16 elements as they are loaded: element 2i in the low half of dword i, element 2i + 1 in the high half
template <int V> struct RawOf;
template <> struct RawOf<1> { using type = uint32_t; };
template <> struct RawOf<8> { using type = u32x4; };

template <int V>
__device__ __forceinline__ typename RawOf<V>::type sd_load(rsrc_t rsrc, uint32_t voffset) {
    if constexpr (V == 1) return __builtin_amdgcn_raw_buffer_load_b16(rsrc, voffset, 0, 0);
    else return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, 0, 0);
}

// element i widened to fp32 exactly: the bits moved to the upper half, nothing flushed or quieted
template <int V>
__device__ __forceinline__ float widen(const typename RawOf<V>::type &raw, int i) {
    if constexpr (V == 1) return __uint_as_float(raw << 16);
    else return __uint_as_float((i & 1) ? (raw[i >> 1] & 0xFFFF0000u) : (raw[i >> 1] << 16));
}

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

// NCH > 0: the group's slice of X[row] -- NCH chunks of G * V columns -- lives in registers; NCH == 0 (G = 64 only): any N,
// X re-read chunk by chunk for every batch of entries.
template <class P, int G, int V, int NCH>
__global__ void __launch_bounds__(kSdBlock) sddmm_csr_bf16_kernel(uint32_t M, uint32_t N, uint32_t xcd_chunk, uint32_t ldx, uint32_t ldy,
                                                                  uint32_t out_bf16, const uint32_t *__restrict__ rowPtrs,
                                                                  const uint32_t *__restrict__ colIdxs, const uint16_t *__restrict__ X,
                                                                  uint32_t x_bytes, const uint16_t *__restrict__ Y, uint32_t y_bytes,
                                                                  void *__restrict__ out) {
    using A = typename P::A;
    using raw_t = typename RawOf<V>::type;
    static_assert(G >= kSdBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's results sit in the first lanes of a group");
    static_assert(NCH > 0 || G == kWave, "the chunk loop is for rows wider than a wave");
    constexpr int GROUPS = kSdBlock / G, E = kSdBatch;
    constexpr uint32_t ES = 2, CHUNK = G * V;
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
    // 0 * 0 = +0 to every live slot (neither the gap columns of a strided operand nor anything behind it is ever read).
    // V8: N is a multiple of 8, so a lane's columns lie inside N or past it together
    auto col_off = [&](uint32_t c0) {
        const uint32_t col = c0 + lane * V;
        return col < N ? col * ES : kDropLoad;
    };
    // A Y read's offset is key + column offset and either part may be kDropLoad.  Both at once -- a slot past the row end
    // in a lane past N -- wrap to offset 0: that lane really reads Y[0][0..V) (zeros where Y is shorter than that).  It is
    // an in-range read that changes no result: the lane's X is zero, the product (0 * y, a NaN if y is not finite) lands
    // only in the sum of a slot past the row end, the butterfly keeps the slots apart and the store is guarded.
    uint32_t off[NCH > 0 ? NCH : 1];
    raw_t xv[NCH > 0 ? NCH : 1];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            off[c] = col_off(c * CHUNK);
            xv[c] = sd_load<V>(xr, x_row + off[c]);
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
                raw_t yv[NCH];
#pragma unroll
                for (int c = 0; c < NCH; ++c) yv[c] = sd_load<V>(yr, kj + off[c]);
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int v = 0; v < V; ++v) P::mac(acc[j], widen<V>(xv[c], v), widen<V>(yv[c], v));
            });
        } else {
            uint32_t kj[E];
            static_for<0, E>([&](auto j_tag) { kj[decltype(j_tag)::value] = group_bcast<8, decltype(j_tag)::value>(key); });
            for (uint32_t c0 = 0; c0 < N; c0 += CHUNK) {
                const uint32_t o = col_off(c0);
                const raw_t x = sd_load<V>(xr, x_row + o);
                raw_t yv[E];
#pragma unroll
                for (int j = 0; j < E; ++j) yv[j] = sd_load<V>(yr, kj[j] + o);
#pragma unroll
                for (int j = 0; j < E; ++j)
#pragma unroll
                    for (int v = 0; v < V; ++v) P::mac(acc[j], widen<V>(x, v), widen<V>(yv[j], v));
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
        if (lane < E && s0 + lane < len) {
            const size_t at = static_cast<size_t>(base) + s0 + lane;
            const float res = P::finish(r);
            if (out_bf16) static_cast<uint16_t *>(out)[at] = bf16_bits(res);  // wave-uniform
            else static_cast<float *>(out)[at] = res;
        }
    }
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

// the chunk ladder of csrc/sddmm.hip (launch_sddmm_shape)
template <class P, int V>
void launch_sddmm_shape(const SdArgs &a) {
    if (try_const<8, 16, 32>(pick_group(a.N, V), [&](auto g) { launch_sddmm<P, decltype(g)::value, V, 1>(a); })) return;
    // a whole wave per row: 1, 2 or 4 chunks of 64 lanes held in registers, 0 = a loop over any number
    const uint32_t chunks = ceil_div(a.N, static_cast<uint32_t>(kWave * V));
    with_const<1, 2, 4, 0>(chunks <= 1 ? 1 : chunks == 2 ? 2 : chunks <= 4 ? 4 : 0, [&](auto c) { launch_sddmm<P, 64, V, decltype(c)::value>(a); });
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
        with_const<8, 1>(wide ? 8 : 1, [&](auto v) { launch_sddmm_shape<typename decltype(acc)::type, decltype(v)::value>(a); });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
