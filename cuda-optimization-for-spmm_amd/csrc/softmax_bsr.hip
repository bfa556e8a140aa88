// Row softmax on a BSR block pattern and its backward (mispmm.h, section "Row softmax on a BSR pattern"): the step between
// the block scores of mispmm_sddmm_bsr_bf16 (fp32) and the blocks mispmm_bsr_bf16 multiplies by (bf16).
//   forward   z = fl32(scale * s + mask)   (one fma; without a mask the product scale * s)
//             out[e][i][j] = exp(z - m) / sum_row exp(z - m),   m the largest z of matrix row R * bS + i
//   backward  ds[e][i][j] = scale * p * (dp - sum_row p * dp)
// Matrix row R * bS + i owns element row i of every block e in [blockRowPtrs[R], blockRowPtrs[R + 1]).  Block column indices
// and A's values are not read.
//
// Shape: one workgroup of 4 waves per block row, the row's blocks dealt to the waves in turn (wave w takes blocks w, w + 4,
// ... of the row), as the SDDMM and the product have it.  A block is read in 16-byte lanes: lane l of a wave holds the 4
// consecutive elements 4 l .. 4 l + 3 of a 256-element step, i.e. of element row (64 step + l) / G, G = bS / 4 lanes to a
// row -- one step and one row per lane at 16 x 16, four steps and four rows (8 apart) per lane at 32 x 32.  A lane reduces
// its own elements per row in ascending order (block by block, then left to right), the G lanes of a row meet in a
// butterfly of xor moves (lane_moves.hpp), and the four waves' partial results meet through 512 bytes of LDS and a
// barrier, combined as ((w0 + w1) + w2) + w3 by every lane for itself: the order of every sum is fixed by the block row's
// length alone.  No atomics.
// A block row of up to C blocks (kHeld: 32 at 16 x 16, 16 at 32 x 32) is read ONCE and held in registers through max, exp
// and sum, divide and store.  A longer one goes in three walks (max; sum; write -- backward two: sum; write) over the same
// blocks in the same order, the re-reads served by L1 / L2 and the exponentials computed twice: to the same bits.  The
// choice is per block row, workgroup-uniform.
//
// Special values need no branch, as in softmax_csr.hip: fmax drops a NaN operand, so m is the largest non-NaN z (-Inf if
// there is none) and the NaN is carried by the sum: NaN - m = NaN, exp(NaN) = NaN, and a NaN term makes the sum and every
// quotient of the row NaN.  m = +Inf gives Inf - Inf = NaN for that element, m = -Inf gives -Inf - -Inf = NaN for every
// element.  A -Inf beside a finite z is exp(-Inf) = +0 and +0 / sum = +0.  The rows of a block are reduced apart, so a NaN
// stays in its matrix row.
#include "lane_moves.hpp"

namespace mispmm {

namespace {

constexpr int kSbmWaves = 4;

// blocks of a block row that are held in registers (C in mispmm.h and in the kernel tag)
template <int BS> constexpr int kHeld = BS == 16 ? 32 : 16;

using f32x4_t = float __attribute__((ext_vector_type(4)));
// the arrays are only as aligned as their element type: global vector loads and stores take any address
using mem_f32x4_t = float __attribute__((ext_vector_type(4), aligned(4)));
using mem_u16x4_t = uint16_t __attribute__((ext_vector_type(4), aligned(2)));

__device__ __forceinline__ float sbm_exp(float t) { return __builtin_amdgcn_exp2f(t * 1.44269504088896340736f); }  // as SmF32Fast
__device__ __forceinline__ float sbm_max(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ float sbm_add(float a, float b) { return a + b; }

__device__ __forceinline__ f32x4_t load_f32(const float *p, size_t at) {
    const mem_f32x4_t v = *reinterpret_cast<const mem_f32x4_t *>(p + at);
    return f32x4_t{v[0], v[1], v[2], v[3]};
}
// bf16 bits widened: exact
__device__ __forceinline__ f32x4_t load_bf16(const uint16_t *p, size_t at) {
    const mem_u16x4_t v = *reinterpret_cast<const mem_u16x4_t *>(p + at);
    f32x4_t r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = __uint_as_float(static_cast<uint32_t>(v[k]) << 16);
    return r;
}
template <bool BF16>
__device__ __forceinline__ f32x4_t load_any(const void *p, size_t at) {
    if constexpr (BF16) return load_bf16(static_cast<const uint16_t *>(p), at);
    else return load_f32(static_cast<const float *>(p), at);
}
template <bool BF16>
__device__ __forceinline__ void store_any(void *p, size_t at, f32x4_t v) {
    if constexpr (BF16) {
        mem_u16x4_t o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = __builtin_bit_cast(uint16_t, static_cast<__bf16>(v[k]));  // v_cvt_pk_bf16_f32, as mispmm_f32_to_bf16: RNE, a NaN stays a NaN
        *reinterpret_cast<mem_u16x4_t *>(static_cast<uint16_t *>(p) + at) = o;
    } else {
        *reinterpret_cast<mem_f32x4_t *>(static_cast<float *>(p) + at) = mem_f32x4_t{v[0], v[1], v[2], v[3]};
    }
}

// z = fl32(scale * s + mask), one fma; without a mask the product
__device__ __forceinline__ f32x4_t scaled(f32x4_t s, f32x4_t m, float scale) {
    f32x4_t z;
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = __builtin_fmaf(scale, s[k], m[k]);
    return z;
}
__device__ __forceinline__ f32x4_t scaled(f32x4_t s, float scale) { return f32x4_t{scale * s[0], scale * s[1], scale * s[2], scale * s[3]}; }

// What a block row's lanes share.  R: 256-element steps of a block = element rows a lane holds; G: lanes to an element row.
template <int BS>
struct Rows {
    static constexpr int R = BS * BS / 256;
    static constexpr int G = BS / 4;
    static constexpr int kStepRows = kWave / G;  // element rows of one step

    // v[k]: this lane's partial result for its row of step k.  Afterwards: the block row's, in every lane.
    template <class F>
    static __device__ __forceinline__ void meet(float (&v)[R], float (*lds)[BS], uint32_t wave, uint32_t lane, F f) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            v[k] = group_all_reduce<G>(v[k], f);
            lds[wave][k * kStepRows + lane / G] = v[k];  // the G lanes of a row write one value
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const uint32_t row = k * kStepRows + lane / G;
            v[k] = f(f(f(lds[0][row], lds[1][row]), lds[2][row]), lds[3][row]);
        }
    }
};

// the lane's element offset of step k in block e
template <int BS>
__device__ __forceinline__ size_t at_of(uint32_t e, int k, uint32_t lane) {
    return static_cast<size_t>(e) * (BS * BS) + static_cast<size_t>(k * 256 + lane * 4);
}

// One walk of a wave over its blocks first, first + 4, ... of a block row, in that order: `use(e, k, load(e, k))` for every
// block e and step k.  A step of the walk takes 4 / R blocks, so that four 16-byte loads per lane and array are in flight;
// its loads are issued before anything of it is used.
template <int BS, class V, class L, class U>
__device__ __forceinline__ void walk(uint32_t first, uint32_t be, L load, U use) {
    constexpr int R = Rows<BS>::R, N = 4 / R;
#pragma unroll 1
    for (uint32_t e0 = first; e0 < be; e0 += N * kSbmWaves) {
        V v[N][R];
#pragma unroll
        for (int n = 0; n < N; ++n)
            if (e0 + n * kSbmWaves < be) {  // wave-uniform
#pragma unroll
                for (int k = 0; k < R; ++k) v[n][k] = load(e0 + n * kSbmWaves, k);
            }
#pragma unroll
        for (int n = 0; n < N; ++n)
            if (e0 + n * kSbmWaves < be) {
#pragma unroll
                for (int k = 0; k < R; ++k) use(e0 + n * kSbmWaves, k, v[n][k]);
            }
    }
}

__device__ __forceinline__ float max4(float m, f32x4_t z) { return sbm_max(sbm_max(sbm_max(sbm_max(m, z[0]), z[1]), z[2]), z[3]); }

template <int BS, bool MASK, bool OUT_BF16>
__global__ void __launch_bounds__(64 * kSbmWaves) softmax_bsr_kernel(uint32_t Mb, const uint32_t *__restrict__ blockRowPtrs,
                                                                      const float *__restrict__ scores, const float *__restrict__ mask,
                                                                      float scale, void *__restrict__ out) {
    using RW = Rows<BS>;
    constexpr int R = RW::R;
    constexpr int CB = kHeld<BS> / kSbmWaves;  // held blocks per wave
    __shared__ float lds_max[kSbmWaves][BS], lds_sum[kSbmWaves][BS];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t Rb = blockIdx.x;
    if (Rb >= Mb) return;
    const uint32_t bs = blockRowPtrs[Rb], be = blockRowPtrs[Rb + 1];
    if (be <= bs) return;  // an empty block row: the whole workgroup leaves, before any barrier
    const float ninf = -__builtin_huge_valf();
    float m[R], sum[R];
#pragma unroll
    for (int k = 0; k < R; ++k) m[k] = ninf, sum[k] = 0.f;

    if (be - bs <= static_cast<uint32_t>(kHeld<BS>)) {
        // No branch around a load or a value: a block past the row's end reads the row's last block instead (valid memory,
        // a cache hit) and takes part as -Inf, which the max ignores and the sum counts as exp(-Inf) = +0.
        f32x4_t z[CB][R];
#pragma unroll
        for (int b = 0; b < CB; ++b) {
            const uint32_t e = bs + wave + b * kSbmWaves;
            const bool there = e < be;  // wave-uniform
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const size_t at = at_of<BS>(there ? e : be - 1, k, lane);
                f32x4_t v;
                if constexpr (MASK) v = scaled(load_f32(scores, at), load_f32(mask, at), scale);
                else v = scaled(load_f32(scores, at), scale);
                z[b][k] = there ? v : f32x4_t{ninf, ninf, ninf, ninf};
            }
        }
#pragma unroll
        for (int b = 0; b < CB; ++b)
#pragma unroll
            for (int k = 0; k < R; ++k) m[k] = max4(m[k], z[b][k]);
        RW::meet(m, lds_max, wave, lane, sbm_max);
#pragma unroll
        for (int b = 0; b < CB; ++b)
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    z[b][k][j] = sbm_exp(z[b][k][j] - m[k]);
                    sum[k] = sum[k] + z[b][k][j];
                }
        RW::meet(sum, lds_sum, wave, lane, sbm_add);
#pragma unroll
        for (int b = 0; b < CB; ++b) {
            const uint32_t e = bs + wave + b * kSbmWaves;
            if (e < be) {
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    f32x4_t q;
#pragma unroll
                    for (int j = 0; j < 4; ++j) q[j] = z[b][k][j] / sum[k];
                    store_any<OUT_BF16>(out, at_of<BS>(e, k, lane), q);
                }
            }
        }
        return;
    }

    auto z_of = [&](uint32_t e, int k) {
        const size_t at = at_of<BS>(e, k, lane);
        if constexpr (MASK) return scaled(load_f32(scores, at), load_f32(mask, at), scale);
        else return scaled(load_f32(scores, at), scale);
    };
    walk<BS, f32x4_t>(bs + wave, be, z_of, [&](uint32_t, int k, f32x4_t z) { m[k] = max4(m[k], z); });
    RW::meet(m, lds_max, wave, lane, sbm_max);
    walk<BS, f32x4_t>(bs + wave, be, z_of, [&](uint32_t, int k, f32x4_t z) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sum[k] = sum[k] + sbm_exp(z[j] - m[k]);
    });
    RW::meet(sum, lds_sum, wave, lane, sbm_add);
    walk<BS, f32x4_t>(bs + wave, be, z_of, [&](uint32_t e, int k, f32x4_t z) {
        f32x4_t q;
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = sbm_exp(z[j] - m[k]) / sum[k];
        store_any<OUT_BF16>(out, at_of<BS>(e, k, lane), q);
    });
}

template <int BS, bool P_BF16, bool DS_BF16>
__global__ void __launch_bounds__(64 * kSbmWaves) softmax_bsr_bwd_kernel(uint32_t Mb, const uint32_t *__restrict__ blockRowPtrs,
                                                                          const void *__restrict__ p, const float *__restrict__ dp, float scale,
                                                                          void *__restrict__ ds) {
    using RW = Rows<BS>;
    constexpr int R = RW::R;
    constexpr int CB = kHeld<BS> / kSbmWaves;
    __shared__ float lds_dot[kSbmWaves][BS];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t Rb = blockIdx.x;
    if (Rb >= Mb) return;
    const uint32_t bs = blockRowPtrs[Rb], be = blockRowPtrs[Rb + 1];
    if (be <= bs) return;
    float dot[R];
#pragma unroll
    for (int k = 0; k < R; ++k) dot[k] = 0.f;
    // ds = scale * (p * (dp - dot)), each operation rounded
    auto result = [&](f32x4_t pv, f32x4_t dv, float d) {
        f32x4_t q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = dv[j] - d;
            const float u = pv[j] * t;
            q[j] = scale * u;
        }
        return q;
    };

    if (be - bs <= static_cast<uint32_t>(kHeld<BS>)) {
        // as in the forward: a block past the row's end reads the last one and takes part as p = dp = +0
        f32x4_t pv[CB][R], dv[CB][R];
#pragma unroll
        for (int b = 0; b < CB; ++b) {
            const uint32_t e = bs + wave + b * kSbmWaves;
            const bool there = e < be;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const size_t at = at_of<BS>(there ? e : be - 1, k, lane);
                const f32x4_t pl = load_any<P_BF16>(p, at), dl = load_f32(dp, at);
                pv[b][k] = there ? pl : f32x4_t{0.f, 0.f, 0.f, 0.f};
                dv[b][k] = there ? dl : f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int b = 0; b < CB; ++b)
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) dot[k] = __builtin_fmaf(pv[b][k][j], dv[b][k][j], dot[k]);
        RW::meet(dot, lds_dot, wave, lane, sbm_add);
#pragma unroll
        for (int b = 0; b < CB; ++b) {
            const uint32_t e = bs + wave + b * kSbmWaves;
            if (e < be) {
#pragma unroll
                for (int k = 0; k < R; ++k) store_any<DS_BF16>(ds, at_of<BS>(e, k, lane), result(pv[b][k], dv[b][k], dot[k]));
            }
        }
        return;
    }

    struct Pair {
        f32x4_t p, d;
    };
    auto load = [&](uint32_t e, int k) { return Pair{load_any<P_BF16>(p, at_of<BS>(e, k, lane)), load_f32(dp, at_of<BS>(e, k, lane))}; };
    walk<BS, Pair>(bs + wave, be, load, [&](uint32_t, int k, Pair v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) dot[k] = __builtin_fmaf(v.p[j], v.d[j], dot[k]);
    });
    RW::meet(dot, lds_dot, wave, lane, sbm_add);
    walk<BS, Pair>(bs + wave, be, load, [&](uint32_t e, int k, Pair v) { store_any<DS_BF16>(ds, at_of<BS>(e, k, lane), result(v.p, v.d, dot[k])); });
}

// `held`: numBlocks <= C, so no block row can be longer and every one is held in registers; `walk`: a block row of more
// than C blocks takes the three walks (the shorter ones of the same launch are still held).
template <int BS>
const char *path_tag(uint32_t numBlocks) { return numBlocks <= static_cast<uint32_t>(kHeld<BS>) ? "held" : "walk"; }

template <int BS, bool MASK, bool OUT_BF16>
void launch_fwd(hipStream_t stream, uint32_t Mb, uint32_t numBlocks, const uint32_t *blockRowPtrs, const float *scores, const float *mask,
                float scale, void *out) {
    note_kernel("softmax_bsr<b%d,%s,%s,C%d,%s>", BS, OUT_BF16 ? "bf16" : "f32", path_tag<BS>(numBlocks), kHeld<BS>, MASK ? "mask" : "nomask");
    hipLaunchKernelGGL((softmax_bsr_kernel<BS, MASK, OUT_BF16>), dim3(Mb), dim3(64 * kSbmWaves), 0, stream, Mb, blockRowPtrs, scores, mask,
                       scale, out);
}

template <int BS, bool P_BF16, bool DS_BF16>
void launch_bwd(hipStream_t stream, uint32_t Mb, uint32_t numBlocks, const uint32_t *blockRowPtrs, const void *p, const float *dp,
                float scale, void *ds) {
    note_kernel("softmax_bsr_bwd<b%d,%s,%s,C%d,p_%s>", BS, DS_BF16 ? "bf16" : "f32", path_tag<BS>(numBlocks), kHeld<BS>, P_BF16 ? "bf16" : "f32");
    hipLaunchKernelGGL((softmax_bsr_bwd_kernel<BS, P_BF16, DS_BF16>), dim3(Mb), dim3(64 * kSbmWaves), 0, stream, Mb, blockRowPtrs, p, dp, scale,
                       ds);
}

// what both entry points check, before any device work
int check_common(const char *name, uint32_t bS, float scale) {
    if (!(scale > 0.f) || scale == __builtin_huge_valf())
        return fail(MISPMM_ERR_INVALID_ARG, "%s: scale must be finite and > 0 (got %g)", name, static_cast<double>(scale));
    if (bS != 16 && bS != 32) return fail(MISPMM_ERR_UNSUPPORTED, "%s: only 16x16 or 32x32 blocks (got bS=%u)", name, bS);
    return MISPMM_OK;
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_softmax_bsr_f32(mispmm_stream_t stream, uint32_t numBlockRows, uint32_t bS, uint32_t numBlocks,
                                      const uint32_t *blockRowPtrs, const float *scores, const float *mask, float scale, void *out,
                                      int out_bf16) {
    if (const int st = check_common("softmax_bsr_f32", bS, scale)) return st;
    if (numBlockRows == 0 || numBlocks == 0) return MISPMM_OK;
    if (!blockRowPtrs || !scores || !out) return fail(MISPMM_ERR_INVALID_ARG, "softmax_bsr_f32: blockRowPtrs, scores or out is null");
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_flag(mask != nullptr, [&](auto m) {
            with_flag(out_bf16 != 0, [&](auto o) {
                launch_fwd<decltype(bs)::value, decltype(m)::value, decltype(o)::value>(as_stream(stream), numBlockRows, numBlocks, blockRowPtrs,
                                                                                        scores, mask, scale, out);
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}

extern "C" int mispmm_softmax_bsr_bwd_f32(mispmm_stream_t stream, uint32_t numBlockRows, uint32_t bS, uint32_t numBlocks,
                                          const uint32_t *blockRowPtrs, const void *p, int p_bf16, const float *dp, float scale, void *ds,
                                          int ds_bf16) {
    if (const int st = check_common("softmax_bsr_bwd_f32", bS, scale)) return st;
    if (numBlockRows == 0 || numBlocks == 0) return MISPMM_OK;
    if (!blockRowPtrs || !p || !dp || !ds) return fail(MISPMM_ERR_INVALID_ARG, "softmax_bsr_bwd_f32: blockRowPtrs, p, dp or ds is null");
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_flag(p_bf16 != 0, [&](auto pb) {
            with_flag(ds_bf16 != 0, [&](auto db) {
                launch_bwd<decltype(bs)::value, decltype(pb)::value, decltype(db)::value>(as_stream(stream), numBlockRows, numBlocks, blockRowPtrs, p,
                                                                                          dp, scale, ds);
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
