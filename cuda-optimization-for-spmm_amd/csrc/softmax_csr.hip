// Row softmax on a CSR pattern and its backward (mispmm.h, section "Row softmax on a CSR pattern"):
//   forward   out[e] = exp(s[e] - m_r) / sum_{e' in row r} exp(s[e'] - m_r),   m_r the largest score of row r
//   backward  ds[e]  = p[e] * (dp[e] - sum_{e' in row r} p[e'] * dp[e'])
// Column indices and A's values are not read: the row pointers alone say which entries belong together.
//
// Shape: G lanes own one row (G = 4 .. 64, picked on the host from nnz / M), lane l of the group holds entries l, l + G,
// l + 2 G, ... of it, so a group's loads and stores are G consecutive elements.  A row of up to kSmRegs * G entries is read
// ONCE into registers, reduced and written from them (2 elem bytes of traffic per entry, the floor).  A longer row is left
// to the WHOLE WAVE: once its groups are through their short rows, the wave takes the long ones in turn, 64 lanes on each --
// from registers again up to kSmRegs * 64 = 256 entries, beyond that in three walks (max, sum, write; backward: sum, write)
// of 256 entries a step, the re-reads served by L1 / L2 and the exponentials computed twice, to the same bits.  Either way
// a lane sums its entries in ascending order and the lanes' partial results meet in a butterfly of xor moves
// (lane_moves.hpp), so the order of every sum is fixed by (row length, G) alone: run to run identical.  One launch, no
// atomics, no LDS, no scratch.
//
// In place (out == scores, ds == dp): an element is written by the lane that read it, after every read of the row that
// any lane needs for the sums has returned -- the written value depends on the row-wide sum -- and in the walks a step's
// loads precede its stores.  The pointers are therefore NOT __restrict__.
//
// Special values need no branch.  fmax drops a NaN operand, so m_r is the largest non-NaN score (-Inf if there is none)
// and the NaN is carried by the sum instead: NaN - m_r = NaN, exp(NaN) = NaN, and a NaN term makes the sum and with it every
// quotient of the row NaN.  m_r = +Inf gives Inf - Inf = NaN for that entry, m_r = -Inf (nothing but -Inf) gives
// -Inf - -Inf = NaN for every entry: the same.  A -Inf beside a finite score is exp(-Inf) = +0, and +0 / sum = +0.
#include "lane_moves.hpp"

namespace mispmm {

namespace {

constexpr int kSmBlock = 256;  // threads per workgroup
constexpr int kSmRegs = 4;     // entries per lane a row may have and still be handled from registers

// The arithmetics.  T: element type in memory, A: the type everything is computed in.
struct SmF32Ref {  // fp64 inside, rounded to fp32 once
    using T = float; using A = double;
    static constexpr const char *tag = "f32,ref64";
    static __device__ __forceinline__ A exp_(A t) { return exp(t); }
    // the fp32 x fp32 product is exact in fp64: the fused form rounds once, at the add, as mul + add would
    static __device__ __forceinline__ A mac(A acc, A x, A y) { return __builtin_fma(x, y, acc); }
};
struct SmF32Fast {  // fp32 throughout, exp as v_exp_f32 of t * log2(e)
    using T = float; using A = float;
    static constexpr const char *tag = "f32,fast";
    static __device__ __forceinline__ A exp_(A t) { return __builtin_amdgcn_exp2f(t * 1.44269504088896340736f); }
    static __device__ __forceinline__ A mac(A acc, A x, A y) { return __builtin_fmaf(x, y, acc); }
};
struct SmF64Ref {  // -ffp-contract=off keeps the product and the add apart
    using T = double; using A = double;
    static constexpr const char *tag = "f64,ref";
    static __device__ __forceinline__ A exp_(A t) { return exp(t); }
    static __device__ __forceinline__ A mac(A acc, A x, A y) {
        const double p = x * y;
        return acc + p;
    }
};
struct SmF64Fast {
    using T = double; using A = double;
    static constexpr const char *tag = "f64,fast";
    static __device__ __forceinline__ A exp_(A t) { return exp(t); }
    static __device__ __forceinline__ A mac(A acc, A x, A y) { return __builtin_fma(x, y, acc); }
};

template <class A> __device__ __forceinline__ A sm_max(A a, A b) {
    if constexpr (sizeof(A) == 4) return __builtin_fmaxf(a, b); else return __builtin_fmax(a, b);
}
template <class A> __device__ __forceinline__ A sm_add(A a, A b) { return a + b; }

// One row by W lanes (W = G: the lane's group; W = 64: the whole wave), lane l of them holding entries l, l + W, ...: from
// registers if the row fits kSmRegs per lane, else in three walks of kSmRegs entries per lane and step -- the loads of a
// step are issued together, before anything of the step is stored (the arrays may be one).
template <class P, int W>
__device__ __forceinline__ void sm_forward_row(const typename P::T *s, typename P::T *o, uint32_t len, uint32_t lane) {
    using T = typename P::T;
    using A = typename P::A;
    const A ninf = -__builtin_huge_val();
    if (len <= static_cast<uint32_t>(kSmRegs * W)) {
        A t[kSmRegs];
        A m = ninf;
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) {
            const uint32_t i = lane + j * W;
            t[j] = i < len ? static_cast<A>(s[i]) : ninf;
            m = sm_max(m, t[j]);
        }
        m = group_all_reduce<W>(m, sm_max<A>);
        A sum = A(0);
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) {
            const uint32_t i = lane + j * W;
            t[j] = i < len ? P::exp_(t[j] - m) : A(0);  // a slot past the row end adds +0
            sum = sum + t[j];
        }
        sum = group_all_reduce<W>(sum, sm_add<A>);
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) {
            const uint32_t i = lane + j * W;
            if (i < len) o[i] = static_cast<T>(t[j] / sum);
        }
        return;
    }
    A m = ninf;
    for (size_t i0 = lane; i0 < len; i0 += kSmRegs * W) {  // 64-bit: a row may end near 2^32
        A t[kSmRegs];
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) t[j] = i0 + j * W < len ? static_cast<A>(s[i0 + j * W]) : ninf;
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) m = sm_max(m, t[j]);
    }
    m = group_all_reduce<W>(m, sm_max<A>);
    A sum = A(0);
    for (size_t i0 = lane; i0 < len; i0 += kSmRegs * W) {  // 64-bit: a row may end near 2^32
        A t[kSmRegs];
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) t[j] = i0 + j * W < len ? static_cast<A>(s[i0 + j * W]) : ninf;
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) sum = sum + (i0 + j * W < len ? P::exp_(t[j] - m) : A(0));
    }
    sum = group_all_reduce<W>(sum, sm_add<A>);
    for (size_t i0 = lane; i0 < len; i0 += kSmRegs * W) {  // 64-bit: a row may end near 2^32
        A t[kSmRegs];
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) t[j] = i0 + j * W < len ? static_cast<A>(s[i0 + j * W]) : ninf;
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j)
            if (i0 + j * W < len) o[i0 + j * W] = static_cast<T>(P::exp_(t[j] - m) / sum);
    }
}

template <class P, int W>
__device__ __forceinline__ void sm_backward_row(const typename P::T *pr, const typename P::T *dr, typename P::T *o, uint32_t len,
                                                uint32_t lane) {
    using T = typename P::T;
    using A = typename P::A;
    if (len <= static_cast<uint32_t>(kSmRegs * W)) {
        A pv[kSmRegs], dv[kSmRegs];
        A dot = A(0);
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) {
            const uint32_t i = lane + j * W;
            pv[j] = i < len ? static_cast<A>(pr[i]) : A(0);  // a slot past the row end adds 0 * 0 = +0
            dv[j] = i < len ? static_cast<A>(dr[i]) : A(0);
            dot = P::mac(dot, pv[j], dv[j]);
        }
        dot = group_all_reduce<W>(dot, sm_add<A>);
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) {
            const uint32_t i = lane + j * W;
            const A d = dv[j] - dot;
            if (i < len) o[i] = static_cast<T>(pv[j] * d);
        }
        return;
    }
    A dot = A(0);
    for (size_t i0 = lane; i0 < len; i0 += kSmRegs * W) {  // 64-bit: a row may end near 2^32
        A pv[kSmRegs], dv[kSmRegs];
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) {
            pv[j] = i0 + j * W < len ? static_cast<A>(pr[i0 + j * W]) : A(0);
            dv[j] = i0 + j * W < len ? static_cast<A>(dr[i0 + j * W]) : A(0);
        }
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) dot = P::mac(dot, pv[j], dv[j]);
    }
    dot = group_all_reduce<W>(dot, sm_add<A>);
    for (size_t i0 = lane; i0 < len; i0 += kSmRegs * W) {  // 64-bit: a row may end near 2^32
        A pv[kSmRegs], dv[kSmRegs];
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) {
            pv[j] = i0 + j * W < len ? static_cast<A>(pr[i0 + j * W]) : A(0);
            dv[j] = i0 + j * W < len ? static_cast<A>(dr[i0 + j * W]) : A(0);
        }
#pragma unroll
        for (int j = 0; j < kSmRegs; ++j) {
            const A d = dv[j] - dot;
            if (i0 + j * W < len) o[i0 + j * W] = static_cast<T>(pv[j] * d);
        }
    }
}

// The rows of a wave: each of its 64 / G groups does its own row if that fits the group's registers; then the wave goes
// through the rows that do not, one after the other, all 64 lanes on each (start and length of a row reach the wave through
// a readlane of the group's first lane).  No lane leaves before the end, so every lane a move reads from is there.
// BWD: a = p, b = dp; else a = scores.
template <class P, int G, bool BWD>
__device__ __forceinline__ void sm_rows(uint32_t M, const uint32_t *__restrict__ rowPtrs, const typename P::T *a, const typename P::T *b,
                                        typename P::T *out) {
    const uint64_t row = static_cast<uint64_t>(blockIdx.x) * (kSmBlock / G) + threadIdx.x / G;
    uint32_t base = 0, len = 0;
    if (row < M) {
        base = rowPtrs[row];
        len = rowPtrs[row + 1] - base;
    }
    constexpr uint32_t FITS = kSmRegs * G;
    if constexpr (G < kWave) {
        if (len != 0 && len <= FITS) {  // all G lanes of a group agree
            if constexpr (BWD) sm_backward_row<P, G>(a + base, b + base, out + base, len, threadIdx.x % G);
            else sm_forward_row<P, G>(a + base, out + base, len, threadIdx.x % G);
        }
    }
    if constexpr (G < kWave) {
        if (__ballot(len > FITS) == 0) return;  // the whole wave agrees
    }
    const uint32_t wlane = threadIdx.x % kWave;
    static_for<0, kWave / G>([&](auto g_tag) {
        constexpr int src = decltype(g_tag)::value * G;
        const uint32_t wlen = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(len), src));
        if (G == kWave ? wlen != 0 : wlen > FITS) {  // wave-uniform
            const size_t wbase = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(base), src));
            if constexpr (BWD) sm_backward_row<P, kWave>(a + wbase, b + wbase, out + wbase, wlen, wlane);
            else sm_forward_row<P, kWave>(a + wbase, out + wbase, wlen, wlane);
        }
    });
}

template <class P, int G>
__global__ void __launch_bounds__(kSmBlock) softmax_csr_kernel(uint32_t M, const uint32_t *__restrict__ rowPtrs, const typename P::T *scores,
                                                               typename P::T *out) {
    sm_rows<P, G, false>(M, rowPtrs, scores, nullptr, out);
}

template <class P, int G>
__global__ void __launch_bounds__(kSmBlock) softmax_csr_bwd_kernel(uint32_t M, const uint32_t *__restrict__ rowPtrs, const typename P::T *p,
                                                                   const typename P::T *dp, typename P::T *ds) {
    sm_rows<P, G, true>(M, rowPtrs, p, dp, ds);
}

// lanes per row: the smallest group whose registers hold the mean row
inline int sm_pick_group(uint32_t M, uint32_t nnz) {
    const uint32_t mean = ceil_div(nnz, M);
    int g = 4;
    while (g < kWave && static_cast<uint32_t>(g * kSmRegs) < mean) g <<= 1;
    return g;
}

template <class P, int G>
void launch_softmax(hipStream_t stream, uint32_t M, const uint32_t *rowPtrs, const typename P::T *a, const typename P::T *b,
                    typename P::T *out, bool bwd) {
    const uint32_t grid = ceil_div(M, static_cast<uint32_t>(kSmBlock / G));
    if (bwd) {
        note_kernel("softmax_csr_bwd<%s,G%d,R%d>", P::tag, G, kSmRegs);
        hipLaunchKernelGGL((softmax_csr_bwd_kernel<P, G>), dim3(grid), dim3(kSmBlock), 0, stream, M, rowPtrs, a, b, out);
    } else {
        note_kernel("softmax_csr<%s,G%d,R%d>", P::tag, G, kSmRegs);
        hipLaunchKernelGGL((softmax_csr_kernel<P, G>), dim3(grid), dim3(kSmBlock), 0, stream, M, rowPtrs, a, out);
    }
}

// forward: a = scores, b unused; backward: a = p, b = dp.  The kernels address through 64-bit pointers, so no array size
// is declined.
template <class PRef, class PFast>
int softmax_csr(const char *name, bool bwd, mispmm_stream_t stream, uint32_t M, uint32_t nnz, const uint32_t *rowPtrs,
                const typename PRef::T *a, const typename PRef::T *b, typename PRef::T *out, int acc_mode) {
    if (int s = check_acc_mode(name, acc_mode)) return s;
    if (M == 0 || nnz == 0) return MISPMM_OK;
    if (!rowPtrs || !a || (bwd && !b) || !out)
        return fail(MISPMM_ERR_INVALID_ARG, bwd ? "%s: rowPtrs, p, dp or ds is null" : "%s: rowPtrs, scores or out is null", name);
    with_acc<PRef, PFast>(acc_mode, [&](auto acc) {
        with_const<4, 8, 16, 32, 64>(sm_pick_group(M, nnz), [&](auto g) {
            launch_softmax<typename decltype(acc)::type, decltype(g)::value>(as_stream(stream), M, rowPtrs, a, b, out, bwd);
        });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_softmax_csr_f32(mispmm_stream_t stream, uint32_t M, uint32_t nnz, const uint32_t *rowPtrs, const float *scores,
                                      float *out, int acc_mode) {
    return softmax_csr<SmF32Ref, SmF32Fast>("softmax_csr_f32", false, stream, M, nnz, rowPtrs, scores, nullptr, out, acc_mode);
}

extern "C" int mispmm_softmax_csr_f64(mispmm_stream_t stream, uint32_t M, uint32_t nnz, const uint32_t *rowPtrs, const double *scores,
                                      double *out, int acc_mode) {
    return softmax_csr<SmF64Ref, SmF64Fast>("softmax_csr_f64", false, stream, M, nnz, rowPtrs, scores, nullptr, out, acc_mode);
}

extern "C" int mispmm_softmax_csr_bwd_f32(mispmm_stream_t stream, uint32_t M, uint32_t nnz, const uint32_t *rowPtrs, const float *p,
                                          const float *dp, float *ds, int acc_mode) {
    return softmax_csr<SmF32Ref, SmF32Fast>("softmax_csr_bwd_f32", true, stream, M, nnz, rowPtrs, p, dp, ds, acc_mode);
}

extern "C" int mispmm_softmax_csr_bwd_f64(mispmm_stream_t stream, uint32_t M, uint32_t nnz, const uint32_t *rowPtrs, const double *p,
                                          const double *dp, double *ds, int acc_mode) {
    return softmax_csr<SmF64Ref, SmF64Fast>("softmax_csr_bwd_f64", true, stream, M, nnz, rowPtrs, p, dp, ds, acc_mode);
}
