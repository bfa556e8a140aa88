// The fp64 row-gather kernel (mispmm_csr_f64): G lanes own one C row, each lane owns VEC consecutive doubles of it (VEC = 2:
// one 16-byte buffer_load_dwordx4 per B row), lane i fetches entry i of the row's current G-entry chunk and the group takes
// (B-row offset, coefficient) from it by ds_bpermute, 8 B-row reads are kept in flight per lane and refilled one by one as
// they are consumed, products are summed in list order, C leaves through non-temporal buffer stores.  Workgroups are laid
// over the 8 XCDs as a P x Q grid of (row part, column part), as the fp32 row-gather kernel does (row_gather.hpp).
// A separate kernel on purpose: templating the fp32 one on the value type would touch its tuned instruction streams.
#pragma once
#include <type_traits>

#include "spmm_common.hpp"

namespace mispmm {

using f64x2 = double __attribute__((ext_vector_type(2)));

template <int VEC> struct VecOf64;
template <> struct VecOf64<1> { using type = double; };
template <> struct VecOf64<2> { using type = f64x2; };

// REFERENCE: the fp64 product rounded once, then the add rounded once, in list order -- the arithmetic every CPU function
// of the reference reduces to with DT = double (-ffp-contract=off keeps the two apart).
struct Acc64Ref {
    static __device__ __forceinline__ double mac(double acc, double a, double b) {
        const double p = a * b;
        return acc + p;
    }
};
// FAST: one fused multiply-add per term, same order.
struct Acc64Fast {
    static __device__ __forceinline__ double mac(double acc, double a, double b) { return __builtin_fma(a, b, acc); }
};

template <int VEC>
__device__ __forceinline__ typename VecOf64<VEC>::type buffer_load_f64(rsrc_t rsrc, uint32_t voffset) {
    if constexpr (VEC == 1) return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voffset, 0, 0));
    else return __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, 0, 0));
}
template <int VEC>
__device__ __forceinline__ void buffer_store_f64_c(rsrc_t rsrc, uint32_t voffset, typename VecOf64<VEC>::type v) {
    using u2 = uint32_t __attribute__((ext_vector_type(2)));
    using u4 = uint32_t __attribute__((ext_vector_type(4)));
    if constexpr (VEC == 1) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), rsrc, voffset, 0, kCStoreAux);
    else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), rsrc, voffset, 0, kCStoreAux);
}
template <int VEC> __device__ __forceinline__ double vec64_get(const typename VecOf64<VEC>::type &v, int i) {
    if constexpr (VEC == 1) return v; else return v[i];
}

constexpr int kF64Block = 128;   // threads per workgroup
constexpr int kF64InFlight = 8;  // B-row reads in flight per lane

// WIDE: B or C spans 2 GiB or more, beyond what a raw buffer descriptor addresses -- 64-bit addresses, plain loads and stores.
template <int G, int VEC, class Acc, bool WIDE>
__global__ void __launch_bounds__(kF64Block) csr_f64_kernel(uint32_t M, uint32_t rb_chunk, uint32_t log2p, uint32_t cols_per_part,
                                                            uint32_t N, uint32_t ldb, const uint32_t *__restrict__ rowPtrs,
                                                            const uint32_t *__restrict__ colIdxs, const double *__restrict__ vals,
                                                            const double *__restrict__ B, uint32_t b_bytes, double *__restrict__ C,
                                                            uint32_t c_bytes, uint32_t ldc) {
    static_assert(G >= kF64InFlight && (G & (G - 1)) == 0, "a block of in-flight slots must lie inside one chunk");
    constexpr int GROUPS = kF64Block / G, R = kF64InFlight;
    using vec_t = typename VecOf64<VEC>::type;
    const uint32_t lane = threadIdx.x % G;
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const uint32_t p = xcd & ((1u << log2p) - 1u), q = xcd >> log2p;
    const uint32_t row = (p * rb_chunk + slot) * GROUPS + threadIdx.x / G;
    const bool row_ok = row < M;
    const uint32_t col0 = q * cols_per_part + blockIdx.y * (G * VEC) + lane * VEC;
    const bool col_ok = col0 < min(N, (q + 1) * cols_per_part);
    // all lanes of a group share the row, hence the trip count below: a group is never split by the loop
    uint32_t base = 0, len = 0;
    if (row_ok) {
        base = rowPtrs[row];
        len = rowPtrs[row + 1] - base;
    }
    double acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0;

    const rsrc_t rsrc = make_rsrc(B, b_bytes);
    const uint32_t lane_off = col_ok ? col0 * 8u : kDropLoad;  // lanes past the column part never fetch
    const uint32_t ldb8 = ldb * 8u;
    // entry c0 + lane of the row, RAW: the loads are issued and nothing uses their values until the chunk opens, so the
    // prefetch of the next chunk does not make the wave wait for it at once.  Nothing past the row is read (len > 0 here:
    // entry `base` exists).
    auto fetch_raw = [&](uint32_t c0, uint32_t &col, double &val) {
        const uint32_t idx = c0 + lane;
        const size_t e = static_cast<size_t>(base) + (idx < len ? idx : 0u);
        col = colIdxs[e];
        val = vals[e];
    };
    // ... made usable when its chunk opens: key = B-row byte offset (buffer body) or column (WIDE body); an entry past the
    // row end gets key kDropLoad / 0xFFFFFFFF and coefficient 0
    auto to_key = [&](uint32_t c0, uint32_t col, double &val) {
        const bool live = c0 + lane < len;
        val = live ? val : 0.0;
        if constexpr (WIDE) return live ? col : 0xFFFFFFFFu;
        else return live ? col * ldb8 : kDropLoad;
    };
    vec_t bv[R];
    double av[R];
    bool wlive[R];  // WIDE only: the slot reads a real B row (a dead slot reads row 0 and is zeroed where it is consumed)
    // slot s of the row into ring position r: the owning lane's entry to the group, then the B read.  A dead slot yields
    // b = 0, a = 0: it adds 0 * 0 = +0 to a sum that started at +0 and is never -0 -- an exact no-op.
    auto issue = [&](auto r_tag, uint32_t s, uint32_t my_key, double my_val) {
        constexpr int r = decltype(r_tag)::value;
        const int src = static_cast<int>(s & (G - 1));
        const uint32_t key = static_cast<uint32_t>(__shfl(static_cast<int>(my_key), src, G));
        av[r] = __shfl(my_val, src, G);
        if constexpr (WIDE) {
            // the select on the loaded value waits for it: it is made in consume(), not here
            wlive[r] = key != 0xFFFFFFFFu;
            bv[r] = *reinterpret_cast<const vec_t *>(B + static_cast<size_t>(wlive[r] ? key : 0u) * ldb + (col_ok ? col0 : 0u));
        } else {
            // a dead key (bit 31) stays out of range after the lane offset is added, so the load returns zeros; in a
            // column-masked lane the sum wraps to an in-range read of a lane that never stores
            bv[r] = buffer_load_f64<VEC>(rsrc, key + lane_off);
        }
    };
    auto consume = [&](auto r_tag) {
        constexpr int r = decltype(r_tag)::value;
        vec_t b = bv[r];
        if constexpr (WIDE) b = wlive[r] ? b : vec_t{};
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = Acc::mac(acc[v], av[r], vec64_get<VEC>(b, v));
    };
    // the refill of a ring position may not be hoisted above the consume that frees it, nor sunk below the next ones: an
    // empty asm that "rewrites" the sums and clobbers memory sits between them, fenced by scheduling barriers (as in
    // row_gather.hpp: sched_barrier alone does not order the side-effect-free arithmetic at instruction selection)
    auto pin = [&] {
        if constexpr (VEC == 2) asm volatile("" : "+v"(acc[0]), "+v"(acc[1]) : : "memory");
        else asm volatile("" : "+v"(acc[0]) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    if (len != 0) {
        uint32_t cur_col, nxt_col;
        double cur_val, nxt_val;
        fetch_raw(0, cur_col, cur_val);
        uint32_t cur_key = to_key(0, cur_col, cur_val);
        fetch_raw(G, nxt_col, nxt_val);  // the next chunk's entries are on their way while this one is gathered
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, R>([&](auto r) { issue(r, decltype(r)::value, cur_key, cur_val); });
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t nblk = (len + R - 1) / R;
        for (uint32_t b = 1; b < nblk; ++b) {
            const uint32_t s0 = b * R;
            if ((s0 & (G - 1)) == 0) {  // block b opens a new chunk (the ring already holds its own copies of the old one)
                // NB: the compiler waits for these entries with vmcnt(0)-(1) here, which also drains the B reads in flight
                // (vmcnt counts in order): once per G slots, so only rows longer than G entries pay it
                cur_val = nxt_val;
                cur_key = to_key(s0, nxt_col, cur_val);
                fetch_raw(s0 + G, nxt_col, nxt_val);
            }
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, R>([&](auto r) {
                consume(r);
                pin();
                issue(r, s0 + decltype(r)::value, cur_key, cur_val);
                __builtin_amdgcn_sched_barrier(0);
            });
        }
        static_for<0, R>([&](auto r) { consume(r); });
    }
    if (row_ok && col_ok) {
        vec_t out;
        if constexpr (VEC == 1) out = acc[0];
        else out = vec_t{acc[0], acc[1]};
        const size_t at = static_cast<size_t>(row) * ldc + col0;
        if constexpr (WIDE) *reinterpret_cast<vec_t *>(C + at) = out;
        else buffer_store_f64_c<VEC>(make_rsrc(C, c_bytes), static_cast<uint32_t>(at * 8u), out);
    }
}

}  // namespace mispmm
