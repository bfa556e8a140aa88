// libmispmm_bf16.so: C = A @ B over a row list (rowPtrs, colIdxs, vals) with A's values in fp32 and B in bf16
// (include/mispmm_bf16.h).  One kernel in the shape of csrc/row_gather_f64.hpp for another element width: G lanes own one
// C row, a lane owns V consecutive columns of it (V8: one 16-byte buffer load per B row, V4: 8 bytes, V1: 2 bytes), lane i
// fetches entry i of the row's current G-entry chunk and the group takes (B-row offset, coefficient) from it by
// ds_bpermute, 8 B-row reads are kept in flight per lane and refilled one by one as they are consumed, the products are
// summed in list order, C leaves through non-temporal buffer stores.  Workgroups go over the 8 XCDs by xcd_grid as 8 row
// parts x 1: a B row of N = 128 is two 128-byte lines, so a column split would hand each XCD lines it shares with no one
// while every XCD still walked the whole index list.
// The sources lie outside csrc/ and fused/: the census tests hold those directories and their libraries to their records.
#include <type_traits>

#include "mispmm_bf16.h"
#include "bf16_lanes.hpp"

namespace mispmm {

namespace {

// one rounding to nearest even, a NaN stays a NaN: v_cvt_pk_bf16_f32, the instruction of mispmm_f32_to_bf16
__device__ __forceinline__ uint32_t bf16_bits(float x) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(x)); }
__device__ __forceinline__ uint32_t bf16_pair(float lo, float hi) { return bf16_bits(lo) | (bf16_bits(hi) << 16); }

constexpr int kRowsBlock = 128;   // threads per workgroup
constexpr int kRowsInFlight = 8;  // B-row reads in flight per lane

template <int G, int V, class Acc>
__global__ void __launch_bounds__(kRowsBlock) rows_bf16_kernel(uint32_t M, uint32_t xcd_chunk, uint32_t N, uint32_t ldb, uint32_t rowNnz,
                                                               uint32_t out_bf16, uint32_t ldc, uint32_t b_bytes, uint32_t c_bytes,
                                                               const uint32_t *__restrict__ rowPtrs, const uint32_t *__restrict__ colIdxs,
                                                               const float *__restrict__ vals, const uint16_t *__restrict__ B,
                                                               void *__restrict__ C) {
    static_assert(G >= kRowsInFlight && (G & (G - 1)) == 0, "a block of in-flight slots must lie inside one chunk");
    static_assert(V == 8 || V == 4 || V == 1);
    constexpr int GROUPS = kRowsBlock / G, R = kRowsInFlight;
    using raw_t = typename RawOf<V>::type;
    using acc_t = typename Acc::T;
    const uint32_t lane = threadIdx.x % G;
    const uint32_t row = xcd_block(blockIdx.x, xcd_chunk) * GROUPS + threadIdx.x / G;
    const bool row_ok = row < M;
    const uint32_t col0 = blockIdx.y * (G * V) + lane * V;
    const bool col_ok = col0 < N;  // N is a multiple of V: a lane's columns lie inside N or past it together
    // all lanes of a group share the row, hence the trip count below: a group is never split by the loop
    uint32_t base = 0, len = 0;
    if (row_ok) {
        if (rowPtrs) {
            base = rowPtrs[row];
            len = rowPtrs[row + 1] - base;
        } else {  // the uniform list: no row-pointer fetch (a wave-uniform branch)
            base = row * rowNnz;
            len = rowNnz;
        }
    }
    acc_t acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0;

    const rsrc_t rsrc = make_rsrc(B, b_bytes);
    const uint32_t lane_off = col_ok ? col0 * 2u : kDropLoad;  // lanes past N never fetch
    const uint32_t ldb2 = ldb * 2u;
    // entry c0 + lane of the row, RAW: the loads are issued and nothing uses their values until the chunk opens, so the
    // prefetch of the next chunk does not make the wave wait for it at once.  Nothing past the row is read (len > 0 here:
    // entry `base` exists).
    auto fetch_raw = [&](uint32_t c0, uint32_t &col, float &val) {
        const uint32_t idx = c0 + lane;
        const size_t e = static_cast<size_t>(base) + (idx < len ? idx : 0u);
        col = colIdxs[e];
        val = vals[e];
    };
    // ... made usable when its chunk opens: key = B-row byte offset.  An entry past the row end and a padding slot (column
    // 0xFFFFFFFF) get key kDropLoad AND coefficient 0: the load is dropped and returns 0, and 0 * 0 = +0 whatever the
    // slot's value held (an Inf times the dropped load's 0 would be a NaN)
    auto to_key = [&](uint32_t c0, uint32_t col, float &val) {
        const bool live = c0 + lane < len && col != 0xFFFFFFFFu;
        val = live ? val : 0.0f;
        return live ? col * ldb2 : kDropLoad;
    };
    raw_t bv[R];
    float av[R];
    // slot s of the row into ring position r: the owning lane's entry to the group, then the B read.  A dead slot yields
    // b = 0, a = 0: it adds 0 * 0 = +0
    auto issue = [&](auto r_tag, uint32_t s, uint32_t my_key, float my_val) {
        constexpr int r = decltype(r_tag)::value;
        const int src = static_cast<int>(s & (G - 1));
        const uint32_t key = static_cast<uint32_t>(__shfl(static_cast<int>(my_key), src, G));
        av[r] = __shfl(my_val, src, G);
        // a dead key (bit 31) stays out of range after the lane offset is added, so the load returns zeros; in a
        // column-masked lane the sum wraps to an in-range read of a lane that never stores
        bv[r] = buffer_load_bf16<V>(rsrc, key + lane_off);
    };
    auto consume = [&](auto r_tag) {
        constexpr int r = decltype(r_tag)::value;
        const raw_t b = bv[r];
#pragma unroll
        for (int v = 0; v < V; ++v) Acc::mac(acc[v], av[r], widen<V>(b, v));
    };
    // the refill of a ring position may not be hoisted above the consume that frees it, nor sunk below the next ones: an
    // empty asm that "rewrites" the sums and clobbers memory sits between them, fenced by scheduling barriers (as in
    // row_gather_f64.hpp: sched_barrier alone does not order the side-effect-free arithmetic at instruction selection)
    auto pin = [&] {
#pragma unroll
        for (int v = 0; v < V; ++v) asm volatile("" : "+v"(acc[v]) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    if (len != 0) {
        uint32_t cur_col, nxt_col;
        float cur_val, nxt_val;
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
                // (the vector-memory counter counts in order): once per G slots, so only rows longer than G entries pay it
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
        // chain + (+0): what the dead slots at a row's end add anyway, made the rule for every row length
        float out[V];
#pragma unroll
        for (int v = 0; v < V; ++v) out[v] = Acc::finish(acc[v]) + 0.0f;
        const rsrc_t crsrc = make_rsrc(C, c_bytes);
        const uint32_t at = row * ldc + col0;  // elements; the bytes stay below 2 GiB (checked by the caller)
        if (out_bf16) {  // wave-uniform
            if constexpr (V == 1) {
                __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(bf16_bits(out[0])), crsrc, at * 2u, 0, kCStoreAux);
            } else if constexpr (V == 4) {
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{bf16_pair(out[0], out[1]), bf16_pair(out[2], out[3])}, crsrc, at * 2u, 0, kCStoreAux);
            } else {
                __builtin_amdgcn_raw_buffer_store_b128(
                    u32x4{bf16_pair(out[0], out[1]), bf16_pair(out[2], out[3]), bf16_pair(out[4], out[5]), bf16_pair(out[6], out[7])}, crsrc,
                    at * 2u, 0, kCStoreAux);
            }
        } else {
            if constexpr (V == 1) {
                buffer_store_vec_c<1>(crsrc, at * 4u, out[0]);
            } else if constexpr (V == 4) {
                buffer_store_vec_c<2>(crsrc, at * 4u, f32x2{out[0], out[1]});
                buffer_store_vec_c<2>(crsrc, at * 4u + 8u, f32x2{out[2], out[3]});
            } else {
                buffer_store_vec_c<4>(crsrc, at * 4u, f32x4{out[0], out[1], out[2], out[3]});
                buffer_store_vec_c<4>(crsrc, at * 4u + 16u, f32x4{out[4], out[5], out[6], out[7]});
            }
        }
    }
}

struct RowsArgs {
    hipStream_t stream;
    uint32_t M, K, rowNnz;
    const uint32_t *rowPtrs, *colIdxs;
    const float *vals;
    const uint16_t *B;
    uint32_t N, ldb;
    void *C;
    uint32_t ldc;
    bool out_bf16;
};

inline bool aligned_to(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// the widest lane the operands allow (mispmm_bf16.h, LANE WIDTHS)
int pick_vec_bf16(const RowsArgs &a) {
    if (a.N % 8 == 0 && a.ldb % 8 == 0 && aligned16(a.B) && aligned16(a.C) && a.ldc % (a.out_bf16 ? 8 : 4) == 0) return 8;
    if (a.N % 4 == 0 && a.ldb % 4 == 0 && aligned8(a.B) && aligned8(a.C) && a.ldc % (a.out_bf16 ? 4 : 2) == 0) return 4;
    return 1;
}

// bytes from the first element of a [rows][ld] operand to the end of its last row's `width` columns
uint32_t span_bytes(uint64_t rows, uint32_t ld, uint32_t width, uint32_t elem_bytes) {
    return static_cast<uint32_t>(((rows - 1) * ld + width) * elem_bytes);
}

template <int G, int V, class Acc>
void launch_rows(const RowsArgs &a) {
    const XcdGrid xg = xcd_grid(ceil_div(a.M, static_cast<uint32_t>(kRowsBlock / G)));
    const dim3 grid(xg.grid, ceil_div(a.N, static_cast<uint32_t>(G * V)));
    // both below 2 GiB (checked by the caller); K >= 1 is not: B is not read where no entry names a row of it
    const uint32_t b_bytes = a.K == 0 ? 0u : span_bytes(a.K, a.ldb, a.N, 2u);
    const uint32_t c_bytes = span_bytes(a.M, a.ldc, a.N, a.out_bf16 ? 2u : 4u);
    note_kernel("rows_bf16<G%d,V%d,%s> %s xcd %ux1", G, V, acc_tag<Acc>(), a.out_bf16 ? "bf16" : "f32", xg.chunk ? 8u : 1u);
    hipLaunchKernelGGL((rows_bf16_kernel<G, V, Acc>), grid, dim3(kRowsBlock), 0, a.stream, a.M, xg.chunk, a.N, a.ldb, a.rowNnz,
                       a.out_bf16 ? 1u : 0u, a.ldc, b_bytes, c_bytes, a.rowPtrs, a.colIdxs, a.vals, a.B, a.C);
}

template <class Acc>
void launch_rows_acc(const RowsArgs &a) {
    const int vec = pick_vec_bf16(a);
    with_const<8, 4, 1>(vec, [&](auto v) {
        with_group(pick_group(a.N, vec), [&](auto g) { launch_rows<decltype(g)::value, decltype(v)::value, Acc>(a); });
    });
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_rows_bf16(mispmm_stream_t stream, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs, uint32_t rowNnz,
                                const uint32_t *colIdxs, const float *vals, const uint16_t *B, uint32_t N, uint32_t ldb, void *C,
                                uint32_t ldc, int out_bf16, int acc_mode, int sum_f32) {
    if (int s = check_acc_mode("rows_bf16", acc_mode)) return s;
    if (ldb < N || ldc < N)
        return fail(MISPMM_ERR_INVALID_ARG, "rows_bf16: leading dimension smaller than N (N=%u ldb=%u ldc=%u)", N, ldb, ldc);
    if (!rowPtrs && static_cast<uint64_t>(M) * rowNnz != nnz)
        return fail(MISPMM_ERR_INVALID_ARG, "rows_bf16: rowPtrs is null (every row holds rowNnz entries) but M * rowNnz != nnz (M=%u rowNnz=%u nnz=%u)",
                    M, rowNnz, nnz);
    if (M == 0 || N == 0) return MISPMM_OK;
    if (nnz != 0 && (!colIdxs || !vals)) return fail(MISPMM_ERR_INVALID_ARG, "rows_bf16: colIdxs or vals is null");
    if (!B || !C) return fail(MISPMM_ERR_INVALID_ARG, "rows_bf16: B or C is null");
    const uint32_t c_elem = out_bf16 ? 2u : 4u;
    if (!aligned_to(B, 2) || !aligned_to(C, c_elem))
        return fail(MISPMM_ERR_INVALID_ARG, "rows_bf16: B must be 2-byte aligned and C %u-byte aligned", c_elem);
    if (!fits_buffer(K, ldb, 2) || !fits_buffer(M, ldc, c_elem))
        return fail(MISPMM_ERR_UNSUPPORTED, "rows_bf16: B or C spans 2 GiB or more (K=%u ldb=%u M=%u ldc=%u); there is no wide body", K, ldb, M,
                    ldc);
    const RowsArgs a{as_stream(stream), M, K, rowNnz, rowPtrs, colIdxs, vals, B, N, ldb, C, ldc, out_bf16 != 0};
    if (acc_mode == MISPMM_ACC_FAST) launch_rows_acc<AccFast>(a);
    else if (sum_f32) launch_rows_acc<AccRefF32>(a);
    else launch_rows_acc<AccRefWide>(a);
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
