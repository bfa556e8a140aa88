// fp64 SpMM: one row-gather kernel (row_gather_f64.hpp) over a row list (rowPtrs, colIdxs, vals).  CSR is such a list; the
// host layers bring COO (stable-sorted by row + mispmm_coo_row_bounds), ELL (mispmm_ell_colmajor_to_rows_f64_host) and BSR
// (mispmm_bsr_nonzeros_f64_host) into the same form once per upload.
#include "row_gather_f64.hpp"

namespace mispmm {

namespace {

struct F64Args {
    hipStream_t stream;
    uint32_t M, K;
    const uint32_t *rowPtrs, *colIdxs;
    const double *vals, *B;
    uint32_t N, ldb;
    double *C;
    uint32_t ldc;
};

// 16-byte lanes wherever B and C rows allow them (16-byte gathers reach 58-61 B/clk, 8-byte ones 35)
int pick_vec_f64(const F64Args &a) {
    return (a.N % 2 == 0 && a.ldb % 2 == 0 && a.ldc % 2 == 0 && aligned16(a.B) && aligned16(a.C)) ? 2 : 1;
}

// P x Q XCD grid: Q column parts of at least 128 doubles (1 KiB of each B row), P = 8 / Q row parts.  N <= 128 keeps 8 x 1:
// a lane group covers the whole row (N = 64: 32 lanes, N = 128: the whole wave).
uint32_t f64_parts(uint32_t N, int vec) {
    uint32_t q = 1;
    if (vec == 2)
        while (q < 8 && N % (2u * q * 16u) == 0 && N / (2u * q) >= 128u) q *= 2;
    return q;
}

template <int G, int VEC, class Acc, bool WIDE>
void launch_f64(const F64Args &a, uint32_t q) {
    const uint32_t log2p = q == 1 ? 3u : q == 2 ? 2u : q == 4 ? 1u : 0u;
    const uint32_t cols_per_part = a.N / q;
    const uint32_t rb = ceil_div(a.M, static_cast<uint32_t>(kF64Block / G));
    const uint32_t rb_chunk = ceil_div(rb, 1u << log2p);
    const dim3 grid(8u * rb_chunk, ceil_div(cols_per_part, G * VEC));
    // WIDE ignores the byte counts; otherwise both are below 2 GiB (checked by the caller)
    const uint32_t b_bytes = WIDE ? 0u : static_cast<uint32_t>(static_cast<uint64_t>(a.K) * a.ldb * 8u);
    const uint32_t c_bytes = WIDE ? 0u : static_cast<uint32_t>(static_cast<uint64_t>(a.M) * a.ldc * 8u);
    note_kernel("csr_f64<G%d,V%d,%s%s> xcd %ux%u", G, VEC, std::is_same_v<Acc, Acc64Ref> ? "ref" : "fast", WIDE ? ",wide" : "",
                1u << log2p, q);
    hipLaunchKernelGGL((csr_f64_kernel<G, VEC, Acc, WIDE>), grid, dim3(kF64Block), 0, a.stream, a.M, rb_chunk, log2p, cols_per_part,
                       a.N, a.ldb, a.rowPtrs, a.colIdxs, a.vals, a.B, b_bytes, a.C, c_bytes, a.ldc);
}

template <class Acc>
void launch_f64_acc(const F64Args &a) {
    const int vec = pick_vec_f64(a);
    const uint32_t q = f64_parts(a.N, vec);
    with_flag(!fits_buffer(a.K, a.ldb, 8) || !fits_buffer(a.M, a.ldc, 8), [&](auto wide) {
        with_const<2, 1>(vec, [&](auto v) {
            with_group(pick_group(a.N / q, vec), [&](auto g) { launch_f64<decltype(g)::value, decltype(v)::value, Acc, decltype(wide)::value>(a, q); });
        });
    });
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_csr_f64(mispmm_stream_t stream, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                              const uint32_t *colIdxs, const double *vals, const double *B, uint32_t N, uint32_t ldb,
                              double *C, uint32_t ldc, int acc_mode) {
    if (int s = check_acc_mode("csr_f64", acc_mode)) return s;
    if (M == 0 || N == 0) return MISPMM_OK;
    if (int s = check_row_list("csr_f64", rowPtrs, nnz, colIdxs, vals)) return s;
    if (!B || !C) return fail(MISPMM_ERR_INVALID_ARG, "csr_f64: B or C is null");
    if (ldb < N || ldc < N)
        return fail(MISPMM_ERR_INVALID_ARG, "csr_f64: leading dimension smaller than N (N=%u ldb=%u ldc=%u)", N, ldb, ldc);
    const F64Args a{as_stream(stream), M, K, rowPtrs, colIdxs, vals, B, N, ldb, C, ldc};
    with_acc<Acc64Ref, Acc64Fast>(acc_mode, [&](auto acc) { launch_f64_acc<typename decltype(acc)::type>(a); });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
