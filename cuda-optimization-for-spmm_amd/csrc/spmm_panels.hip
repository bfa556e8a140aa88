// CSR x dense for the DENSE regime (every B row re-read by hundreds of rows of A): B walked in PANELS of P consecutive rows,
// each panel staged once per workgroup into LDS, every row of the workgroup summing its entries of that panel from there.
// Stands in for the shared-memory staging of /root/reference/src/spmm/csr/spmm_csr_k4.cu:26-79 on inputs like the reference's
// test/sparsity.sh sweep (2048 x 2048 at density 0.1 .. 0.9): the row-gather kernel fetches 16 bytes of B from the vector L1
// per four products, which is its floor there; LDS serves the same bytes at four times that rate.
//
// Work split: a 320-thread workgroup = four summing waves + one staging wave.  The summing waves' 16 lane groups of 16 lanes own
// R = 16 * RPG rows of A (lane group g: rows g, g + 16, ... of the block) and 64 output columns (lane l: columns 4 l .. 4 l + 3)
// and keep R x 64 sums in registers across all panels.
// Staging: panel p = B rows [p P, (p + 1) P) x 64 columns = P slices of 256 bytes, slice j at LDS offset 256 j of one of two
// buffers; the staging wave puts panel p + 1 on its way (LDS-DMA, 1 KiB = 4 slices per wave instruction as in spmm_tiles.hip)
// while panel p is consumed; one barrier per panel.  A wave of its own because the vector-memory counter retires in order: a
// summing wave that had issued the DMA would wait for the whole next panel at its next wait for 16 entries of A.
// No column list: an entry's slice is col - p P.
// A side: panelPtrs (mispmm_csr_panels_host) -- per row numPanels + 1 offsets into the matrix's own colIdxs / vals, so the
// kernel never searches.  A lane group fetches 16 entries at a time (lane i entry i, next 16 prefetched), the entries reach the
// group by DPP broadcast, ds_read_b128 reads the slice (16 lanes x 16 bytes = one 256-byte bank row: conflict-free).  Entries
// past a row's share of the panel are dropped buffer loads (value 0) pointed at a slice of zeros: + 0 * 0, an exact no-op.
// Order: panels ascend, and inside a panel a row's entries are taken in storage order -- for rows whose columns ascend (the
// builder declines others) that IS storage order, so AccRefWide gives the oracle's bits.
#include "row_gather.hpp"

namespace mispmm {

static bool panel_rows_supported(uint32_t p) { return p == 64u || p == 128u; }

template <class Acc, int P, int RPG, bool DMA>
__global__ __launch_bounds__(320, 2) void csr_panel_kernel(
    const uint32_t *__restrict__ panelPtrs, const uint32_t *__restrict__ colIdxs, const float *__restrict__ vals, uint32_t a_bytes,
    const float *__restrict__ B, uint32_t b_bytes, uint32_t M, uint32_t K, uint32_t numPanels, uint32_t ldb, uint32_t numRowBlocks,
    uint32_t tiling /* bits 0..7 log2 of the row parts of the XCD grid, bits 8.. row blocks per row part */, uint32_t cols_per_part,
    uint32_t N, float *__restrict__ C, uint32_t c_bytes, uint32_t ldc) {
    constexpr int G = 16, VEC = 4, R = G * RPG, SUMMING = 256;
    constexpr uint32_t kZeroSlice = 2u * P;                   // slice index of the 256 zero bytes behind the two buffers
    __shared__ f32x4 lds[(2 * P + 1) * G];                    // ONE array: 2 x P slices x 16 lanes x 16 B (+ the zero slice)
    const uint32_t lane = threadIdx.x % G, g = threadIdx.x / G;   // g 0..15: the summing lane groups; 16..19: the staging wave's
    const uint32_t xcd = blockIdx.x & 7u, log2p = tiling & 0xFFu, chunk = tiling >> 8;
    const uint32_t part = xcd & ((1u << log2p) - 1u), q = xcd >> log2p;
    const uint32_t rb = part * chunk + (blockIdx.x >> 3);
    if (rb >= numRowBlocks) return;                           // the whole workgroup leaves: no barrier is left waiting
    const uint32_t col0 = q * cols_per_part + blockIdx.y * (G * VEC) + lane * VEC;
    const bool col_ok = col0 < min(N, (q + 1) * cols_per_part);
    const uint32_t lane_off = col_ok ? col0 * 4u : kDropLoad;

    if (threadIdx.x >= SUMMING) {
        // ---- the staging wave (wave-uniform branch): one barrier per panel, the same count as the summing waves
        const rsrc_t brs = make_rsrc(B, b_bytes);
        const uint32_t ldb4 = ldb * 4u, sub = g - SUMMING / G;   // which of the four B rows of one 1 KiB step this lane group moves
        if (sub == 0) lds[kZeroSlice * G + lane] = f32x4{0.f, 0.f, 0.f, 0.f};
        // step k moves B rows p P + 4 k .. + 3 (one per lane group) to slices 4 k .. 4 k + 3 of the buffer: 1 KiB contiguous.
        // Rows past K and columns past the part are dropped loads.
        auto stage = [&](uint32_t p, uint32_t buf) {
            const uint32_t row0 = p * P + sub;                    // this lane group's B row of step 0
            if constexpr (DMA) {
                using lds_ptr_t = __attribute__((address_space(3))) void *;
#pragma unroll 8
                for (uint32_t k = 0; k < P / 4; ++k) {
                    // LDS destination = base + lane-in-wave * 16
                    const uint32_t lds_base = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds)) + (buf * P + 4u * k) * (G * 16u);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(brs, reinterpret_cast<lds_ptr_t>(static_cast<uintptr_t>(lds_base)), 16,
                                                             row0 + 4u * k < K ? (row0 + 4u * k) * ldb4 + lane_off : kDropLoad, 0, 0, 0);
                }
            } else {
                for (uint32_t k0 = 0; k0 < P / 4; k0 += 8) {      // through registers, eight 1 KiB steps at a time
                    f32x4 v[8];
#pragma unroll
                    for (uint32_t u = 0; u < 8; ++u) v[u] = buffer_load_vec<VEC>(brs, row0 + 4u * (k0 + u) < K ? (row0 + 4u * (k0 + u)) * ldb4 + lane_off : kDropLoad, 0);
#pragma unroll
                    for (uint32_t u = 0; u < 8; ++u) lds[(buf * P + 4u * (k0 + u) + sub) * G + lane] = v[u];
                }
            }
        };
        if (numPanels != 0) stage(0, 0);
        for (uint32_t p = 0; p < numPanels; ++p) {
            // panel p has landed before the barrier that lets the summing waves read it; behind that barrier nobody reads
            // buffer (p + 1) & 1 any more (it held panel p - 1)
            if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (p + 1 < numPanels) stage(p + 1, (p + 1) & 1u);
        }
        return;
    }

    // ---- the summing waves
    const rsrc_t crs = make_rsrc(colIdxs, a_bytes), vrs = make_rsrc(vals, a_bytes);
    // this lane group's rows and their shares of the current panel: entries [beg, end); end of panel p + 1 is read a panel ahead
    uint32_t pp_at[RPG], beg[RPG], end[RPG], nxt_end[RPG];
    bool row_ok[RPG];
#pragma unroll
    for (int rr = 0; rr < RPG; ++rr) {
        const uint32_t row = rb * R + rr * G + g;
        row_ok[rr] = row < M;
        pp_at[rr] = min(row, M - 1u) * (numPanels + 1u);
        beg[rr] = panelPtrs[pp_at[rr]];
        end[rr] = panelPtrs[pp_at[rr] + min(1u, numPanels)];
        if (!row_ok[rr]) beg[rr] = end[rr] = 0u;
    }
    typename Acc::T acc[RPG][VEC];
#pragma unroll
    for (int rr = 0; rr < RPG; ++rr)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[rr][i] = 0;
    // entries idx = at + lane of a row's share as (LDS slice-lane index, coefficient); past `stop`: the zero slice, 0
    auto fetch = [&](uint32_t at, uint32_t stop, uint32_t slice0, uint32_t pbase, uint32_t &sidx, float &val) {
        const uint32_t idx = at + lane;
        const bool live = idx < stop;
        const uint32_t voff = live ? idx * 4u : kDropLoad;
        const uint32_t col = __builtin_amdgcn_raw_buffer_load_b32(crs, voff, 0, 0);
        val = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vrs, voff, 0, 0));
        sidx = (live ? slice0 + (col - pbase) : kZeroSlice) * G;
    };
    // the first 16 entries of every row of the group for panel 0 (later panels: fetched while the previous one is summed)
    uint32_t first_sidx[RPG];
    float first_val[RPG];
#pragma unroll
    for (int rr = 0; rr < RPG; ++rr) fetch(beg[rr], end[rr], 0u, 0u, first_sidx[rr], first_val[rr]);

    for (uint32_t p = 0; p < numPanels; ++p) {
        const uint32_t buf = p & 1u, pbase = p * P, slice0 = buf * P;
        __syncthreads();                                      // panel p is in buffer `buf` (the staging wave waited for it)
#pragma unroll
        for (int rr = 0; rr < RPG; ++rr) nxt_end[rr] = panelPtrs[pp_at[rr] + min(p + 2u, numPanels)];
        static_for<0, RPG>([&](auto rr_tag) {
            constexpr int RR = decltype(rr_tag)::value;
            uint32_t nxt_sidx = first_sidx[RR];
            float nxt_val = first_val[RR];
            // as long as any of the wave's four lane groups has entries left in this panel (wave-uniform)
            for (uint32_t at = beg[RR]; __any(at < end[RR]); at += G) {
                const uint32_t my_sidx = nxt_sidx;
                const float my_val = nxt_val;
                fetch(at + G, end[RR], slice0, pbase, nxt_sidx, nxt_val);
                static_for<0, 4>([&](auto quad_tag) {
                    constexpr int Q4 = decltype(quad_tag)::value * 4;
                    if (Q4 == 0 || __any(at + Q4 < end[RR])) {            // the body is as long as the wave's longest share needs
                        static_for<Q4, Q4 + 4>([&](auto s) {
                            constexpr int S = decltype(s)::value;
                            const uint32_t sidx = group_bcast<G, S>(my_sidx);
                            const float a = __builtin_bit_cast(float, group_bcast<G, S>(__builtin_bit_cast(uint32_t, my_val)));
                            const f32x4 b = lds[sidx + lane];
                            if constexpr (std::is_same_v<Acc, AccRefWide>) {
                                Acc::mac4(acc[RR], a, b[0], b[1], b[2], b[3]);
                            } else {
#pragma unroll
                                for (int i = 0; i < VEC; ++i) Acc::mac(acc[RR][i], a, b[i]);
                            }
                        });
                    }
                });
            }
            // this row's first entries of the NEXT panel, on their way while the group's other rows are summed
            const uint32_t nend = row_ok[RR] ? nxt_end[RR] : 0u;
            fetch(end[RR], nend, (buf ^ 1u) * P, pbase + P, first_sidx[RR], first_val[RR]);
            beg[RR] = end[RR];
            end[RR] = nend;
        });
    }
    const rsrc_t ors = make_rsrc(C, c_bytes);
#pragma unroll
    for (int rr = 0; rr < RPG; ++rr) {
        f32x4 out;
#pragma unroll
        for (int i = 0; i < VEC; ++i) out[i] = Acc::finish(acc[rr][i]);
        const uint32_t row = rb * R + rr * G + g;
        buffer_store_vec_c<VEC>(ors, (row_ok[rr] && col_ok) ? (row * ldc + col0) * 4u : kDropLoad, out);
    }
}

struct PanelArgs {
    hipStream_t st;
    uint32_t M, K, nnz;
    const uint32_t *colIdxs;
    const float *vals;
    const uint32_t *panelPtrs;
    const float *B;
    uint32_t N, ldb;
    float *C;
    uint32_t ldc;
};

template <class Acc, int P, int RPG, bool DMA>
static void launch_panels_as(const PanelArgs &a, const XcdTiling &t) {
    const uint32_t cols_per_part = a.N / t.q;
    const uint32_t numRowBlocks = ceil_div(a.M, 16u * RPG), chunk = ceil_div(numRowBlocks, 1u << t.log2p);
    dim3 grid(8u * chunk, ceil_div(cols_per_part, 64u));
    note_kernel("csr_panel<%s,P%d,R%d,%s> xcd %ux%u, %u panels", std::is_same_v<Acc, AccRefWide> ? "ref" : "fast", P, 16 * RPG,
                DMA ? "lds-dma" : "ds_write", 1u << t.log2p, t.q, ceil_div(a.K, static_cast<uint32_t>(P)));
    hipLaunchKernelGGL((csr_panel_kernel<Acc, P, RPG, DMA>), grid, dim3(320), 0, a.st, a.panelPtrs, a.colIdxs, a.vals, a.nnz * 4u, a.B,
                       static_cast<uint32_t>(static_cast<uint64_t>(a.K) * a.ldb * 4u), a.M, a.K, ceil_div(a.K, static_cast<uint32_t>(P)), a.ldb,
                       numRowBlocks, t.log2p | (chunk << 8), cols_per_part, a.N, a.C,
                       static_cast<uint32_t>(static_cast<uint64_t>(a.M) * a.ldc * 4u), a.ldc);
}

// false: a knob combination the tuning build holds no kernel for (nothing launched)
template <class Acc>
static bool launch_panels(const PanelArgs &a, uint32_t panelRows) {
    const XcdTiling t = xcd_tiling(a.N, 4, a.K);
    // MISPMM_PANEL_R = 32 | 64 rows per workgroup, MISPMM_PANEL_DMA = 0: staging through registers and ds_write_b128
    // (tuning build only; the production library holds the default form of each panel depth)
    [[maybe_unused]] static const int rows = knob_int("MISPMM_PANEL_R", 64);
    [[maybe_unused]] static const bool dma = knob_int("MISPMM_PANEL_DMA", 1) != 0;
#ifdef MISPMM_TUNING
    if (rows != 64 || !dma) {
        if (panelRows == 128u && rows == 32 && dma) launch_panels_as<Acc, 128, 2, true>(a, t);
        else if (panelRows == 64u && rows == 32 && dma) launch_panels_as<Acc, 64, 2, true>(a, t);
        else if (panelRows == 128u && rows == 64 && !dma) launch_panels_as<Acc, 128, 4, false>(a, t);
        else return false;
        return true;
    }
#endif
    if (panelRows == 64u) launch_panels_as<Acc, 64, 4, true>(a, t);
    else launch_panels_as<Acc, 128, 4, true>(a, t);
    return true;
}

}  // namespace mispmm

using namespace mispmm;

extern "C" uint32_t mispmm_csr_panel_rows(void) {
    const int p = knob_int("MISPMM_PANEL_P", static_cast<int>(MISPMM_PANEL_ROWS));
    return panel_rows_supported(static_cast<uint32_t>(p)) ? static_cast<uint32_t>(p) : MISPMM_PANEL_ROWS;
}

extern "C" int mispmm_csr_panel_f32(mispmm_stream_t stream, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                    const uint32_t *colIdxs, const float *vals, const uint32_t *panelPtrs, uint32_t panelRows,
                                    const float *B, uint32_t N, uint32_t ldb, float *C, uint32_t ldc, int acc_mode) {
    (void)rowPtrs;  // panelPtrs holds every row's bounds (its first and last offset): the kernel never reads the row pointers
    if (int s = check_acc_mode("csr_panel", acc_mode)) return s;
    if (M == 0 || N == 0) return MISPMM_OK;
    if (!panelPtrs || (nnz != 0 && (!colIdxs || !vals))) return fail(MISPMM_ERR_INVALID_ARG, "csr_panel: null pointer");
    if (int s = check_dense_args(B, N, ldb, C, ldc)) return s;
    if (!panel_rows_supported(panelRows))
        return fail(MISPMM_ERR_UNSUPPORTED, "csr_panel: panels of 64 or 128 B rows (got %u; build them with mispmm_csr_panel_rows())", panelRows);
    const uint64_t offsets = static_cast<uint64_t>(M) * (ceil_div(K, panelRows) + 1u);
    if (pick_vec(B, ldb, C, ldc, N) != 4 || !fits_buffer(K, ldb, 4) || !fits_buffer(M, ldc, 4) || !fits_buffer(nnz, 1, 4) ||
        !fits_buffer(offsets, 1, 1) || ceil_div(M, 32u) >= (1u << 24))
        return fail(MISPMM_ERR_UNSUPPORTED, "csr_panel: N a multiple of 4 with 16-byte-aligned B, C, ldb, ldc; B, C and the entries below 2 GiB");
    const PanelArgs a{as_stream(stream), M, K, nnz, colIdxs, vals, panelPtrs, B, N, ldb, C, ldc};
    if (!with_acc<AccRefWide, AccFast>(acc_mode, [&](auto acc) { return launch_panels<typename decltype(acc)::type>(a, panelRows); }))
        return fail(MISPMM_ERR_UNSUPPORTED, "csr_panel: no kernel is built for this MISPMM_PANEL_P / MISPMM_PANEL_R / MISPMM_PANEL_DMA combination");
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
