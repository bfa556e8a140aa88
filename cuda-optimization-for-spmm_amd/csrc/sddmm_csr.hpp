// SDDMM on a CSR pattern, written once for every element type: out[e] = <X[row(e), :], Y[col(e), :]> for every stored entry e
// of A (A's values are not read).  csrc/sddmm.hip (fp32, fp64) and sddmm_bf16/sddmm_csr_bf16.hip (bf16) each wrap the body
// below in their own __global__ kernel, with their own parameter list and their own store, and launch it through the ladder
// at the end.
//
// Shape: the row-gather kernel's (row_gather.hpp) -- G lanes own one row of A, a lane owns VEC consecutive columns of each
// column chunk of G * VEC.  The group keeps its slice of X[row] in registers as it was loaded (up to 4 chunks; wider
// rows re-read X per batch, from L1), walks the row's entries in batches of 8 with the 8 x NCH Y-row reads of a batch
// independent of each other, and sums every lane's 8 partial dot products across the group with a TRANSPOSING butterfly:
// in step k a lane keeps the half of its values whose entry number has bit k equal to its own lane bit k and hands the other
// half to lane ^ (1 << k), so 8 values cross the group in 4 + 2 + 1 moves (then one per further doubling of G) instead of
// 8 * log2(G), and lane i of the group ends up with the result of entry i of the batch: lanes 0..7 store 8 consecutive
// elements of `out`.  The moves (lane_moves.hpp) are DPP (quad_perm, row_ror) or ds_swizzle; lane ^ 32 goes through ds_bpermute.
// A batch's column keys reach the group by DPP row_newbcast: per key two moves (lane j and lane 8 + j of the 16-lane row) and
// a select on the lane's own half, 16 moves per batch; with G >= 16 one move would do (both halves hold the same keys).
// Fixed order throughout: run to run identical.  No LDS, no scratch.
//
// An element policy Elem names: in_t (what X and Y point at), kBytes (bytes per element), raw_t<VEC> (a lane's slice of a
// row as it is loaded), load<VEC> (through a raw buffer descriptor; the dropped-load mark gives zeros) and at<VEC>(raw, i)
// (column i of the slice as the arithmetic policy P takes it).  P names A (the type of a partial sum), mac and finish.
#pragma once
#include "lane_moves.hpp"

namespace mispmm {

namespace {

constexpr int kSdBlock = 256;  // threads per workgroup
constexpr int kSdBatch = 8;    // entries of a row summed at once: lane i < 8 of a group stores the i-th

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
// X re-read chunk by chunk for every batch of entries.  store(e, r): result r of entry e of A, called by the lane that holds it.
template <class Elem, class P, int G, int VEC, int NCH, class Store>
__device__ __forceinline__ void sddmm_csr_body(uint32_t M, uint32_t N, uint32_t xcd_chunk, uint32_t ldx, uint32_t ldy,
                                               const uint32_t *rowPtrs, const uint32_t *colIdxs,
                                               const typename Elem::in_t *X, uint32_t x_bytes,
                                               const typename Elem::in_t *Y, uint32_t y_bytes, Store store) {
    using A = typename P::A;
    using raw_t = typename Elem::template raw_t<VEC>;
    static_assert(G >= kSdBatch && (G & (G - 1)) == 0 && G <= kWave, "a batch's results sit in the first lanes of a group");
    static_assert(NCH > 0 || G == kWave, "the chunk loop is for rows wider than a wave");
    constexpr int GROUPS = kSdBlock / G, E = kSdBatch;
    constexpr uint32_t ES = Elem::kBytes, CHUNK = G * VEC;
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
    // A lane of several columns: N is a multiple of VEC, so a lane's columns lie inside N or past it together
    auto col_off = [&](uint32_t c0) {
        const uint32_t col = c0 + lane * VEC;
        return col < N ? col * ES : kDropLoad;
    };
    // A Y read's offset is key + column offset and either part may be kDropLoad.  Both at once -- a slot past the row end
    // in a lane past N -- wrap to offset 0: that lane really reads Y[0][0..VEC) (zeros where Y is shorter than that).  It is
    // an in-range read that changes no result: the lane's X is zero, the product (0 * y, a NaN if y is not finite) lands
    // only in the sum of a slot past the row end, the butterfly keeps the slots apart and the store is guarded.
    uint32_t off[NCH > 0 ? NCH : 1];
    raw_t xv[NCH > 0 ? NCH : 1];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            off[c] = col_off(c * CHUNK);
            xv[c] = Elem::template load<VEC>(xr, x_row + off[c]);
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
                for (int c = 0; c < NCH; ++c) yv[c] = Elem::template load<VEC>(yr, kj + off[c]);
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) P::mac(acc[j], Elem::template at<VEC>(xv[c], v), Elem::template at<VEC>(yv[c], v));
            });
        } else {
            uint32_t kj[E];
            static_for<0, E>([&](auto j_tag) { kj[decltype(j_tag)::value] = group_bcast<8, decltype(j_tag)::value>(key); });
            for (uint32_t c0 = 0; c0 < N; c0 += CHUNK) {
                const uint32_t o = col_off(c0);
                const raw_t x = Elem::template load<VEC>(xr, x_row + o);
                raw_t yv[E];
#pragma unroll
                for (int j = 0; j < E; ++j) yv[j] = Elem::template load<VEC>(yr, kj[j] + o);
#pragma unroll
                for (int j = 0; j < E; ++j)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) P::mac(acc[j], Elem::template at<VEC>(x, v), Elem::template at<VEC>(yv[j], v));
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
        if (lane < E && s0 + lane < len) store(static_cast<size_t>(base) + s0 + lane, P::finish(r));
    }
}

// launch(G, NCH) as constants for lanes of VEC columns: 8, 16 or 32 lanes own a row that fits them in one chunk, or ...
template <int VEC, class F>
void launch_sddmm_shape(uint32_t N, F &&launch) {
    using std::integral_constant;
    if (try_const<8, 16, 32>(pick_group(N, VEC), [&](auto g) { launch(g, integral_constant<int, 1>{}); })) return;
    // a whole wave per row: 1, 2 or 4 chunks of 64 lanes held in registers, 0 = a loop over any number
    const uint32_t chunks = ceil_div(N, static_cast<uint32_t>(kWave * VEC));
    with_const<1, 2, 4, 0>(chunks <= 1 ? 1 : chunks == 2 ? 2 : chunks <= 4 ? 4 : 0, [&](auto c) { launch(integral_constant<int, 64>{}, c); });
}

}  // namespace

}  // namespace mispmm
