// The lane group of the fused fp32 attention on a CSR pattern, written once for the three kernels that are built on it:
// attn_csr_kernel (attn_csr.hip) and the row pass and the column pass of the backward (bwd/attn_csr_bwd.hip).
//
// Shape: G lanes own one (head, row) of the pass's own pattern; a lane owns VEC consecutive columns of each of NCH column chunks
// of G * VEC and holds its slices of the row's operands and of the fp32 accumulators in registers (G and NCH from max(D, Dv):
// every width up to 256 is held, there is no re-reading form).  The row's entries are walked in storage order in batches of 8.
// The 8 x NCH rows a batch needs of one operand are gathered by one key per entry, which lane i of every 8-lane segment holds
// for entry i; every lane sums its columns' products for the 8 entries (one fma chain each), and the TRANSPOSING butterfly of
// csrc/sddmm.hip leaves the sum of entry i in lane i of every 8-lane segment of the group -- the further doublings of G add
// commutatively, so all segments hold the same bits and the per-entry arithmetic of a kernel runs redundantly in each of them
// with no broadcast between segments.  The 8 per-entry results come back by a segment broadcast for the accumulating fmas.
// Dead slots of a last batch and lanes past a width read through the dropped-load offset, and the key and the lane offset are
// joined by a SATURATING add: two dropped halves stay dropped instead of wrapping to offset 0, so row 0 of an operand is never
// read on their behalf.
// Heads are the slow axis of the flattened grid and the (head, row block) items go over the XCDs by xcd_grid, so an XCD walks
// one head's rows at a time.  No LDS, no atomics, no scratch; fixed order throughout.
//
// What is NOT here, and stands in each kernel as before:
//  - the fetch of a batch's keys one batch ahead: where it stands relative to the batch's own reads is what makes it work, and
//    each kernel's loop spells it out;
//  - the item decode with its two early returns, the broadcast-and-fma accumulate, the masked row store and the forward's dot
//    chain.  Each was tried as a helper that takes the kernel's arrays by reference, and each changed the ISA of some of the 30
//    instances (registers, schedule of the row's first reads): the helper is optimised on its own before it is inlined, and the
//    scheduler sees another order.  Helpers that take and return VALUES (join_off, lane_off, dot_chain) and helpers that wrap the
//    very lambda the kernel had (gather_rows) left every instance as it was.
// The header lies beside its users and not in csrc/: every csrc/*.hpp is a prerequisite of libmispmm.so, and the census
// tests read csrc/ for its kernel tags.  The host pieces have internal linkage: each library exports its one entry point.
#pragma once
#include "lane_moves.hpp"

namespace mispmm {

namespace {

constexpr int kLgBlock = 256;  // threads per workgroup
constexpr int kLgBatch = 8;    // entries of a row per step: lane i of an 8-lane segment holds the i-th entry's scalars
constexpr int kLgMaxWidth = 256;

__device__ __forceinline__ float lg_exp(float t) { return __builtin_amdgcn_exp2f(t * 1.44269504088896340736f); }  // as softmax_csr.hip, FAST

// key + lane offset where either may be the dropped-load mark: saturating, so that two marks do not wrap to offset 0
__device__ __forceinline__ uint32_t join_off(uint32_t key, uint32_t off) { return __builtin_elementwise_add_sat(key, off); }

// one step of the transposing butterfly (sddmm.hip): 2 * H values in, H out; the lane whose bit MASK is clear keeps the even ones
template <int MASK, int H>
__device__ __forceinline__ void fold(const float *in, float *out, bool odd) {
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const float keep = odd ? in[2 * j + 1] : in[2 * j];
        const float send = odd ? in[2 * j] : in[2 * j + 1];
        out[j] = keep + lane_xor<MASK>(send);
    }
}

// the 8 per-lane partial sums of a batch -> the full sum of entry i in lane i of every 8-lane segment of the group
template <int G>
__device__ __forceinline__ float transpose_sum(const float *acc, uint32_t lane) {
    float w4[4], w2[2], w1[1];
    fold<1, 4>(acc, w4, (lane & 1u) != 0);
    fold<2, 2>(w4, w2, (lane & 2u) != 0);
    fold<4, 1>(w2, w1, (lane & 4u) != 0);
    float s = w1[0];
    if constexpr (G >= 16) s = s + lane_xor<8>(s);
    if constexpr (G >= 32) s = s + lane_xor<16>(s);
    if constexpr (G >= 64) s = s + lane_xor<32>(s);
    return s;
}

// byte offset of the lane's columns of chunk c in a row of `width` columns; past the width: the dropped-load mark
template <int G, int VEC>
__device__ __forceinline__ uint32_t lane_off(uint32_t lane, int c, uint32_t width) {
    const uint32_t col = c * (G * VEC) + lane * VEC;
    return col < width ? col * 4u : kDropLoad;
}

// the lane's slices of the batch's 8 rows of one operand; key: byte offset of the row of entry `sub`, or the mark
template <int VEC, int NCH>
__device__ __forceinline__ void gather_rows(uint32_t key, rsrc_t r, const uint32_t (&off)[NCH], typename VecOf<VEC>::type (&rows)[kLgBatch][NCH]) {
    static_for<0, kLgBatch>([&](auto j_tag) {
        constexpr int j = decltype(j_tag)::value;
        const uint32_t kj = group_bcast<8, j>(key);
#pragma unroll
        for (int c = 0; c < NCH; ++c) rows[j][c] = buffer_load_vec<VEC>(r, join_off(kj, off[c]), 0);
    });
}

// acc + the lane's part of <a, b> over one chunk: one fma chain in column order.  The backward's four chains; in the forward it
// moves the Q[r] read of the VEC == 4 instances behind the first key fetch, so the chain is spelled out there
template <int VEC>
__device__ __forceinline__ float dot_chain(typename VecOf<VEC>::type a, typename VecOf<VEC>::type b, float acc) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc = __builtin_fmaf(vec_get<VEC>(a, v), vec_get<VEC>(b, v), acc);
    return acc;
}

// elements one head's rows span: the last row ends with its last column, not with its stride
uint64_t span(uint64_t rows, uint32_t ld, uint32_t width) { return rows == 0 ? 0 : (rows - 1) * ld + width; }

// f(G, VEC, NCH) as constants -- lanes of a row, elements of a lane, chunks of G * VEC columns: the one list of the instances
// that exist
template <class F>
void with_instance(int vec, int g, uint32_t width, F &&f) {
    using std::integral_constant;
    if (vec == 4) {
        with_group(g, [&](auto gr) { f(gr, integral_constant<int, 4>{}, integral_constant<int, 1>{}); });  // 64 x 4 covers 256
    } else if (!try_const<8, 16, 32>(g, [&](auto gr) { f(gr, integral_constant<int, 1>{}, integral_constant<int, 1>{}); })) {
        const uint32_t chunks = ceil_div(width, static_cast<uint32_t>(kWave));
        with_const<1, 2, 4>(chunks <= 1 ? 1 : chunks == 2 ? 2 : 4,
                            [&](auto ch) { f(integral_constant<int, 64>{}, integral_constant<int, 1>{}, ch); });
    }
}

// the grid of a pass over `rows` rows of each of H heads, a group of G lanes per row: completes p, returns the blocks to launch
template <int G, class Params>
uint32_t finish_grid(Params &p, uint32_t rows, uint32_t H) {
    p.blocks_per_head = ceil_div(rows, static_cast<uint32_t>(kLgBlock / G));
    p.total = p.blocks_per_head * H;
    const XcdGrid xg = xcd_grid(p.total);
    p.xcd_chunk = xg.chunk;
    return xg.grid;
}

// what every entry point refuses first, whatever its sizes; `name` begins the message
int refuse_shape(const char *name, uint32_t D, uint32_t Dv, float scale) {
    if (D == 0 || Dv == 0 || D > kLgMaxWidth || Dv > kLgMaxWidth)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: D and Dv must be from 1 to %d (got D=%u Dv=%u)", name, kLgMaxWidth, D, Dv);
    if (!(__builtin_fabsf(scale) < __builtin_huge_valf()))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: scale must be finite (got %g)", name, static_cast<double>(scale));
    return MISPMM_OK;
}

// ... and last: the flattened grid of the larger pass has to fit one launch
int refuse_grid(const char *name, uint32_t rows, uint32_t H, int g) {
    if (static_cast<uint64_t>(ceil_div(rows, static_cast<uint32_t>(kLgBlock / g))) * H > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: %u rows x %u heads are more workgroups than one launch takes", name, rows, H);
    return MISPMM_OK;
}

}  // namespace

}  // namespace mispmm
