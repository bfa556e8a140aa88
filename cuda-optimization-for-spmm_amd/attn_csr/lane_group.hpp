// The lane group of the fused attention on a CSR pattern, written once for the three kernels that are built on it: the forward
// (attn_csr_fwd.hpp) and the row pass and the column pass of the backward (attn_csr_bwd.hpp), each written once over the element
// policy of elem.hpp and instantiated for fp32 and for bf16 operands by the four libraries' own units.
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
//  - the item decode with its two early returns, the broadcast-and-fma accumulate, the masked row store and the dot chains.
//    Each was tried as a helper that takes the kernel's arrays by reference, and each changed the ISA of some of the
//    instances (registers, schedule of the row's first reads): the helper is optimised on its own before it is inlined, and the
//    scheduler sees another order.  Helpers that take and return VALUES (join_off, the policy's lane_off, load and at) and
//    helpers that wrap the very lambda the kernel had (the policy's gather) left every instance as it was (DESIGN.md section 9
//    items 17, 18 and 22).
// What depends on the element type (a lane's offset, the gather, the list of instances) is in elem.hpp.
// The headers lie beside their users and not in csrc/: every csrc/*.hpp is a prerequisite of libmispmm.so, and the census
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

// elements one head's rows span: the last row ends with its last column, not with its stride
uint64_t span(uint64_t rows, uint32_t ld, uint32_t width) { return rows == 0 ? 0 : (rows - 1) * ld + width; }

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
