// Fused block-sparse attention forward in bf16 (mispmm_attn.h): scores, row softmax and the product with V in ONE launch for
// all heads.  The scores and the weights P never leave the registers; per matrix row only a log-sum-exp is kept.
//   s[e][i][j] = <Q_h[R * bS + i, :D], K_h[c * bS + j, :D]>           v_mfma_f32_16x16x32_bf16, columns ascending (as sddmm_bsr.hip)
//   z          = fl32(scale * s + mask[e][i][j])                      one fma; no mask: the product (as softmax_bsr.hip)
//   out_h[r,:] = sum_e sum_j softmax_row(z)[e][j] * V_h[c * bS + j, :Dv]
//
// Work unit, lane layout of the two transposed products, loads and the MFMA hazard: attn_bsr_tiles.hpp.  Here the wave's 16
// rows are matrix rows, a step's 32 rows are keys (a half step's second tile has scores -Inf and its V loads are dropped),
// X = V and W = P: the rescale factor and 1 / l of row i are lane-local.  Every sum has a fixed order: run to run identical.
//
// Online softmax in fp32: a running maximum m (two xor moves over g per step, lane_moves.hpp: the only cross-lane traffic
// of the loop), running sums and the accumulator O rescaled by exp(mu_old - mu_new) when the maximum moves.  The weights
// enter the second MFMA as bf16 -- exp(z - mu) rounded once to nearest even -- and l sums the ROUNDED weights, the values
// the product multiplies by: a constant column of V comes back to fp32 accuracy.  A second sum lx of the unrounded weights
// gives lse = mu + log lx.  Each lane sums its own keys; the four lanes of a row meet once, after the loop.
// mu is m with an infinite m replaced by 0 (what torch.logsumexp subtracts): a row of nothing but -Inf has weights
// exp(-Inf) = 0, l = 0, out = 0 * (1 / 0) = NaN, lse = -Inf; a +Inf gives the weight +Inf, l = +Inf, O = +-Inf or NaN,
// out = NaN throughout the row, lse = +Inf; a NaN is dropped by the maximum and carried by the weight: l, lx, O are NaN.  While
// m is still -Inf (every key so far masked) O and l are exactly 0 and the rescale factor is set to 1: exp(0 - m_new) could
// overflow and 0 * Inf would poison the row.  Column i of P^T reaches only column i of O^T: a NaN stays in its matrix row.
//
// O is read by VALU (the rescale) in the iteration after the MFMAs that wrote it, and by the store after the loop: settle()
// once per step, after the step's exponentials and before the rescale, and once before the store.
//
// Everything a step reads -- K fragments, the mask's elements, V's rows -- is fetched one step ahead into the other of two
// register stages (in turn, no copy, as sddmm_bsr.hip has it), and the block columns of a fetch are read one step further
// ahead by scalar loads: the memory counter is in order, so a step that waited for a load issued inside it would wait for
// its prefetches too.
#include "attn_bsr_tiles.hpp"
#include "mispmm_attn.h"

namespace mispmm {

namespace {

struct AttnParams {
    uint32_t units, wgs_per_head, total, xcd_chunk;  // units: 16-row work units of one head; total: workgroups of all heads
    uint32_t Kb, D, Dv, rows;                        // rows = numBlockRows * bS
    uint32_t ldq2, ldk2, ldv2, ldo;                  // ld*2: row strides in bytes; ldo in elements
    uint32_t q_bytes, k_bytes, v_bytes;              // one head's span: (rows - 1) * ld + width elements
    float scale;
    uint64_t q_head, k_head, v_head, o_head;         // elements
};

// BS: block size.  DS: 32-column steps of D held (D <= 32 DS).  TPL: accumulator tiles = consecutive V columns per lane
// (Dv <= 16 TPL).  The arrays are kernel arguments of their own, `const __restrict__`: the block columns then come by scalar
// loads, which do not queue behind the vector loads in flight.
template <int BS, int DS, int TPL, bool MASK, bool OUT_BF16>
__global__ void __launch_bounds__(64 * kTileWaves)
    attn_bsr_kernel(const AttnParams p, const uint32_t *__restrict__ blockRowPtrs, const uint32_t *__restrict__ blockColIdxs,
                    const uint16_t *__restrict__ Q, const uint16_t *__restrict__ K, const uint16_t *__restrict__ V, const float *__restrict__ mask,
                    void *__restrict__ out, float *__restrict__ lse_out) {
    using W = Walk<BS>;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t item = xcd_block(blockIdx.x, p.xcd_chunk);
    if (item >= p.total) return;
    const uint32_t h = item / p.wgs_per_head;
    const uint32_t unit = (item - h * p.wgs_per_head) * kTileWaves + wave;
    if (unit >= p.units) return;
    const uint32_t R = unit / W::T, sub = unit % W::T;
    const uint32_t i = lane & 15, g = lane >> 4;
    const uint32_t row = unit * 16u + i;  // < rows
    const uint32_t bs = blockRowPtrs[R], be = blockRowPtrs[R + 1];
    const float ninf = -__builtin_huge_valf();

    f32x4_t acc[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    auto store = [&](float inv, float lse) {
        const size_t base = static_cast<size_t>(h) * p.o_head + static_cast<size_t>(row) * p.ldo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t col = TPL * (4u * g + k);
            if (col < p.Dv) store_run<TPL>(acc, k, inv, out, base, col, OUT_BF16);
        }
        if (lse_out && g == 0) lse_out[static_cast<size_t>(h) * p.rows + row] = lse;
    };
    if (be <= bs) {  // an empty block row: zero rows, lse = log 0
        store(1.f, ninf);
        return;
    }

    auto settle_acc = [&] { settle<TPL>(acc); };  // a lambda, like store: through a plain call the step's ISA moves

    const rsrc_t qr = make_rsrc(Q + h * p.q_head, p.q_bytes), kr = make_rsrc(K + h * p.k_head, p.k_bytes), vr = make_rsrc(V + h * p.v_head, p.v_bytes);
    const uint32_t kcol = g * 8u;  // the lane's 8 columns of a 32-column step of D
    bf16x8_t qf[DS];
#pragma unroll
    for (int s = 0; s < DS; ++s) qf[s] = load_frag(qr, row * p.ldq2, s * 32u + kcol, p.D);  // < 2 GiB: the host declines anything larger

    // the lane's share of the offsets of K's fragments and of V in the V layout (attn_bsr_tiles.hpp, LOADS)
    uint32_t koff[DS], voff[4];
#pragma unroll
    for (int s = 0; s < DS; ++s) koff[s] = s * 32u + kcol < p.D ? i * p.ldk2 + (s * 32u + kcol) * 2u : kDropLoad;
    const uint32_t vcol = i * TPL;  // first of the lane's TPL V columns, one per accumulator tile
#pragma unroll
    for (int j = 0; j < 4; ++j) voff[j] = vcol < p.Dv ? (4u * g + j) * p.ldv2 + vcol * 2u : kDropLoad;
    const size_t mask_at = static_cast<size_t>(sub * 16u + i) * BS + 4u * g;  // the lane's 4 mask elements inside a block (32 x 32: + 16 for the second tile)

    // the block columns behind the two 16-key tiles of the step that starts at block e (bS = 32: one block); past the row's
    // end: none
    struct Cols {
        uint32_t a, b;
    };
    const uint32_t last = be - 1;
    auto cols_at = [&](uint32_t e) {
        const uint32_t ca = blockColIdxs[min(e, last)];
        if constexpr (BS == 16) {
            const uint32_t cb = blockColIdxs[min(e + 1, last)];
            return Cols{e < be ? ca : 0xFFFFFFFFu, e + 1 < be ? cb : 0xFFFFFFFFu};
        } else {
            return Cols{e < be ? ca : 0xFFFFFFFFu, e < be ? ca : 0xFFFFFFFFu};
        }
    };
    constexpr uint32_t kSecond = W::kSecond, EPS = W::EPS;
    // everything a step reads, fetched one step ahead: K fragments, the mask's elements, V's rows
    struct Stage {
        bf16x8_t k[2][DS];
        f32x4_t ma, mb;
        TRows<TPL> v;
    };
    auto load_stage = [&](Cols c, uint32_t e, Stage &st) {
        const bool va = c.a < p.Kb, vb = c.b < p.Kb;  // wave-uniform
        const uint32_t ra = va ? c.a * BS : 0u, rb = vb ? c.b * BS + kSecond : 0u;
#pragma unroll
        for (int s = 0; s < DS; ++s) {
            st.k[0][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(kr, va ? koff[s] : kDropLoad, ra * p.ldk2, 0));
            st.k[1][s] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(kr, vb ? koff[s] : kDropLoad, rb * p.ldk2, 0));
        }
        if constexpr (MASK) {  // a step past the row's end re-reads the row's last block: valid memory, never used
            const size_t ea = static_cast<size_t>(min(e, last)) * (BS * BS);
            const size_t eb = BS == 32 ? ea + 16u : static_cast<size_t>(min(e + 1, last)) * (BS * BS);
            st.ma = *reinterpret_cast<const f32x4_t *>(mask + ea + mask_at);
            st.mb = *reinterpret_cast<const f32x4_t *>(mask + eb + mask_at);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) load_trow<TPL>(st.v, j, vr, (j < 4 ? va : vb) ? voff[j & 3] : kDropLoad, (j < 4 ? ra : rb) * p.ldv2);
    };

    float m = ninf, mu = 0.f, l = 0.f, lx = 0.f;
    uint32_t e = bs;
    Cols nxt = cols_at(e + EPS);

    auto step = [&](const Stage &use, Stage &fill) {
        const Cols after = cols_at(e + 2 * EPS);
        load_stage(nxt, e + EPS, fill);
        const bool second = BS == 32 || e + 1 < be;  // wave-uniform: a half step has no second tile
        f32x4_t sa{0.f, 0.f, 0.f, 0.f}, sb{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DS; ++s) sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(use.k[0][s], qf[s], sa, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < DS; ++s) sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(use.k[1][s], qf[s], sb, 0, 0, 0);
        float z[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            z[j] = scaled<MASK>(p.scale, sa[j], use.ma, j);
            z[4 + j] = second ? scaled<MASK>(p.scale, sb[j], use.mb, j) : ninf;
        }
        float mx = z[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) mx = __builtin_fmaxf(mx, z[j]);  // drops a NaN operand: the weight carries it
        mx = __builtin_fmaxf(mx, lane_xor<16>(mx));
        mx = __builtin_fmaxf(mx, lane_xor<32>(mx));
        const float m_new = __builtin_fmaxf(m, mx);
        const float mu_new = __builtin_fabsf(m_new) == __builtin_huge_valf() ? 0.f : m_new;
        const float alpha = m == ninf ? 1.f : tile_exp(mu - mu_new);
        m = m_new;
        mu = mu_new;
        u32x4_t pw;
        float t = 0.f, tx = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float p0 = tile_exp(z[2 * w] - mu), p1 = tile_exp(z[2 * w + 1] - mu);
            pw[w] = __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(p0), static_cast<__bf16>(p1)});
            t = t + __uint_as_float(pw[w] << 16);
            t = t + __uint_as_float(pw[w] & 0xFFFF0000u);
            tx = tx + p0;
            tx = tx + p1;
        }
        l = l * alpha + t;
        lx = lx * alpha + tx;
        settle_acc();
#pragma unroll
        for (int tt = 0; tt < TPL; ++tt) acc[tt] = acc[tt] * alpha;
        const bf16x8_t pfrag = __builtin_bit_cast(bf16x8_t, pw);
#pragma unroll
        for (int w = 0; w < TPL / 2; ++w) mfma_trow_pair<TPL>(acc[2 * w], acc[2 * w + 1], use.v, w, pfrag);
        nxt = after;
        e += EPS;
    };

    // two stages in turn (a copy `cur = nxt` would wait for the loads it is meant to hide)
    Stage s0, s1;
    load_stage(cols_at(e), e, s0);
    for (;;) {
        step(s0, s1);
        if (e >= be) break;
        step(s1, s0);
        if (e >= be) break;
    }
    // the four lanes of a row meet: (g0 + g1) + (g2 + g3), both partners of a move holding the same sum
    l = l + lane_xor<16>(l);
    l = l + lane_xor<32>(l);
    lx = lx + lane_xor<16>(lx);
    lx = lx + lane_xor<32>(lx);
    settle_acc();
    store(1.f / l, mu + __builtin_logf(lx));
}

struct AttnCall {
    hipStream_t stream;
    uint32_t H, Mb;
    AttnParams p;
    const uint32_t *blockRowPtrs, *blockColIdxs;
    const uint16_t *Q, *K, *V;
    const float *mask;
    void *out;
    float *lse;
};

template <int BS, int DS, int TPL, bool MASK, bool OUT_BF16>
void launch_attn(const AttnCall &c) {
    AttnParams p = c.p;
    const uint32_t grid = finish_grid(p, c.Mb * (BS / 16), c.H);
    note_kernel("attn_bsr<b%d,%s,%s,D%d,T%d>", BS, OUT_BF16 ? "bf16" : "f32", MASK ? "mask" : "nomask", DS, TPL);
    hipLaunchKernelGGL((attn_bsr_kernel<BS, DS, TPL, MASK, OUT_BF16>), dim3(grid), dim3(64 * kTileWaves), 0, c.stream, p, c.blockRowPtrs,
                       c.blockColIdxs, c.Q, c.K, c.V, c.mask, c.out, c.lse);
}

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" int mispmm_attn_bsr_bf16(mispmm_stream_t stream, uint32_t H, uint32_t numBlockRows, uint32_t K, uint32_t bS, uint32_t numBlocks,
                                    const uint32_t *blockRowPtrs, const uint32_t *blockColIdxs, const uint16_t *Q, uint32_t ldq,
                                    uint64_t q_head, const uint16_t *Kmat, uint32_t ldk, uint64_t k_head, const uint16_t *V, uint32_t ldv,
                                    uint64_t v_head, uint32_t D, uint32_t Dv, const float *mask, float scale, void *out, uint32_t ldo,
                                    uint64_t o_head, int out_bf16, float *lse) {
    if (const int refused = refuse_shape("attn_bsr_bf16", bS, scale, D, Dv, K)) return refused;
    if (H == 0 || numBlockRows == 0) return MISPMM_OK;
    if (!blockRowPtrs || !Q || !Kmat || !V || !out || (numBlocks != 0 && !blockColIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_bf16: blockRowPtrs, blockColIdxs, Q, K, V or out is null");
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_bsr_bf16: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)", D,
                    ldq, ldk, Dv, ldv, ldo);
    // every lane reads and writes 16-byte (a 64-column bf16 out: 8-byte) vectors
    const uint32_t oq = out_bf16 ? 8u : 4u;  // elements of out to 16 bytes
    if (!aligned16(Q) || !aligned16(Kmat) || !aligned16(V) || !aligned16(out) || (mask && !aligned16(mask)) || ldq % 8 || ldk % 8 || ldv % 8 ||
        ldo % oq || q_head % 8 || k_head % 8 || v_head % 8 || o_head % oq)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "attn_bsr_bf16: Q, K, V, mask and out must be 16-byte aligned, and so every row and head stride (ldq=%u ldk=%u ldv=%u ldo=%u "
                    "heads %llu %llu %llu %llu)",
                    ldq, ldk, ldv, ldo, static_cast<unsigned long long>(q_head), static_cast<unsigned long long>(k_head),
                    static_cast<unsigned long long>(v_head), static_cast<unsigned long long>(o_head));
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    const uint64_t rows = static_cast<uint64_t>(numBlockRows) * bS;
    const uint64_t qs = span(rows, ldq, D) * 2u, ks = span(K, ldk, D) * 2u, vs = span(K, ldv, Dv) * 2u;
    if (qs > 0x7FFFFFFFull || ks > 0x7FFFFFFFull || vs > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "attn_bsr_bf16: Q, K or V of one head spans 2 GiB or more (%llu, %llu, %llu bytes)",
                    static_cast<unsigned long long>(qs), static_cast<unsigned long long>(ks), static_cast<unsigned long long>(vs));
    if (rows > 0x7FFFFFFFull || ceil_div64(rows / 16, kTileWaves) * H > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "attn_bsr_bf16: %llu rows x %u heads are more work units than one launch takes",
                    static_cast<unsigned long long>(rows), H);
    AttnCall c{};
    c.stream = as_stream(stream);
    c.H = H;
    c.Mb = numBlockRows;
    c.blockRowPtrs = blockRowPtrs, c.blockColIdxs = blockColIdxs;
    c.Q = Q, c.K = Kmat, c.V = V;
    c.mask = mask, c.out = out, c.lse = lse;
    AttnParams &p = c.p;
    p.Kb = K / bS, p.D = D, p.Dv = Dv, p.rows = static_cast<uint32_t>(rows);
    p.ldq2 = ldq * 2u, p.ldk2 = ldk * 2u, p.ldv2 = ldv * 2u, p.ldo = ldo;
    p.q_bytes = static_cast<uint32_t>(qs), p.k_bytes = static_cast<uint32_t>(ks), p.v_bytes = static_cast<uint32_t>(vs);
    p.q_head = q_head, p.k_head = k_head, p.v_head = v_head, p.o_head = o_head;
    p.scale = scale;
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_const<2, 4>(D <= 64 ? 2 : 4, [&](auto ds) {
            with_const<4, 8>(Dv <= 64 ? 4 : 8, [&](auto tpl) {
                with_flag(mask != nullptr, [&](auto mk) {
                    with_flag(out_bf16 != 0, [&](auto ob) {
                        launch_attn<decltype(bs)::value, decltype(ds)::value, decltype(tpl)::value, decltype(mk)::value, decltype(ob)::value>(c);
                    });
                });
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
