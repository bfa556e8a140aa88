// libmispmm_attn_fp8_decode.so: decode attention on a paged e4m3 KV cache (include/mispmm_attn_fp8_decode.h) -- one query token
// per sequence, H query heads over H / G KV heads, a page list per sequence -- with the G query heads of a KV group PACKED into
// the 16 rows of one MFMA tile.  Bent into ../split/attn_bsr_fp8_split.hip a token is a block row of 16 or 32 query rows of
// which one is real, and the G heads of a group are G waves that each load, transpose and multiply the same K / V panel.
//
// PARTIAL KERNEL.  (sequence b, KV head kvh, segment s) is one wave.  The transposed score product of ../attn_bsr_fp8.hip puts
// query row i in lane i & 15, and nothing in it makes those rows 16 tokens of one head: here row i is query head kvh * G + i of
// token b.  Lane (i, g) holds the 16 bytes 64 s + 16 g .. of that head's q, read once through ONE descriptor over the group's G
// heads (offset i * q_head); lanes with i >= G take a dropped load -- zeros -- and store nothing.  The scale is per lane:
// c_i = fl(fl(scale * q_scale[kvh * G + i]) * k_scale[kvh]), q_scale by a vector load, k_scale by a scalar one.  Everything
// else a step does is ../split/attn_bsr_fp8_split.hip's step, operation for operation (16-byte K reads feeding two MFMAs, the
// weights as e4m3 of fl(2^8 w), V through v_perm_b32 byte transposes, two named stages, page indices one step further ahead by
// scalar loads), spelled a third time for that file's reason: the other two units stay byte for byte what they are.  A row's
// arithmetic does not look at the other rows of its tile, so (b, h) has the bits that kernel gives the token alone.
// THE TAIL replaces that kernel's MASK axis and the 16 mask VGPRs of each stage.  len = min(seqLens[b], pages * bS).  A step
// whose 32 keys end past len (wave-uniform: one scalar compare in a full step) REPLACES the scores of the keys at positions
// >= len by -Inf with a select and the V rows of those keys by zero bytes before the byte transposes: what K and V hold there
// -- a cache page's uninitialised tail, NaN bytes included -- never reaches a result.  The loads themselves stay as they are
// (a page is whole inside the cache): a branch around a load would drain the queue the two stages exist to keep full.
// A sequence with no pages or len = 0 returns at once: the combine kernel writes its +0 and -Inf.
// THE GRID.  Workgroups are numbered (KV head, sequence, segment), KV head outermost, and run in XCD order (xcd_block: an XCD
// owns a contiguous run): the sequences of one KV head are adjacent, so sequences that share prefix pages pull that head's
// panel into one XCD's L2 once.  Sequences outermost would put the Hkv panels of a shared prefix B / 8 workgroups apart on
// every XCD.  4 waves to a workgroup: consecutive segments of one (sequence, KV head), disjoint K / V panels, Q through L1.
// No LDS, no barrier, no atomics.
//
// WORKSPACE (floats), sized by the G real rows.  item = (b * Hkv + kvh) * S + s.  O: [items][G][Dv] from the start; then the
// states: [items][3][G] = m, l, lx.
//
// COMBINE KERNEL.  ../split/attn_bsr_fp8_split.hip's over (b, h) rows: 256 threads take 8 rows, 32 threads to a row.  The 8
// rows may belong to different sequences, so every row lists its own non-empty segments: its 32 threads ballot s = j and
// s = j + 32 and take their half of the wave's mask.  The rows' threads fetch the listed states into LDS; thread 0 of each row
// forms M, the weights, l and lx (s ascending, every sum starting from its first term) and writes lse [B][H]; then every thread
// streams its run of 4 columns of the listed O partials as 16-byte loads and stores fl(fl(O * (1 / l)) * v_scale[h / G]) to
// out [B][H][Dv].  No thread leaves before the last barrier.
#include "../../fused/attn_bsr_tiles.hpp"
#include "mispmm_attn_fp8_decode.h"

namespace mispmm {

namespace {

constexpr uint32_t kMaxSplits = 64;
constexpr uint32_t kMaxGroup = 16;    // the rows of an MFMA tile
constexpr uint32_t kCombineRows = 8;  // (b, h) rows to a workgroup of the combine kernel, 32 threads each

struct DecodeParams {
    uint32_t units, wgs_per_head, total, xcd_chunk;  // units: work items of one KV head = B * S (finish_grid, its "head" the KV head)
    uint32_t Kb, D, Dv, Hkv;                         // Kb: pages the cache holds
    uint32_t ldq, ldk, ldv, S;                       // row strides in elements = bytes; ldq: from token to token
    uint32_t q_bytes, k_bytes, v_bytes, G;           // q_bytes: the G heads of one group of one token; k, v: one head
    float scale;
    uint32_t q_head32;                               // q_head as a lane multiplies it: (G - 1) * q_head + D < 2 GiB (G = 1: never used)
    uint64_t q_head, k_head, v_head;                 // elements
};

constexpr float kWeightScale = 256.f;  // the weights enter e4m3 times 2^8

// rows r0 .. r3 hold byte j = tile j; out[j] holds byte e = row e of tile j
__device__ __forceinline__ void transpose4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t (&out)[4]) {
    const uint32_t lo01 = __builtin_amdgcn_perm(r1, r0, 0x05010400u);  // {r0.b0, r1.b0, r0.b1, r1.b1}
    const uint32_t hi01 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);  // {r0.b2, r1.b2, r0.b3, r1.b3}
    const uint32_t lo23 = __builtin_amdgcn_perm(r3, r2, 0x05010400u);
    const uint32_t hi23 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
    out[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

// the two 8-byte operands of a 16-byte read: the low half goes to one MFMA, the high half to the next
__device__ __forceinline__ long low8(u32x4_t v) { return __builtin_bit_cast(long, u32x2_t{v[0], v[1]}); }
__device__ __forceinline__ long high8(u32x4_t v) { return __builtin_bit_cast(long, u32x2_t{v[2], v[3]}); }

__device__ __forceinline__ f32x4_t mfma8(long a, long b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0); }

// first step of segment s of a sequence of n = q * S + r steps: floor(s n / S) without a 64-bit product (s <= S <= 64, r < S)
__device__ __forceinline__ uint32_t seg_start(uint32_t s, uint32_t q, uint32_t r, uint32_t S) { return s * q + s * r / S; }

// the unmasked keys of a sequence of `pages` pages (pages * BS < 2^31: the host declines more)
__device__ __forceinline__ uint32_t seq_len(const uint32_t *__restrict__ seqLens, uint32_t b, uint32_t pages, uint32_t bs) {
    return seqLens ? min(seqLens[b], pages * bs) : pages * bs;
}

// BS: page size.  LEN: seqLens is given.  DS: 64-column steps of D held (D <= 64 DS).  TPL: accumulator tiles = consecutive V
// bytes per lane (Dv <= 16 TPL).  The arrays are kernel arguments of their own, `const __restrict__`: page indices, lengths and
// k_scale come by scalar loads.
template <int BS, bool LEN, int DS, int TPL>
__global__ void __launch_bounds__(64 * kTileWaves)
    attn_decode_fp8_kernel(const DecodeParams p, const uint32_t *__restrict__ pagePtrs, const uint32_t *__restrict__ pageIdxs,
                           const uint32_t *__restrict__ seqLens, const uint8_t *__restrict__ Q, const uint8_t *__restrict__ K,
                           const uint8_t *__restrict__ V, const float *__restrict__ q_scale, const float *__restrict__ k_scale,
                           float *__restrict__ ws_o, float *__restrict__ ws_state) {
    static_assert((BS == 16 || BS == 32) && (DS == 1 || DS == 2) && (TPL == 4 || TPL == 8), "the instances of the header");
    using W = Walk<BS>;
    constexpr int VW = TPL / 4;  // dwords of one V row read
    constexpr uint32_t kSecond = W::kSecond, EPS = W::EPS;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wg = xcd_block(blockIdx.x, p.xcd_chunk);
    if (wg >= p.total) return;
    // (KV head, sequence, segment): the sequences of one KV head are neighbours
    const uint32_t kvh = wg / p.wgs_per_head;
    const uint32_t idx = (wg - kvh * p.wgs_per_head) * kTileWaves + wave;
    if (idx >= p.units) return;
    const uint32_t b = idx / p.S, seg = idx - b * p.S;
    const uint32_t i = lane & 15, g = lane >> 4;
    const uint32_t rs = pagePtrs[b], re = pagePtrs[b + 1];
    if (re <= rs) return;  // a sequence without pages: the combine kernel writes its zeros
    uint32_t len = 0;
    if constexpr (LEN) {
        len = seq_len(seqLens, b, re - rs, BS);
        if (len == 0) return;  // a sequence without keys: as above
    }
    const uint32_t n = (re - rs + EPS - 1) / EPS, nq = n / p.S, nr = n - nq * p.S;
    const uint32_t lo = seg_start(seg, nq, nr, p.S), hi = seg_start(seg + 1, nq, nr, p.S);
    if (hi <= lo) return;  // an empty segment writes nothing
    const uint32_t bs = rs + lo * EPS, be = min(re, rs + hi * EPS);  // the segment as a page list of its own: rs <= bs < be <= re
    const float ninf = -__builtin_huge_valf();
    const bool real = i < p.G;  // the lane's row of the tile is a query head

    f32x4_t acc[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto settle_acc = [&] { settle<TPL>(acc); };

    // c_i = fl(fl(scale * q_scale[kvh * G + i]) * k_scale[kvh]): the products of c_h in its order; a NULL scale is no multiply
    // (a lane without a head reads the group's last scale: inside the array, never stored)
    float c_i = p.scale;
    if (q_scale) c_i = c_i * q_scale[kvh * p.G + min(i, p.G - 1u)];
    if (k_scale) c_i = c_i * k_scale[kvh];

    const rsrc_t qr = make_rsrc(Q + static_cast<size_t>(b) * p.ldq + static_cast<size_t>(kvh) * p.G * p.q_head, p.q_bytes),
                 kr = make_rsrc(K + kvh * p.k_head, p.k_bytes), vr = make_rsrc(V + kvh * p.v_head, p.v_bytes);
    const uint32_t dcol = g * 16u;  // the lane's 16 columns of a 64-column step of D
    u32x4_t qf[DS];
    uint32_t koff[DS], voff[4];
#pragma unroll
    for (int s = 0; s < DS; ++s) {
        const bool in = s * 64u + dcol < p.D;  // all 16 columns or none: D is a multiple of 16
        qf[s] = __builtin_amdgcn_raw_buffer_load_b128(qr, in && real ? i * p.q_head32 + s * 64u + dcol : kDropLoad, 0, 0);  // < 2 GiB: the host declines more
        koff[s] = in ? i * p.ldk + s * 64u + dcol : kDropLoad;
    }
    const uint32_t vcol = i * TPL;  // first of the lane's TPL V columns, one per accumulator tile
#pragma unroll
    for (int j = 0; j < 4; ++j) voff[j] = vcol < p.Dv ? (4u * g + j) * p.ldv + vcol : kDropLoad;

    // the pages behind the two 16-key tiles of the step that starts at list entry e (bS = 32: one page); past the segment's end: none
    struct Cols {
        uint32_t a, b;
    };
    const uint32_t last = be - 1;
    auto cols_at = [&](uint32_t e) {
        const uint32_t ca = pageIdxs[min(e, last)];
        if constexpr (BS == 16) {
            const uint32_t cb = pageIdxs[min(e + 1, last)];
            return Cols{e < be ? ca : 0xFFFFFFFFu, e + 1 < be ? cb : 0xFFFFFFFFu};
        } else {
            return Cols{e < be ? ca : 0xFFFFFFFFu, e < be ? ca : 0xFFFFFFFFu};
        }
    };
    // everything a step reads, fetched one step ahead: K's 16-byte fragments, V's rows
    struct Stage {
        u32x4_t k[2][DS];
        uint32_t v[8][VW];
    };
    auto load_stage = [&](Cols c, Stage &st) {
        const bool va = c.a < p.Kb, vb = c.b < p.Kb;  // wave-uniform
        const uint32_t ra = va ? c.a * BS : 0u, rb = vb ? c.b * BS + kSecond : 0u;
#pragma unroll
        for (int s = 0; s < DS; ++s) {
            st.k[0][s] = __builtin_amdgcn_raw_buffer_load_b128(kr, va ? koff[s] : kDropLoad, ra * p.ldk, 0);
            st.k[1][s] = __builtin_amdgcn_raw_buffer_load_b128(kr, vb ? koff[s] : kDropLoad, rb * p.ldk, 0);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t vo = (j < 4 ? va : vb) ? voff[j & 3] : kDropLoad, so = (j < 4 ? ra : rb) * p.ldv;
            if constexpr (TPL == 8) {
                const auto r = __builtin_amdgcn_raw_buffer_load_b64(vr, vo, so, 0);
                st.v[j][0] = r[0];
                st.v[j][1] = r[1];
            } else {
                st.v[j][0] = __builtin_amdgcn_raw_buffer_load_b32(vr, vo, so, 0);
            }
        }
    };

    float m = ninf, mu = 0.f, l = 0.f, lx = 0.f;
    uint32_t e = bs;
    Cols nxt = cols_at(e + EPS);

    // the step of ../split/attn_bsr_fp8_split.hip's nomask instance, operation for operation, and the tail's two selects
    auto step = [&](const Stage &use, Stage &fill) {
        const Cols after = cols_at(e + 2 * EPS);
        load_stage(nxt, fill);
        const bool second = BS == 32 || e + 1 < be;  // wave-uniform: a half step (the sequence's last) has no second tile
        // per tile: columns 64 s + 16 g + 0 .. 7, then + 8 .. 15, s ascending; the two tiles' chains interleaved
        f32x4_t sa{0.f, 0.f, 0.f, 0.f}, sb{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DS; ++s) {
            sa = mfma8(low8(use.k[0][s]), low8(qf[s]), sa);
            sb = mfma8(low8(use.k[1][s]), low8(qf[s]), sb);
            sa = mfma8(high8(use.k[0][s]), high8(qf[s]), sa);
            sb = mfma8(high8(use.k[1][s]), high8(qf[s]), sb);
        }
        float z[8];
        uint32_t vrow[8][VW];  // V's rows as they enter the second product
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            z[j] = c_i * sa[j];
            z[4 + j] = second ? c_i * sb[j] : ninf;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int w = 0; w < VW; ++w) vrow[j][w] = use.v[j][w];
        if constexpr (LEN) {
            const uint32_t kpos = (e - rs) * BS;  // the step's first key in the sequence's key order
            if (kpos + 32u > len) {               // wave-uniform: the step holds a masked key
                // the lane's keys: 4 g + j of the first tile, 16 + 4 g + j of the second; unmasked where kpos + that < len
                const int rem = static_cast<int>(len) - static_cast<int>(kpos) - static_cast<int>(4u * g);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ka = j < rem, kb = 16 + j < rem;
                    z[j] = ka ? z[j] : ninf;
                    z[4 + j] = kb ? z[4 + j] : ninf;
#pragma unroll
                    for (int w = 0; w < VW; ++w) {
                        vrow[j][w] = ka ? vrow[j][w] : 0u;
                        vrow[4 + j][w] = kb ? vrow[4 + j][w] : 0u;
                    }
                }
            }
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
        // the lane's 8 weights: unrounded into tx, times 2^8 into the two dwords of the B operand, read back into t
        uint32_t pw[2] = {0u, 0u};
        float t = 0.f, tx = 0.f;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            float pz[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pz[j] = tile_exp(z[4 * w + j] - mu);
                tx = tx + pz[j];
            }
            int d = __builtin_amdgcn_cvt_pk_fp8_f32(pz[0] * kWeightScale, pz[1] * kWeightScale, 0, false);
            d = __builtin_amdgcn_cvt_pk_fp8_f32(pz[2] * kWeightScale, pz[3] * kWeightScale, d, true);
            const auto lo8 = __builtin_amdgcn_cvt_pk_f32_fp8(d, false), hi8 = __builtin_amdgcn_cvt_pk_f32_fp8(d, true);
            t = t + lo8[0];
            t = t + lo8[1];
            t = t + hi8[0];
            t = t + hi8[1];
            pw[w] = static_cast<uint32_t>(d);
        }
        t = t + (tx - tx);  // +0, or NaN where a weight is +Inf or NaN: the row is NaN whatever the converter made of it
        l = l * alpha + t;
        lx = lx * alpha + tx;
        settle_acc();
#pragma unroll
        for (int tt = 0; tt < TPL; ++tt) acc[tt] = acc[tt] * alpha;
        const long pfrag = __builtin_bit_cast(long, u32x2_t{pw[0], pw[1]});
#pragma unroll
        for (int w = 0; w < VW; ++w) {
            uint32_t tl[4], th[4];
            transpose4(vrow[0][w], vrow[1][w], vrow[2][w], vrow[3][w], tl);
            transpose4(vrow[4][w], vrow[5][w], vrow[6][w], vrow[7][w], th);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * w + j] = mfma8(__builtin_bit_cast(long, u32x2_t{tl[j], th[j]}), pfrag, acc[4 * w + j]);
        }
        nxt = after;
        e += EPS;
    };

    // two stages in turn (a copy `cur = nxt` would wait for the loads it is meant to hide)
    Stage s0, s1;
    load_stage(cols_at(e), s0);
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
    if (!real) return;
    // item < B * Hkv * S, i < G and col + TPL <= Dv: inside the O part of the workspace the host sized
    const size_t item = (static_cast<size_t>(b) * p.Hkv + kvh) * p.S + seg;
    const size_t base = (item * p.G + i) * p.Dv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t col = TPL * (4u * g + k);
        if (col < p.Dv) store_run<TPL>(acc, k, 1.f, ws_o, base, col, false);
    }
    if (g == 0) {
        float *st = ws_state + item * 3u * p.G + i;
        st[0] = m;
        st[p.G] = l;
        st[2u * p.G] = lx;
    }
}

struct DecodeCombineParams {
    uint32_t rows, H, Hkv, G, S, Dv, ldo, eps, bs;  // rows = B * H; eps: pages per step
    uint64_t o_head;                                // elements
};

template <bool OUT_BF16>
__global__ void __launch_bounds__(32 * kCombineRows)
    attn_decode_fp8_combine_kernel(const DecodeCombineParams p, const uint32_t *__restrict__ pagePtrs, const uint32_t *__restrict__ seqLens,
                                   const float *__restrict__ ws_o, const float *__restrict__ ws_state, const float *__restrict__ v_scale,
                                   void *__restrict__ out, float *__restrict__ lse_out) {
    __shared__ uint32_t s_list[kCombineRows][kMaxSplits], s_count[kCombineRows];
    __shared__ float s_m[kCombineRows][kMaxSplits], s_l[kCombineRows][kMaxSplits], s_lx[kCombineRows][kMaxSplits], s_w[kCombineRows][kMaxSplits];
    __shared__ float s_inv[kCombineRows];
    const uint32_t rw = threadIdx.x >> 5, j = threadIdx.x & 31;
    const uint32_t want = blockIdx.x * kCombineRows + rw;
    const bool there = want < p.rows;              // the last workgroup may hold fewer than 8 rows
    const uint32_t row = there ? want : p.rows - 1u;  // such threads follow the last row and store nothing
    const uint32_t b = row / p.H, h = row - b * p.H;
    const uint32_t kvh = h / p.G, i = h - kvh * p.G;
    const uint32_t pages = pagePtrs[b + 1] - pagePtrs[b];
    const bool empty = static_cast<int32_t>(pages) <= 0 || seq_len(seqLens, b, pages, p.bs) == 0;
    const uint32_t col = 4u * j;
    const size_t o_at = static_cast<size_t>(b) * p.ldo + static_cast<size_t>(h) * p.o_head + col;
    auto store = [&](f32x4_t v) {
        if (!there || col >= p.Dv) return;
        if constexpr (OUT_BF16) {
            const uint32_t o0 = __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(v[0]), static_cast<__bf16>(v[1])});
            const uint32_t o1 = __builtin_bit_cast(uint32_t, bf2{static_cast<__bf16>(v[2]), static_cast<__bf16>(v[3])});
            *reinterpret_cast<u32x2_t *>(static_cast<uint16_t *>(out) + o_at) = u32x2_t{o0, o1};
        } else {
            *reinterpret_cast<f32x4_t *>(static_cast<float *>(out) + o_at) = v;
        }
    };
    // the row's non-empty segments, ascending: s = j, then s = j + 32, each row taking its 32 bits of the wave's ballot
    {
        const uint32_t n = (pages + p.eps - 1) / p.eps, nq = n / p.S, nr = n - nq * p.S;
        const uint32_t half = (rw & 1u) * 32u;
        const bool live_lo = !empty && j < p.S && seg_start(j, nq, nr, p.S) < seg_start(j + 1, nq, nr, p.S);
        const bool live_hi = !empty && j + 32u < p.S && seg_start(j + 32u, nq, nr, p.S) < seg_start(j + 33u, nq, nr, p.S);
        const uint32_t lo = static_cast<uint32_t>(__ballot(live_lo) >> half), hi = static_cast<uint32_t>(__ballot(live_hi) >> half);
        const uint32_t below = (1u << j) - 1u;
        if (live_lo) s_list[rw][__popc(lo & below)] = j;
        if (live_hi) s_list[rw][__popc(lo) + __popc(hi & below)] = j + 32u;
        if (j == 0) s_count[rw] = __popc(lo) + __popc(hi);
    }
    __syncthreads();
    const uint32_t count = s_count[rw];  // 0 for a sequence without keys, else >= 1
    const size_t item0 = (static_cast<size_t>(b) * p.Hkv + kvh) * p.S;
    for (uint32_t k = j; k < count; k += 32) {
        const float *st = ws_state + (item0 + s_list[rw][k]) * 3u * p.G + i;
        s_m[rw][k] = st[0];
        s_l[rw][k] = st[p.G];
        s_lx[rw][k] = st[2u * p.G];
    }
    __syncthreads();
    if (j == 0 && count != 0) {  // the merge of the header, steps 1 to 4 for l and lx
        const float inf = __builtin_huge_valf();
        float M = s_m[rw][0];
        for (uint32_t k = 1; k < count; ++k) M = __builtin_fmaxf(M, s_m[rw][k]);
        const float mu = __builtin_fabsf(M) == inf ? 0.f : M;
        float l = 0.f, lx = 0.f;
        for (uint32_t k = 0; k < count; ++k) {
            const float ms = s_m[rw][k];
            const float mus = __builtin_fabsf(ms) == inf ? 0.f : ms;
            const float w = ms == -inf ? 1.f : tile_exp(mus - mu);
            s_w[rw][k] = w;
            const float tl = w * s_l[rw][k], tlx = w * s_lx[rw][k];
            l = k == 0 ? tl : l + tl;
            lx = k == 0 ? tlx : lx + tlx;
        }
        s_inv[rw] = 1.f / l;
        if (lse_out && there) lse_out[row] = mu + __builtin_logf(lx);
    }
    __syncthreads();
    if (count == 0) {  // a sequence without unmasked keys: +0 whatever v_scale holds, lse = log 0
        store(f32x4_t{0.f, 0.f, 0.f, 0.f});
        if (lse_out && there && j == 0) lse_out[row] = -__builtin_huge_valf();
        return;
    }
    if (col >= p.Dv) return;
    const size_t stride = static_cast<size_t>(p.G) * p.Dv;  // floats between the same row of two segments
    const float *src = ws_o + (item0 * p.G + i) * p.Dv + col;
    f32x4_t o = *reinterpret_cast<const f32x4_t *>(src + s_list[rw][0] * stride) * s_w[rw][0];
#pragma unroll 4
    for (uint32_t k = 1; k < count; ++k) o = o + *reinterpret_cast<const f32x4_t *>(src + s_list[rw][k] * stride) * s_w[rw][k];
    // out = fl(fl(O * inv) * vs): two multiplies; a NULL v_scale: the first alone
    o = o * s_inv[rw];
    if (v_scale) o = o * v_scale[kvh];
    store(o);
}

struct DecodeCall {
    hipStream_t stream;
    uint32_t B, Hkv;
    DecodeParams p;
    DecodeCombineParams c;
    const uint32_t *pagePtrs, *pageIdxs, *seqLens;
    const uint8_t *Q, *K, *V;
    const float *q_scale, *k_scale, *v_scale;
    float *ws_o, *ws_state;
    void *out;
    float *lse;
};

template <int BS, bool LEN, int DS, int TPL>
void launch_partial(const DecodeCall &c) {
    DecodeParams p = c.p;
    const uint32_t grid = finish_grid(p, c.B * p.S, c.Hkv);
    note_kernel("attn_decode_fp8<b%d,%s,D%d,T%d,S%u>", BS, LEN ? "len" : "full", DS, TPL, p.S);
    hipLaunchKernelGGL((attn_decode_fp8_kernel<BS, LEN, DS, TPL>), dim3(grid), dim3(64 * kTileWaves), 0, c.stream, p, c.pagePtrs, c.pageIdxs,
                       c.seqLens, c.Q, c.K, c.V, c.q_scale, c.k_scale, c.ws_o, c.ws_state);
}

template <bool OUT_BF16>
void launch_combine(const DecodeCall &c) {
    const uint32_t grid = ceil_div(c.c.rows, kCombineRows);
    note_kernel("attn_decode_fp8_combine<%s,S%u>", OUT_BF16 ? "bf16" : "f32", c.c.S);
    hipLaunchKernelGGL((attn_decode_fp8_combine_kernel<OUT_BF16>), dim3(grid), dim3(32 * kCombineRows), 0, c.stream, c.c, c.pagePtrs, c.seqLens,
                       c.ws_o, c.ws_state, c.v_scale, c.out, c.lse);
}

bool aligned4(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 3u) == 0; }

}  // namespace

}  // namespace mispmm

using namespace mispmm;

extern "C" uint64_t mispmm_attn_decode_fp8_workspace(uint32_t B, uint32_t H, uint32_t kv_group, uint32_t Dv, uint32_t splits) {
    return static_cast<uint64_t>(B) * H * splits * (static_cast<uint64_t>(Dv) + 3u) * 4u;  // the G real rows of every tile: kv_group cancels
}

extern "C" int mispmm_attn_decode_fp8(mispmm_stream_t stream, uint32_t B, uint32_t H, uint32_t K, uint32_t bS, uint32_t numPages,
                                      const uint32_t *pagePtrs, const uint32_t *pageIdxs, const uint32_t *seqLens, const uint8_t *Q, uint32_t ldq,
                                      uint64_t q_head, const uint8_t *Kmat, uint32_t ldk, uint64_t k_head, const uint8_t *V, uint32_t ldv,
                                      uint64_t v_head, uint32_t D, uint32_t Dv, float scale, const float *q_scale, const float *k_scale,
                                      const float *v_scale, void *out, uint32_t ldo, uint64_t o_head, int out_bf16, float *lse, uint32_t kv_group,
                                      uint32_t splits, void *workspace, uint64_t workspace_bytes) {
    constexpr const char *fn = "attn_decode_fp8";
    if (const int refused = refuse_shape(fn, bS, scale, D, Dv, K)) return refused;
    if (D % 16 != 0)  // a lane reads 16 bytes of a row of Q or K: wholly inside D or wholly dropped
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: D must be a multiple of 16 from 16 to 128 (got D=%u)", fn, D);
    if (kv_group == 0) return fail(MISPMM_ERR_INVALID_ARG, "%s: kv_group must be 1 to %u and divide H (got kv_group=0, H=%u)", fn, kMaxGroup, H);
    if (kv_group > kMaxGroup)  // the heads of a group are the rows of one 16-row tile
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: kv_group above %u is not supported (got kv_group=%u)", fn, kMaxGroup, kv_group);
    if (H % kv_group != 0)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: kv_group must be 1 to %u and divide H (got kv_group=%u, H=%u)", fn, kMaxGroup, kv_group, H);
    if (splits == 0 || splits > kMaxSplits) return fail(MISPMM_ERR_INVALID_ARG, "%s: splits must be 1 to %u (got %u)", fn, kMaxSplits, splits);
    const uint64_t need = mispmm_attn_decode_fp8_workspace(B, H, kv_group, Dv, splits);
    if (!workspace || !aligned16(workspace) || workspace_bytes < need)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: the workspace must be 16-byte aligned and hold %llu bytes (got %s, %llu bytes)", fn,
                    static_cast<unsigned long long>(need), !workspace ? "null" : aligned16(workspace) ? "an aligned pointer" : "a misaligned pointer",
                    static_cast<unsigned long long>(workspace_bytes));
    if (B == 0 || H == 0) return MISPMM_OK;
    if (!pagePtrs || !Q || !Kmat || !V || !out || (numPages != 0 && !pageIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: pagePtrs, pageIdxs, Q, K, V or out is null", fn);
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)", fn, D, ldq,
                    ldk, Dv, ldv, ldo);
    // a lane reads 16 bytes of Q and K and 8 (T4: 4) of V; a combine thread writes 4 columns: 16 bytes of fp32, 8 of bf16 (the
    // alignment of mispmm_attn_bsr_fp8)
    const uint32_t oq = out_bf16 ? 8u : 4u;
    if (!aligned16(Q) || !aligned16(Kmat) || !aligned8(V) || !aligned16(out) || ldq % 16 || ldk % 16 || ldv % 8 || ldo % oq || q_head % 16 ||
        k_head % 16 || v_head % 8 || o_head % oq)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "%s: Q, K and out must be 16-byte aligned and V 8-byte, and so every row and head stride (ldq=%u ldk=%u ldv=%u ldo=%u "
                    "heads %llu %llu %llu %llu)",
                    fn, ldq, ldk, ldv, ldo, static_cast<unsigned long long>(q_head), static_cast<unsigned long long>(k_head),
                    static_cast<unsigned long long>(v_head), static_cast<unsigned long long>(o_head));
    if (!aligned4(q_scale) || !aligned4(k_scale) || !aligned4(v_scale) || !aligned4(pagePtrs) || !aligned4(pageIdxs) || !aligned4(seqLens))
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: q_scale, k_scale, v_scale, pagePtrs, pageIdxs and seqLens must be 4-byte aligned", fn);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load; Q's covers the G heads of a group
    const uint64_t qs = kv_group == 1 ? D : q_head > 0x7FFFFFFFull ? 0x80000000ull : span(kv_group, static_cast<uint32_t>(q_head), D);
    const uint64_t ks = span(K, ldk, D), vs = span(K, ldv, Dv);
    if (qs > 0x7FFFFFFFull || ks > 0x7FFFFFFFull || vs > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: the heads of a KV group of Q, or K or V of one head, span 2 GiB or more (%llu, %llu, %llu bytes)",
                    fn, static_cast<unsigned long long>(qs), static_cast<unsigned long long>(ks), static_cast<unsigned long long>(vs));
    const uint32_t Hkv = H / kv_group;
    const uint64_t items = static_cast<uint64_t>(B) * splits;  // of one KV head
    if (items > 0xFFFFFFFFull || ceil_div64(items, kTileWaves) * Hkv > 0x7FFFFFFFull || static_cast<uint64_t>(B) * H > 0x7FFFFFFFull ||
        static_cast<uint64_t>(numPages) * bS > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: %u sequences x %u heads x %u splits over %u pages are more work units than one launch takes", fn,
                    B, H, splits, numPages);
    DecodeCall c{};
    c.stream = as_stream(stream);
    c.B = B, c.Hkv = Hkv;
    c.pagePtrs = pagePtrs, c.pageIdxs = pageIdxs, c.seqLens = seqLens;
    c.Q = Q, c.K = Kmat, c.V = V;
    c.q_scale = q_scale, c.k_scale = k_scale, c.v_scale = v_scale;
    c.out = out, c.lse = lse;
    c.ws_o = static_cast<float *>(workspace);
    c.ws_state = c.ws_o + static_cast<uint64_t>(B) * H * splits * Dv;
    DecodeParams &p = c.p;
    p.Kb = K / bS, p.D = D, p.Dv = Dv, p.Hkv = Hkv, p.S = splits, p.G = kv_group;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv;
    p.q_bytes = static_cast<uint32_t>(qs), p.k_bytes = static_cast<uint32_t>(ks), p.v_bytes = static_cast<uint32_t>(vs);
    p.q_head = q_head, p.k_head = k_head, p.v_head = v_head;
    p.q_head32 = kv_group == 1 ? 0u : static_cast<uint32_t>(q_head);
    p.scale = scale;
    c.c = DecodeCombineParams{B * H, H, Hkv, kv_group, splits, Dv, ldo, bS == 16 ? 2u : 1u, bS, o_head};
    with_const<16, 32>(static_cast<int>(bS), [&](auto bs) {
        with_flag(seqLens != nullptr, [&](auto ln) {
            with_const<1, 2>(D <= 64 ? 1 : 2, [&](auto ds) {
                with_const<4, 8>(Dv <= 64 ? 4 : 8, [&](auto tpl) {
                    launch_partial<decltype(bs)::value, decltype(ln)::value, decltype(ds)::value, decltype(tpl)::value>(c);
                });
            });
        });
    });
    MISPMM_LAUNCH_CHECK();
    with_flag(out_bf16 != 0, [&](auto ob) { launch_combine<decltype(ob)::value>(c); });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
