// The entry points of the fused attention on a CSR pattern, host only, written once over the element policy of elem.hpp:
// fwd_entry (attn_csr.hip, attn_csr_bf16/attn_csr_bf16.hip), bwd_entry (bwd/attn_csr_bwd.hip, attn_csr_bf16/bwd/) and
// dbias_entry (attn_csr_dbias/attn_csr_dbias.hip).  Each unit keeps its extern "C" functions, which forward here with the name
// that begins their messages and their note_kernel tags; an fp32 export passes 0 for the out_bf16 / grads_bf16 its ABI lacks.
// An entry is its refusals in the order the headers document (shape; the no-op returns; nulls; leading dimensions; spans; the
// lane width; grid; 2-byte alignment; overlap), then the parameter block.  What two or three entries share stands once below:
// over2g (the span test), Reads (what the backward and the bias gradient both read: spans, width rule, extents, block fields),
// writes_wide (the rule for a written gradient) and aligned2s.  What they do NOT share, as found and kept (DESIGN.md section 9
// item 27):
//  - the forward holds ldo and out_head_stride to the operands' wide lane width (8 for bf16 also where out is fp32); the
//    backward and the bias gradient hold out to 4, and a gradient to 8 or 4 by its own type;
//  - FwdParams<ElemF32> keeps Q's row stride in elements (kFwdLdqUnit), every other row stride of every block is in bytes;
//  - the forward has no overlap check; the backward's input extents leave out the pattern, the bias gradient's hold it;
//  - the bias gradient is a no-op on nnz == 0 and wants colIdxs always, the others want it where nnz != 0.
// The parameter blocks are the kernels' own and are only filled here: nothing in this header reaches device code.
#pragma once
#include <initializer_list>

#include "attn_csr_bwd.hpp"
#include "attn_csr_dbias.hpp"
#include "attn_csr_fwd.hpp"

namespace mispmm {

namespace {

using ull = unsigned long long;

// a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load: one head's spans, in elements of
// `elem` bytes (span > limit / elem is span * elem > limit for 2 and for 4, and has no product to wrap)
inline bool over2g(uint64_t elem, std::initializer_list<uint64_t> spans) {
    for (const uint64_t s : spans)
        if (s > 0x7FFFFFFFull / elem) return true;
    return false;
}
inline bool mult(uint64_t x, uint64_t m) { return x % m == 0; }
// a gradient that is asked for keeps 16-byte lanes if its strides are multiples of `m` elements and its base is aligned
inline bool writes_wide(const void *d, uint32_t ldd, uint64_t head_stride, uint64_t m) {
    return !d || (mult(ldd, m) && mult(head_stride, m) && aligned16(d));
}
inline bool aligned2s(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (!aligned2(p)) return false;
    return true;
}

// Q's row stride as FwdParams<Elem>::q_row() takes it
template <class Elem> constexpr uint32_t kFwdLdqUnit = Elem::kBytes;
template <> constexpr uint32_t kFwdLdqUnit<ElemF32> = 1;

template <class Elem>
int fwd_entry(const char *name, const char *tag, mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz,
              const uint32_t *rowPtrs, const uint32_t *colIdxs, const typename Elem::in_t *Q, uint64_t q_head_stride, uint32_t ldq,
              const typename Elem::in_t *Kmat, uint64_t k_head_stride, uint32_t ldk, uint32_t D, const typename Elem::in_t *V,
              uint64_t v_head_stride, uint32_t ldv, uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride,
              typename Elem::out_t *out, uint64_t out_head_stride, uint32_t ldo, int out_bf16, float *lse) {
    constexpr uint64_t EB = Elem::kBytes, WIDE = Elem::kWide;
    if (const int st = refuse_shape(name, D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0) return MISPMM_OK;
    if (!rowPtrs || !Q || !Kmat || !V || !out || (nnz != 0 && !colIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: rowPtrs, colIdxs, Q, K, V or out is null", name);
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)", name, D,
                    ldq, ldk, Dv, ldv, ldo);
    const uint64_t o_elem = out_bf16 ? 2u : 4u;
    const uint64_t qs = span(M, ldq, D), ks = span(K, ldk, D), vs = span(K, ldv, Dv), os = span(M, ldo, Dv);
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) : 0u;
    if (over2g(EB, {qs, ks, vs}) || over2g(o_elem, {os}) || over2g(4, {bs}))
        return fail(MISPMM_ERR_UNSUPPORTED, "%s: Q, K, V, out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu bytes)", name,
                    static_cast<ull>(qs * EB), static_cast<ull>(ks * EB), static_cast<ull>(vs * EB), static_cast<ull>(os * o_elem),
                    static_cast<ull>(bs * 4u));
    const bool wide = D % WIDE == 0 && Dv % WIDE == 0 && mult(ldq, WIDE) && mult(ldk, WIDE) && mult(ldv, WIDE) && mult(ldo, WIDE) &&
                      mult(q_head_stride, WIDE) && mult(k_head_stride, WIDE) && mult(v_head_stride, WIDE) && mult(out_head_stride, WIDE) &&
                      aligned16(Q) && aligned16(Kmat) && aligned16(V) && aligned16(out);
    const int vec = wide ? Elem::kWide : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid(name, M, H, g); st != MISPMM_OK) return st;
    if (EB == 2 && !(aligned2s({Q, Kmat, V}) && (!out_bf16 || aligned2(out))))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: Q, K, V and a bf16 out must be 2-byte aligned", name);
    FwdCall<Elem> c{};
    c.stream = as_stream(stream);
    c.H = H;
    c.rowPtrs = rowPtrs, c.colIdxs = colIdxs;
    c.Q = Q, c.K = Kmat, c.V = V, c.bias = bias, c.out = out, c.lse = lse;
    FwdParams<Elem> &p = c.p;
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq = ldq * kFwdLdqUnit<Elem>, p.ldk = static_cast<uint32_t>(ldk * EB), p.ldv = static_cast<uint32_t>(ldv * EB), p.ldo = ldo;
    p.q_bytes = static_cast<uint32_t>(qs * EB), p.k_bytes = static_cast<uint32_t>(ks * EB), p.v_bytes = static_cast<uint32_t>(vs * EB);
    p.bias_bytes = static_cast<uint32_t>(bs * 4u);
    if constexpr (Elem::kWidens) p.narrow = out_bf16 ? 1u : 0u;
    p.scale = scale;
    p.q_head = q_head_stride, p.k_head = k_head_stride, p.v_head = v_head_stride, p.o_head = out_head_stride, p.bias_head = bias_head_stride;
    Elem::with_instance(vec, g, width, [&](auto gr, auto v, auto ch) {
        launch_attn_csr<Elem, decltype(gr)::value, decltype(v)::value, decltype(ch)::value>(c, tag);
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}

// what the backward and the bias gradient both read: Q, K, V and grad_out of the element type, out, lse and the bias in fp32
template <class Elem>
struct Reads {
    static constexpr uint64_t EB = Elem::kBytes, WIDE = Elem::kWide;
    using in_t = typename Elem::in_t;
    uint32_t H, M, K, nnz, D, Dv;
    const in_t *Q;
    uint64_t q_head;
    uint32_t ldq;
    const in_t *Kmat;
    uint64_t k_head;
    uint32_t ldk;
    const in_t *V;
    uint64_t v_head;
    uint32_t ldv;
    float scale;
    const float *bias;
    uint64_t bias_head;
    const float *out;
    uint64_t o_head;
    uint32_t ldo;
    const float *lse;
    const in_t *dO;
    uint64_t g_head;
    uint32_t ldg;
    uint64_t qs, ks, vs, os, gs, bs;  // one head's spans in elements: measure()

    bool short_ld() const { return ldq < D || ldk < D || ldv < Dv || ldo < Dv || ldg < Dv; }
    int measure(const char *name) {
        qs = span(M, ldq, D), ks = span(K, ldk, D), vs = span(K, ldv, Dv), os = span(M, ldo, Dv), gs = span(M, ldg, Dv);
        bs = bias ? static_cast<uint64_t>(nnz) : 0u;
        if (over2g(EB, {qs, ks, vs, gs}) || over2g(4, {os, bs}))
            return fail(MISPMM_ERR_UNSUPPORTED,
                        "%s: Q, K, V, out, grad_out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu, %llu bytes)", name,
                        static_cast<ull>(qs * EB), static_cast<ull>(ks * EB), static_cast<ull>(vs * EB), static_cast<ull>(os * 4u),
                        static_cast<ull>(gs * EB), static_cast<ull>(bs * 4u));
        return MISPMM_OK;
    }
    // 16-byte lanes on everything read: the element operands in multiples of the wide lane width, the fp32 out in multiples of 4
    bool wide() const {
        return D % WIDE == 0 && Dv % WIDE == 0 && mult(ldq, WIDE) && mult(ldk, WIDE) && mult(ldv, WIDE) && mult(ldg, WIDE) && mult(ldo, 4) &&
               mult(q_head, WIDE) && mult(k_head, WIDE) && mult(v_head, WIDE) && mult(g_head, WIDE) && mult(o_head, 4) && aligned16(Q) &&
               aligned16(Kmat) && aligned16(V) && aligned16(out) && aligned16(dO);
    }
    bool reads_aligned2() const { return EB != 2 || aligned2s({Q, Kmat, V, dO}); }
    // the bytes of each, in its own type
    static constexpr size_t kExtents = 7;
    void extents(Extent *e) const {
        e[0] = extent(Q, H, q_head, qs, EB), e[1] = extent(Kmat, H, k_head, ks, EB), e[2] = extent(V, H, v_head, vs, EB);
        e[3] = extent(out, H, o_head, os, 4), e[4] = extent(dO, H, g_head, gs, EB), e[5] = extent(bias, H, bias_head, bs, 4);
        e[6] = extent(lse, 1, 0, static_cast<uint64_t>(H) * M, 4);
    }
    // the fields BwdParams and DbiasParams have in common, and those of BwdPtrs and DbiasPtrs
    template <class Params, class Ptrs>
    void fill(Params &p, Ptrs &a) const {
        p.M = M, p.D = D, p.Dv = Dv;
        p.ldq = static_cast<uint32_t>(ldq * EB), p.ldk = static_cast<uint32_t>(ldk * EB), p.ldv = static_cast<uint32_t>(ldv * EB);
        p.ldg = static_cast<uint32_t>(ldg * EB), p.ldo = ldo * 4u;
        p.q_bytes = static_cast<uint32_t>(qs * EB), p.k_bytes = static_cast<uint32_t>(ks * EB), p.v_bytes = static_cast<uint32_t>(vs * EB);
        p.g_bytes = static_cast<uint32_t>(gs * EB), p.o_bytes = static_cast<uint32_t>(os * 4u), p.bias_bytes = static_cast<uint32_t>(bs * 4u);
        p.scale = scale;
        p.q_head = q_head, p.k_head = k_head, p.v_head = v_head, p.g_head = g_head, p.o_head = o_head, p.bias_head = bias_head;
        a.Q = Q, a.K = Kmat, a.V = V, a.dO = dO, a.out = out, a.lse = lse, a.bias = bias;
    }
};

template <class Elem>
int bwd_entry(const char *name, const char *row_tag, const char *col_tag, mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K,
              uint32_t nnz, const uint32_t *rowPtrs, const uint32_t *colIdxs, const uint32_t *tRowPtrs, const uint32_t *tColIdxs,
              const uint32_t *perm, const typename Elem::in_t *Q, uint64_t q_head_stride, uint32_t ldq, const typename Elem::in_t *Kmat,
              uint64_t k_head_stride, uint32_t ldk, uint32_t D, const typename Elem::in_t *V, uint64_t v_head_stride, uint32_t ldv, uint32_t Dv,
              float scale, const float *bias, uint64_t bias_head_stride, const float *out, uint64_t out_head_stride, uint32_t ldo,
              const float *lse, const typename Elem::in_t *grad_out, uint64_t g_head_stride, uint32_t ldg, float *delta, int grads_bf16,
              typename Elem::out_t *dQ, uint64_t dq_head_stride, uint32_t lddq, typename Elem::out_t *dK, uint64_t dk_head_stride,
              uint32_t lddk, typename Elem::out_t *dV, uint64_t dv_head_stride, uint32_t lddv) {
    if (const int st = refuse_shape(name, D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0 || (!dQ && !dK && !dV)) return MISPMM_OK;
    const bool col_pass = (dK || dV) && K != 0;
    const bool row_pass = dQ || (dK && K != 0);  // dK reads delta
    if (!rowPtrs || !Q || !Kmat || !V || (nnz != 0 && !colIdxs)) return fail(MISPMM_ERR_INVALID_ARG, "%s: rowPtrs, colIdxs, Q, K or V is null", name);
    if (!out || !lse || !grad_out || (row_pass && !delta)) return fail(MISPMM_ERR_INVALID_ARG, "%s: out, lse, grad_out or delta is null", name);
    if (col_pass && (!tRowPtrs || (nnz != 0 && !tColIdxs)))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: dK and dV need the pattern of A^T: tRowPtrs or tColIdxs is null", name);
    if (col_pass && bias && nnz != 0 && !perm) return fail(MISPMM_ERR_INVALID_ARG, "%s: with a bias, dK and dV need perm, which is null", name);
    Reads<Elem> r{H, M, K, nnz, D, Dv, Q, q_head_stride, ldq, Kmat, k_head_stride, ldk, V, v_head_stride, ldv, scale, bias, bias_head_stride,
                  out, out_head_stride, ldo, lse, grad_out, g_head_stride, ldg, 0, 0, 0, 0, 0, 0};
    if (r.short_ld() || (dQ && lddq < D) || (dK && lddk < D) || (dV && lddv < Dv))
        return fail(MISPMM_ERR_INVALID_ARG,
                    "%s: leading dimension smaller than the width (D=%u ldq=%u ldk=%u lddq=%u lddk=%u, Dv=%u ldv=%u ldo=%u ldg=%u lddv=%u)", name, D,
                    ldq, ldk, lddq, lddk, Dv, ldv, ldo, ldg, lddv);
    if (const int st = r.measure(name); st != MISPMM_OK) return st;
    const uint64_t d_elem = grads_bf16 ? 2u : 4u, d_mult = grads_bf16 ? 8u : 4u;
    const bool wide = r.wide() && writes_wide(dQ, lddq, dq_head_stride, d_mult) && writes_wide(dK, lddk, dk_head_stride, d_mult) &&
                      writes_wide(dV, lddv, dv_head_stride, d_mult);
    const int vec = wide ? Elem::kWide : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid(name, M > K ? M : K, H, g); st != MISPMM_OK) return st;
    if (!r.reads_aligned2() || (grads_bf16 && !aligned2s({dQ, dK, dV})))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: Q, K, V, grad_out and bf16 gradients must be 2-byte aligned", name);
    // an output must not overlap an input, the workspace or another output
    Extent ins[Reads<Elem>::kExtents];
    r.extents(ins);
    const Extent outs[] = {extent(dQ, H, dq_head_stride, dQ ? span(M, lddq, D) : 0, d_elem), extent(dK, H, dk_head_stride, dK ? span(K, lddk, D) : 0, d_elem),
                           extent(dV, H, dv_head_stride, dV ? span(K, lddv, Dv) : 0, d_elem),
                           extent(row_pass ? delta : nullptr, 1, 0, static_cast<uint64_t>(H) * M, 4)};
    for (size_t i = 0; i < 4; ++i) {
        for (const Extent &in : ins)
            if (meet(outs[i], in)) return fail(MISPMM_ERR_INVALID_ARG, "%s: dQ, dK, dV or delta overlaps an input", name);
        for (size_t j = i + 1; j < 4; ++j)
            if (meet(outs[i], outs[j])) return fail(MISPMM_ERR_INVALID_ARG, "%s: dQ, dK, dV and delta overlap one another", name);
    }
    BwdCall<Elem> c{};
    c.stream = as_stream(stream);
    c.H = H;
    BwdParams<Elem> &p = c.p;
    BwdPtrs<Elem> &a = c.a;
    r.fill(p, a);
    a.delta = delta;
    if constexpr (Elem::kWidens) p.narrow = grads_bf16 ? 1u : 0u;
    if (row_pass) {
        p.N = M;
        a.ptrs = rowPtrs, a.idxs = colIdxs, a.perm = nullptr;
        a.d0 = dQ, a.d1 = nullptr;
        p.ldd0 = lddq, p.d0_head = dq_head_stride;
        dispatch_pass<Elem, true>(c, vec, g, width, row_tag);
        MISPMM_LAUNCH_CHECK();
    }
    if (col_pass) {
        p.N = K;
        a.ptrs = tRowPtrs, a.idxs = tColIdxs, a.perm = bias ? perm : nullptr;
        a.d0 = dK, a.d1 = dV;
        p.ldd0 = lddk, p.d0_head = dk_head_stride, p.ldd1 = lddv, p.d1_head = dv_head_stride;
        dispatch_pass<Elem, false>(c, vec, g, width, col_tag);
        MISPMM_LAUNCH_CHECK();
    }
    return MISPMM_OK;
}

template <class Elem>
int dbias_entry(const char *name, const char *tag, mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz,
                const uint32_t *rowPtrs, const uint32_t *colIdxs, const typename Elem::in_t *Q, uint64_t q_head_stride, uint32_t ldq,
                const typename Elem::in_t *Kmat, uint64_t k_head_stride, uint32_t ldk, uint32_t D, const typename Elem::in_t *V,
                uint64_t v_head_stride, uint32_t ldv, uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride,
                const float *out, uint64_t out_head_stride, uint32_t ldo, const float *lse, const typename Elem::in_t *grad_out,
                uint64_t g_head_stride, uint32_t ldg, float *dBias, uint64_t dbias_head_stride) {
    if (const int st = refuse_shape(name, D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0 || nnz == 0) return MISPMM_OK;
    if (!rowPtrs || !colIdxs || !Q || !Kmat || !V) return fail(MISPMM_ERR_INVALID_ARG, "%s: rowPtrs, colIdxs, Q, K or V is null", name);
    if (!out || !lse || !grad_out || !dBias) return fail(MISPMM_ERR_INVALID_ARG, "%s: out, lse, grad_out or dBias is null", name);
    Reads<Elem> r{H, M, K, nnz, D, Dv, Q, q_head_stride, ldq, Kmat, k_head_stride, ldk, V, v_head_stride, ldv, scale, bias, bias_head_stride,
                  out, out_head_stride, ldo, lse, grad_out, g_head_stride, ldg, 0, 0, 0, 0, 0, 0};
    if (r.short_ld())
        return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u ldg=%u)", name,
                    D, ldq, ldk, Dv, ldv, ldo, ldg);
    if (H > 1 && dbias_head_stride < nnz)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: dbias_head_stride %llu is smaller than nnz %u: dBias is per head", name,
                    static_cast<ull>(dbias_head_stride), nnz);
    if (const int st = r.measure(name); st != MISPMM_OK) return st;
    // dBias is stored a word at a time and has no say in the lane width
    const int vec = r.wide() ? Elem::kWide : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid(name, M, H, g); st != MISPMM_OK) return st;
    if (!r.reads_aligned2()) return fail(MISPMM_ERR_INVALID_ARG, "%s: Q, K, V and grad_out must be 2-byte aligned", name);
    // the output must not overlap an input, the pattern included
    Extent ins[Reads<Elem>::kExtents + 2];
    r.extents(ins);
    ins[Reads<Elem>::kExtents] = extent(rowPtrs, 1, 0, static_cast<uint64_t>(M) + 1, 4);
    ins[Reads<Elem>::kExtents + 1] = extent(colIdxs, 1, 0, nnz, 4);
    const Extent o = extent(dBias, H, dbias_head_stride, nnz, 4);
    for (const Extent &in : ins)
        if (meet(o, in)) return fail(MISPMM_ERR_INVALID_ARG, "%s: dBias overlaps an input", name);
    DbiasCall<Elem> c{};
    c.stream = as_stream(stream);
    c.H = H;
    r.fill(c.p, c.a);
    c.p.dbias_head = dbias_head_stride;
    c.a.ptrs = rowPtrs, c.a.idxs = colIdxs, c.a.dbias = dBias;
    dispatch_dbias<Elem>(c, vec, g, width, tag);
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}

}  // namespace

}  // namespace mispmm
