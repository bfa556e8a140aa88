// libmispmm_attn_csr_dbias.so: the bias gradient of fused attention on a CSR pattern, for fp32 operands and for bf16 ones
// (include/mispmm_attn_csr_dbias.h) -- dBias for all heads in one launch.  The kernel is attn_csr/attn_csr_dbias.hpp's over
// ElemF32 (V4: 16-byte lanes, or V1) and ElemBf16 (V8 or V1); what stands here is the entry point, written once for both: its
// refusals, the choice of the lane width (the backward's rule on the operands this kernel reads), the overlap check and the
// parameter block.
#include "../attn_csr/attn_csr_dbias.hpp"
#include "mispmm_attn_csr_dbias.h"

using namespace mispmm;

namespace {

template <class Elem>
int dbias_entry(const char *name, const char *tag, mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz,
                const uint32_t *rowPtrs, const uint32_t *colIdxs, const typename Elem::in_t *Q, uint64_t q_head_stride, uint32_t ldq,
                const typename Elem::in_t *Kmat, uint64_t k_head_stride, uint32_t ldk, uint32_t D, const typename Elem::in_t *V,
                uint64_t v_head_stride, uint32_t ldv, uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride,
                const float *out, uint64_t out_head_stride, uint32_t ldo, const float *lse, const typename Elem::in_t *grad_out,
                uint64_t g_head_stride, uint32_t ldg, float *dBias, uint64_t dbias_head_stride) {
    constexpr uint64_t EB = Elem::kBytes, WIDE = Elem::kWide;
    if (const int st = refuse_shape(name, D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0 || nnz == 0) return MISPMM_OK;
    if (!rowPtrs || !colIdxs || !Q || !Kmat || !V) return fail(MISPMM_ERR_INVALID_ARG, "%s: rowPtrs, colIdxs, Q, K or V is null", name);
    if (!out || !lse || !grad_out || !dBias) return fail(MISPMM_ERR_INVALID_ARG, "%s: out, lse, grad_out or dBias is null", name);
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv || ldg < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u ldg=%u)", name,
                    D, ldq, ldk, Dv, ldv, ldo, ldg);
    if (H > 1 && dbias_head_stride < nnz)
        return fail(MISPMM_ERR_INVALID_ARG, "%s: dbias_head_stride %llu is smaller than nnz %u: dBias is per head", name,
                    static_cast<unsigned long long>(dbias_head_stride), nnz);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load: bytes of each operand's type
    const uint64_t qs = span(M, ldq, D), ks = span(K, ldk, D), vs = span(K, ldv, Dv), os = span(M, ldo, Dv), gs = span(M, ldg, Dv);
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) : 0u;
    const uint64_t lim = 0x7FFFFFFFull;
    if (qs * EB > lim || ks * EB > lim || vs * EB > lim || os * 4u > lim || gs * EB > lim || bs * 4u > lim)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "%s: Q, K, V, out, grad_out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu, %llu bytes)", name,
                    static_cast<unsigned long long>(qs * EB), static_cast<unsigned long long>(ks * EB), static_cast<unsigned long long>(vs * EB),
                    static_cast<unsigned long long>(os * 4u), static_cast<unsigned long long>(gs * EB), static_cast<unsigned long long>(bs * 4u));
    // the backward's rule on what this kernel reads; dBias is stored a word at a time and has no say
    auto mult = [](uint64_t x, uint64_t m) { return x % m == 0; };
    const bool wide = D % WIDE == 0 && Dv % WIDE == 0 && mult(ldq, WIDE) && mult(ldk, WIDE) && mult(ldv, WIDE) && mult(ldg, WIDE) && mult(ldo, 4) &&
                      mult(q_head_stride, WIDE) && mult(k_head_stride, WIDE) && mult(v_head_stride, WIDE) && mult(g_head_stride, WIDE) &&
                      mult(out_head_stride, 4) && aligned16(Q) && aligned16(Kmat) && aligned16(V) && aligned16(out) && aligned16(grad_out);
    const int vec = wide ? Elem::kWide : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid(name, M, H, g); st != MISPMM_OK) return st;
    if (EB == 2 && (!aligned2(Q) ||!aligned2(Kmat) || !aligned2(V) || !aligned2(grad_out)))
        return fail(MISPMM_ERR_INVALID_ARG, "%s: Q, K, V and grad_out must be 2-byte aligned", name);
    // the output must not overlap an input: extents in bytes of each operand's own type
    const Extent ins[] = {extent(Q, H, q_head_stride, qs, EB),        extent(Kmat, H, k_head_stride, ks, EB),
                          extent(V, H, v_head_stride, vs, EB),        extent(out, H, out_head_stride, os, 4),
                          extent(grad_out, H, g_head_stride, gs, EB), extent(bias, H, bias_head_stride, bs, 4),
                          extent(lse, 1, 0, static_cast<uint64_t>(H) * M, 4), extent(rowPtrs, 1, 0, static_cast<uint64_t>(M) + 1, 4),
                          extent(colIdxs, 1, 0, nnz, 4)};
    const Extent o = extent(dBias, H, dbias_head_stride, nnz, 4);
    for (const Extent &in : ins)
        if (meet(o, in)) return fail(MISPMM_ERR_INVALID_ARG, "%s: dBias overlaps an input", name);
    DbiasCall<Elem> c{};
    c.stream = as_stream(stream);
    c.H = H;
    DbiasParams &p = c.p;
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq = static_cast<uint32_t>(ldq * EB), p.ldk = static_cast<uint32_t>(ldk * EB), p.ldv = static_cast<uint32_t>(ldv * EB);
    p.ldg = static_cast<uint32_t>(ldg * EB), p.ldo = ldo * 4u;
    p.q_bytes = static_cast<uint32_t>(qs * EB), p.k_bytes = static_cast<uint32_t>(ks * EB), p.v_bytes = static_cast<uint32_t>(vs * EB);
    p.g_bytes = static_cast<uint32_t>(gs * EB), p.o_bytes = static_cast<uint32_t>(os * 4u), p.bias_bytes = static_cast<uint32_t>(bs * 4u);
    p.scale = scale;
    p.q_head = q_head_stride, p.k_head = k_head_stride, p.v_head = v_head_stride, p.g_head = g_head_stride, p.o_head = out_head_stride;
    p.bias_head = bias_head_stride, p.dbias_head = dbias_head_stride;
    DbiasPtrs<Elem> &a = c.a;
    a.ptrs = rowPtrs, a.idxs = colIdxs, a.Q = Q, a.K = Kmat, a.V = V, a.dO = grad_out, a.out = out, a.lse = lse, a.bias = bias, a.dbias = dBias;
    dispatch_dbias<Elem>(c, vec, g, width, tag);
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}

}  // namespace

extern "C" int mispmm_attn_csr_dbias_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                         const uint32_t *colIdxs, const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat,
                                         uint64_t k_head_stride, uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv,
                                         uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, const float *out,
                                         uint64_t out_head_stride, uint32_t ldo, const float *lse, const float *grad_out, uint64_t g_head_stride,
                                         uint32_t ldg, float *dBias, uint64_t dbias_head_stride) {
    return dbias_entry<ElemF32>("attn_csr_dbias_f32", "attn_csr_dbias<f32,G%d,V%d,C%d>", stream, H, M, K, nnz, rowPtrs, colIdxs, Q, q_head_stride, ldq,
                                Kmat, k_head_stride, ldk, D, V, v_head_stride, ldv, Dv, scale, bias, bias_head_stride, out, out_head_stride, ldo, lse,
                                grad_out, g_head_stride, ldg, dBias, dbias_head_stride);
}

extern "C" int mispmm_attn_csr_dbias_bf16(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                          const uint32_t *colIdxs, const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat,
                                          uint64_t k_head_stride, uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv,
                                          uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, const float *out,
                                          uint64_t out_head_stride, uint32_t ldo, const float *lse, const uint16_t *grad_out,
                                          uint64_t g_head_stride, uint32_t ldg, float *dBias, uint64_t dbias_head_stride) {
    return dbias_entry<ElemBf16>("attn_csr_dbias_bf16", "attn_csr_dbias<bf16,G%d,V%d,C%d>", stream, H, M, K, nnz, rowPtrs, colIdxs, Q, q_head_stride,
                                 ldq, Kmat, k_head_stride, ldk, D, V, v_head_stride, ldv, Dv, scale, bias, bias_head_stride, out, out_head_stride, ldo,
                                 lse, grad_out, g_head_stride, ldg, dBias, dbias_head_stride);
}
