// libmispmm_attn_csr.so: fused attention on a CSR pattern in fp32 (include/mispmm_attn_csr.h) -- scores, row softmax and the
// product with V in ONE launch for all heads.  Neither the scores nor the weights are written; per row only out and, where
// asked for, a log-sum-exp.  The kernel is attn_csr_fwd.hpp's over ElemF32 (V4: 16-byte lanes, or V1); what stands here is
// the entry point: its refusals, the choice of the lane width and the parameter block.
// The sources lie outside csrc/, fused/ and rows_bf16/: the census tests hold those directories and their libraries to their
// records.
#include "attn_csr_fwd.hpp"
#include "mispmm_attn_csr.h"

using namespace mispmm;

extern "C" int mispmm_attn_csr_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                   const uint32_t *colIdxs, const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat,
                                   uint64_t k_head_stride, uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv,
                                   uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, float *out,
                                   uint64_t out_head_stride, uint32_t ldo, float *lse) {
    if (const int st = refuse_shape("attn_csr_f32", D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0) return MISPMM_OK;
    if (!rowPtrs || !Q || !Kmat || !V || !out || (nnz != 0 && !colIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_f32: rowPtrs, colIdxs, Q, K, V or out is null");
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_f32: leading dimension smaller than the width (D=%u ldq=%u ldk=%u, Dv=%u ldv=%u ldo=%u)", D,
                    ldq, ldk, Dv, ldv, ldo);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    const uint64_t qs = span(M, ldq, D) * 4u, ks = span(K, ldk, D) * 4u, vs = span(K, ldv, Dv) * 4u, os = span(M, ldo, Dv) * 4u;
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) * 4u : 0u;
    if (qs > 0x7FFFFFFFull || ks > 0x7FFFFFFFull || vs > 0x7FFFFFFFull || os > 0x7FFFFFFFull || bs > 0x7FFFFFFFull)
        return fail(MISPMM_ERR_UNSUPPORTED, "attn_csr_f32: Q, K, V, out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu bytes)",
                    static_cast<unsigned long long>(qs), static_cast<unsigned long long>(ks), static_cast<unsigned long long>(vs),
                    static_cast<unsigned long long>(os), static_cast<unsigned long long>(bs));
    const bool wide = D % 4 == 0 && Dv % 4 == 0 && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 && q_head_stride % 4 == 0 &&
                      k_head_stride % 4 == 0 && v_head_stride % 4 == 0 && out_head_stride % 4 == 0 && aligned16(Q) && aligned16(Kmat) &&
                      aligned16(V) && aligned16(out);
    const int vec = wide ? 4 : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid("attn_csr_f32", M, H, g); st != MISPMM_OK) return st;
    FwdCall<ElemF32> c{};
    c.stream = as_stream(stream);
    c.H = H;
    c.rowPtrs = rowPtrs, c.colIdxs = colIdxs;
    c.Q = Q, c.K = Kmat, c.V = V, c.bias = bias, c.out = out, c.lse = lse;
    FwdParams<ElemF32> &p = c.p;
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq = ldq, p.ldk = ldk * 4u, p.ldv = ldv * 4u, p.ldo = ldo;
    p.q_bytes = static_cast<uint32_t>(qs), p.k_bytes = static_cast<uint32_t>(ks), p.v_bytes = static_cast<uint32_t>(vs);
    p.bias_bytes = static_cast<uint32_t>(bs);
    p.scale = scale;
    p.q_head = q_head_stride, p.k_head = k_head_stride, p.v_head = v_head_stride, p.o_head = out_head_stride, p.bias_head = bias_head_stride;
    ElemF32::with_instance(vec, g, width, [&](auto gr, auto v, auto ch) {
        launch_attn_csr<ElemF32, decltype(gr)::value, decltype(v)::value, decltype(ch)::value>(c, "attn_csr<f32,G%d,V%d,C%d>");
    });
    MISPMM_LAUNCH_CHECK();
    return MISPMM_OK;
}
