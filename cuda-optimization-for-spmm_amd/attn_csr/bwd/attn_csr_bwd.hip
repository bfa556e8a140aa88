// libmispmm_attn_csr_bwd.so: the backward of fused attention on a CSR pattern in fp32 (include/mispmm_attn_csr_bwd.h) -- dQ, dK
// and dV for all heads in at most two launches.  The two kernels are attn_csr_bwd.hpp's over ElemF32 (V4: 16-byte lanes, or
// V1); what stands here is the entry point: its refusals, the choice of the lane width, the overlap check and the two parameter
// blocks.
#include "../attn_csr_bwd.hpp"
#include "mispmm_attn_csr_bwd.h"

using namespace mispmm;

extern "C" int mispmm_attn_csr_bwd_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                       const uint32_t *colIdxs, const uint32_t *tRowPtrs, const uint32_t *tColIdxs, const uint32_t *perm,
                                       const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat, uint64_t k_head_stride,
                                       uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv, uint32_t Dv,
                                       float scale, const float *bias, uint64_t bias_head_stride, const float *out,
                                       uint64_t out_head_stride, uint32_t ldo, const float *lse, const float *grad_out,
                                       uint64_t g_head_stride, uint32_t ldg, float *delta, float *dQ, uint64_t dq_head_stride,
                                       uint32_t lddq, float *dK, uint64_t dk_head_stride, uint32_t lddk, float *dV,
                                       uint64_t dv_head_stride, uint32_t lddv) {
    if (const int st = refuse_shape("attn_csr_bwd_f32", D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0 || (!dQ && !dK && !dV)) return MISPMM_OK;
    const bool col_pass = (dK || dV) && K != 0;
    const bool row_pass = dQ || (dK && K != 0);  // dK reads delta
    if (!rowPtrs || !Q || !Kmat || !V || (nnz != 0 && !colIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: rowPtrs, colIdxs, Q, K or V is null");
    if (!out || !lse || !grad_out || (row_pass && !delta))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: out, lse, grad_out or delta is null");
    if (col_pass && (!tRowPtrs || (nnz != 0 && !tColIdxs)))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: dK and dV need the pattern of A^T: tRowPtrs or tColIdxs is null");
    if (col_pass && bias && nnz != 0 && !perm)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: with a bias, dK and dV need perm, which is null");
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv || ldg < Dv || (dQ && lddq < D) || (dK && lddk < D) || (dV && lddv < Dv))
        return fail(MISPMM_ERR_INVALID_ARG,
                    "attn_csr_bwd_f32: leading dimension smaller than the width (D=%u ldq=%u ldk=%u lddq=%u lddk=%u, Dv=%u ldv=%u ldo=%u ldg=%u lddv=%u)",
                    D, ldq, ldk, lddq, lddk, Dv, ldv, ldo, ldg, lddv);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load
    const uint64_t qs = span(M, ldq, D), ks = span(K, ldk, D), vs = span(K, ldv, Dv), os = span(M, ldo, Dv), gs = span(M, ldg, Dv);
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) : 0u;
    const uint64_t lim = 0x7FFFFFFFull / 4u;
    if (qs > lim || ks > lim || vs > lim || os > lim || gs > lim || bs > lim)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "attn_csr_bwd_f32: Q, K, V, out, grad_out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu, %llu bytes)",
                    static_cast<unsigned long long>(qs * 4u), static_cast<unsigned long long>(ks * 4u), static_cast<unsigned long long>(vs * 4u),
                    static_cast<unsigned long long>(os * 4u), static_cast<unsigned long long>(gs * 4u), static_cast<unsigned long long>(bs * 4u));
    auto mult4 = [](uint64_t x) { return x % 4 == 0; };
    bool wide = D % 4 == 0 && Dv % 4 == 0 && mult4(ldq) && mult4(ldk) && mult4(ldv) && mult4(ldo) && mult4(ldg) && mult4(q_head_stride) &&
                mult4(k_head_stride) && mult4(v_head_stride) && mult4(out_head_stride) && mult4(g_head_stride) && aligned16(Q) &&
                aligned16(Kmat) && aligned16(V) && aligned16(out) && aligned16(grad_out);
    wide = wide && (!dQ || (mult4(lddq) && mult4(dq_head_stride) && aligned16(dQ))) && (!dK || (mult4(lddk) && mult4(dk_head_stride) && aligned16(dK))) &&
           (!dV || (mult4(lddv) && mult4(dv_head_stride) && aligned16(dV)));
    const int vec = wide ? 4 : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid("attn_csr_bwd_f32", M > K ? M : K, H, g); st != MISPMM_OK) return st;
    // an output must not overlap an input, the workspace or another output: extents in bytes
    const Extent ins[] = {extent(Q, H, q_head_stride, qs, 4),           extent(Kmat, H, k_head_stride, ks, 4), extent(V, H, v_head_stride, vs, 4),
                          extent(out, H, out_head_stride, os, 4),       extent(grad_out, H, g_head_stride, gs, 4), extent(bias, H, bias_head_stride, bs, 4),
                          extent(lse, 1, 0, static_cast<uint64_t>(H) * M, 4)};
    const Extent outs[] = {extent(dQ, H, dq_head_stride, dQ ? span(M, lddq, D) : 0, 4), extent(dK, H, dk_head_stride, dK ? span(K, lddk, D) : 0, 4),
                           extent(dV, H, dv_head_stride, dV ? span(K, lddv, Dv) : 0, 4), extent(row_pass ? delta : nullptr, 1, 0, static_cast<uint64_t>(H) * M, 4)};
    for (size_t i = 0; i < 4; ++i) {
        for (const Extent &in : ins)
            if (meet(outs[i], in)) return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: dQ, dK, dV or delta overlaps an input");
        for (size_t j = i + 1; j < 4; ++j)
            if (meet(outs[i], outs[j])) return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bwd_f32: dQ, dK, dV and delta overlap one another");
    }
    BwdCall<ElemF32> c{};
    c.stream = as_stream(stream);
    c.H = H;
    BwdParams<ElemF32> &p = c.p;
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq = ldq * 4u, p.ldk = ldk * 4u, p.ldv = ldv * 4u, p.ldg = ldg * 4u, p.ldo = ldo * 4u;
    p.q_bytes = static_cast<uint32_t>(qs * 4u), p.k_bytes = static_cast<uint32_t>(ks * 4u), p.v_bytes = static_cast<uint32_t>(vs * 4u);
    p.g_bytes = static_cast<uint32_t>(gs * 4u), p.o_bytes = static_cast<uint32_t>(os * 4u), p.bias_bytes = static_cast<uint32_t>(bs * 4u);
    p.scale = scale;
    p.q_head = q_head_stride, p.k_head = k_head_stride, p.v_head = v_head_stride, p.g_head = g_head_stride, p.o_head = out_head_stride;
    p.bias_head = bias_head_stride;
    BwdPtrs<ElemF32> &a = c.a;
    a.Q = Q, a.K = Kmat, a.V = V, a.dO = grad_out, a.out = out, a.lse = lse, a.bias = bias, a.delta = delta;
    if (row_pass) {
        p.N = M;
        a.ptrs = rowPtrs, a.idxs = colIdxs, a.perm = nullptr;
        a.d0 = dQ, a.d1 = nullptr;
        p.ldd0 = lddq, p.d0_head = dq_head_stride;
        dispatch_pass<ElemF32, true>(c, vec, g, width, "attn_csr_bwd_row<f32,G%d,V%d,C%d>");
        MISPMM_LAUNCH_CHECK();
    }
    if (col_pass) {
        p.N = K;
        a.ptrs = tRowPtrs, a.idxs = tColIdxs, a.perm = bias ? perm : nullptr;
        a.d0 = dK, a.d1 = dV;
        p.ldd0 = lddk, p.d0_head = dk_head_stride, p.ldd1 = lddv, p.d1_head = dv_head_stride;
        dispatch_pass<ElemF32, false>(c, vec, g, width, "attn_csr_bwd_col<f32,G%d,V%d,C%d>");
        MISPMM_LAUNCH_CHECK();
    }
    return MISPMM_OK;
}
