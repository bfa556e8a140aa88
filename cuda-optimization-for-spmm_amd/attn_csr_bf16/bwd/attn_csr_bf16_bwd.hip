// libmispmm_attn_csr_bf16_bwd.so: the backward of fused attention on a CSR pattern with Q, K, V and grad_out in bf16
// (include/mispmm_attn_csr_bf16_bwd.h) -- dQ, dK and dV for all heads in at most two launches, fp32 arithmetic on the exactly
// widened operands, no fp32 copy of any operand; out and lse are the fp32 ones the bf16 forward wrote; the gradients in fp32 or
// bf16.  The two kernels are attn_csr/attn_csr_bwd.hpp's over ElemBf16 (V8: 16-byte lanes, or V1); what stands here is the
// entry point: its refusals, the choice of the lane width, the overlap check and the two parameter blocks.
#include "../../attn_csr/attn_csr_bwd.hpp"
#include "mispmm_attn_csr_bf16_bwd.h"

using namespace mispmm;

extern "C" int mispmm_attn_csr_bf16_bwd(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                        const uint32_t *colIdxs, const uint32_t *tRowPtrs, const uint32_t *tColIdxs, const uint32_t *perm,
                                        const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat, uint64_t k_head_stride,
                                        uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv, uint32_t Dv,
                                        float scale, const float *bias, uint64_t bias_head_stride, const float *out,
                                        uint64_t out_head_stride, uint32_t ldo, const float *lse, const uint16_t *grad_out,
                                        uint64_t g_head_stride, uint32_t ldg, float *delta, int grads_bf16, void *dQ,
                                        uint64_t dq_head_stride, uint32_t lddq, void *dK, uint64_t dk_head_stride, uint32_t lddk, void *dV,
                                        uint64_t dv_head_stride, uint32_t lddv) {
    if (const int st = refuse_shape("attn_csr_bf16_bwd", D, Dv, scale); st != MISPMM_OK) return st;
    if (H == 0 || M == 0 || (!dQ && !dK && !dV)) return MISPMM_OK;
    const bool col_pass = (dK || dV) && K != 0;
    const bool row_pass = dQ || (dK && K != 0);  // dK reads delta
    if (!rowPtrs || !Q || !Kmat || !V || (nnz != 0 && !colIdxs))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: rowPtrs, colIdxs, Q, K or V is null");
    if (!out || !lse || !grad_out || (row_pass && !delta))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: out, lse, grad_out or delta is null");
    if (col_pass && (!tRowPtrs || (nnz != 0 && !tColIdxs)))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: dK and dV need the pattern of A^T: tRowPtrs or tColIdxs is null");
    if (col_pass && bias && nnz != 0 && !perm)
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: with a bias, dK and dV need perm, which is null");
    if (ldq < D || ldk < D || ldv < Dv || ldo < Dv || ldg < Dv || (dQ && lddq < D) || (dK && lddk < D) || (dV && lddv < Dv))
        return fail(MISPMM_ERR_INVALID_ARG,
                    "attn_csr_bf16_bwd: leading dimension smaller than the width (D=%u ldq=%u ldk=%u lddq=%u lddk=%u, Dv=%u ldv=%u ldo=%u ldg=%u lddv=%u)",
                    D, ldq, ldk, lddq, lddk, Dv, ldv, ldo, ldg, lddv);
    // a raw buffer descriptor spans less than 2 GiB and bit 31 of an offset marks a dropped load: bytes of the element type
    const uint64_t qs = span(M, ldq, D), ks = span(K, ldk, D), vs = span(K, ldv, Dv), os = span(M, ldo, Dv), gs = span(M, ldg, Dv);
    const uint64_t bs = bias ? static_cast<uint64_t>(nnz) : 0u;
    const uint64_t lim = 0x7FFFFFFFull;
    if (qs * 2u > lim || ks * 2u > lim || vs * 2u > lim || os * 4u > lim || gs * 2u > lim || bs * 4u > lim)
        return fail(MISPMM_ERR_UNSUPPORTED,
                    "attn_csr_bf16_bwd: Q, K, V, out, grad_out or bias of one head spans 2 GiB or more (%llu, %llu, %llu, %llu, %llu, %llu bytes)",
                    static_cast<unsigned long long>(qs * 2u), static_cast<unsigned long long>(ks * 2u), static_cast<unsigned long long>(vs * 2u),
                    static_cast<unsigned long long>(os * 4u), static_cast<unsigned long long>(gs * 2u), static_cast<unsigned long long>(bs * 4u));
    const uint64_t d_elem = grads_bf16 ? 2u : 4u, d_mult = grads_bf16 ? 8u : 4u;
    auto mult = [](uint64_t x, uint64_t m) { return x % m == 0; };
    bool wide = D % 8 == 0 && Dv % 8 == 0 && mult(ldq, 8) && mult(ldk, 8) && mult(ldv, 8) && mult(ldg, 8) && mult(ldo, 4) &&
                mult(q_head_stride, 8) && mult(k_head_stride, 8) && mult(v_head_stride, 8) && mult(g_head_stride, 8) &&
                mult(out_head_stride, 4) && aligned16(Q) && aligned16(Kmat) && aligned16(V) && aligned16(out) && aligned16(grad_out);
    wide = wide && (!dQ || (mult(lddq, d_mult) && mult(dq_head_stride, d_mult) && aligned16(dQ))) &&
           (!dK || (mult(lddk, d_mult) && mult(dk_head_stride, d_mult) && aligned16(dK))) &&
           (!dV || (mult(lddv, d_mult) && mult(dv_head_stride, d_mult) && aligned16(dV)));
    const int vec = wide ? 8 : 1;
    const uint32_t width = D > Dv ? D : Dv;
    const int g = pick_group(width, vec);
    if (const int st = refuse_grid("attn_csr_bf16_bwd", M > K ? M : K, H, g); st != MISPMM_OK) return st;
    if (!aligned2(Q) || !aligned2(Kmat) || !aligned2(V) || !aligned2(grad_out) ||
        (grads_bf16 && (!aligned2(dQ) || !aligned2(dK) || !aligned2(dV))))
        return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: Q, K, V, grad_out and bf16 gradients must be 2-byte aligned");
    // an output must not overlap an input, the workspace or another output: extents in bytes of each operand's own type
    const Extent ins[] = {extent(Q, H, q_head_stride, qs, 2),           extent(Kmat, H, k_head_stride, ks, 2),
                          extent(V, H, v_head_stride, vs, 2),           extent(out, H, out_head_stride, os, 4),
                          extent(grad_out, H, g_head_stride, gs, 2),    extent(bias, H, bias_head_stride, bs, 4),
                          extent(lse, 1, 0, static_cast<uint64_t>(H) * M, 4)};
    const Extent outs[] = {extent(dQ, H, dq_head_stride, dQ ? span(M, lddq, D) : 0, d_elem), extent(dK, H, dk_head_stride, dK ? span(K, lddk, D) : 0, d_elem),
                           extent(dV, H, dv_head_stride, dV ? span(K, lddv, Dv) : 0, d_elem),
                           extent(row_pass ? delta : nullptr, 1, 0, static_cast<uint64_t>(H) * M, 4)};
    for (size_t i = 0; i < 4; ++i) {
        for (const Extent &in : ins)
            if (meet(outs[i], in)) return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: dQ, dK, dV or delta overlaps an input");
        for (size_t j = i + 1; j < 4; ++j)
            if (meet(outs[i], outs[j])) return fail(MISPMM_ERR_INVALID_ARG, "attn_csr_bf16_bwd: dQ, dK, dV and delta overlap one another");
    }
    BwdCall<ElemBf16> c{};
    c.stream = as_stream(stream);
    c.H = H;
    BwdParams<ElemBf16> &p = c.p;
    p.M = M, p.D = D, p.Dv = Dv;
    p.ldq = ldq * 2u, p.ldk = ldk * 2u, p.ldv = ldv * 2u, p.ldg = ldg * 2u, p.ldo = ldo * 4u;
    p.q_bytes = static_cast<uint32_t>(qs * 2u), p.k_bytes = static_cast<uint32_t>(ks * 2u), p.v_bytes = static_cast<uint32_t>(vs * 2u);
    p.g_bytes = static_cast<uint32_t>(gs * 2u), p.o_bytes = static_cast<uint32_t>(os * 4u), p.bias_bytes = static_cast<uint32_t>(bs * 4u);
    p.narrow = grads_bf16 ? 1u : 0u;
    p.scale = scale;
    p.q_head = q_head_stride, p.k_head = k_head_stride, p.v_head = v_head_stride, p.g_head = g_head_stride, p.o_head = out_head_stride;
    p.bias_head = bias_head_stride;
    BwdPtrs<ElemBf16> &a = c.a;
    a.Q = Q, a.K = Kmat, a.V = V, a.dO = grad_out, a.out = out, a.lse = lse, a.bias = bias, a.delta = delta;
    if (row_pass) {
        p.N = M;
        a.ptrs = rowPtrs, a.idxs = colIdxs, a.perm = nullptr;
        a.d0 = dQ, a.d1 = nullptr;
        p.ldd0 = lddq, p.d0_head = dq_head_stride;
        dispatch_pass<ElemBf16, true>(c, vec, g, width, "attn_csr_bf16_bwd_row<G%d,V%d,C%d>");
        MISPMM_LAUNCH_CHECK();
    }
    if (col_pass) {
        p.N = K;
        a.ptrs = tRowPtrs, a.idxs = tColIdxs, a.perm = bias ? perm : nullptr;
        a.d0 = dK, a.d1 = dV;
        p.ldd0 = lddk, p.d0_head = dk_head_stride, p.ldd1 = lddv, p.d1_head = dv_head_stride;
        dispatch_pass<ElemBf16, false>(c, vec, g, width, "attn_csr_bf16_bwd_col<G%d,V%d,C%d>");
        MISPMM_LAUNCH_CHECK();
    }
    return MISPMM_OK;
}
