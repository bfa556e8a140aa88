// libmispmm_attn_csr_bf16_bwd.so: the backward of fused attention on a CSR pattern with Q, K, V and grad_out in bf16
// (include/mispmm_attn_csr_bf16_bwd.h) -- dQ, dK and dV for all heads in at most two launches, fp32 arithmetic on the exactly
// widened operands, no fp32 copy of any operand; out and lse are the fp32 ones the bf16 forward wrote; the gradients in fp32 or
// bf16.  The two kernels are attn_csr/attn_csr_bwd.hpp's over ElemBf16 (V8: 16-byte lanes, or V1) and the entry point is
// attn_csr/attn_csr_entry.hpp's bwd_entry over the same policy (its refusals, the choice of the lane width, the overlap check
// and the two parameter blocks); what stands here is the export, its name and its two tags.
#include "../../attn_csr/attn_csr_entry.hpp"
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
    return bwd_entry<ElemBf16>("attn_csr_bf16_bwd", "attn_csr_bf16_bwd_row<G%d,V%d,C%d>", "attn_csr_bf16_bwd_col<G%d,V%d,C%d>", stream, H, M, K, nnz,
                               rowPtrs, colIdxs, tRowPtrs, tColIdxs, perm, Q, q_head_stride, ldq, Kmat, k_head_stride, ldk, D, V, v_head_stride, ldv,
                               Dv, scale, bias, bias_head_stride, out, out_head_stride, ldo, lse, grad_out, g_head_stride, ldg, delta, grads_bf16,
                               dQ, dq_head_stride, lddq, dK, dk_head_stride, lddk, dV, dv_head_stride, lddv);
}
