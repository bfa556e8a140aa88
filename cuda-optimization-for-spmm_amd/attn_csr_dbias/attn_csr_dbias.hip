// libmispmm_attn_csr_dbias.so: the bias gradient of fused attention on a CSR pattern, for fp32 operands and for bf16 ones
// (include/mispmm_attn_csr_dbias.h) -- dBias for all heads in one launch.  The kernel is attn_csr/attn_csr_dbias.hpp's over
// ElemF32 (V4: 16-byte lanes, or V1) and ElemBf16 (V8 or V1) and the entry point is attn_csr/attn_csr_entry.hpp's dbias_entry,
// written once for both (its refusals, the choice of the lane width by the backward's rule on the operands this kernel reads,
// the overlap check and the parameter block); what stands here is the two exports, their names and their tags.
#include "../attn_csr/attn_csr_entry.hpp"
#include "mispmm_attn_csr_dbias.h"

using namespace mispmm;

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
