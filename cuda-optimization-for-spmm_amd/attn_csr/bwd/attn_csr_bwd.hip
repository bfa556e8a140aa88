// libmispmm_attn_csr_bwd.so: the backward of fused attention on a CSR pattern in fp32 (include/mispmm_attn_csr_bwd.h) -- dQ, dK
// and dV for all heads in at most two launches.  The two kernels are attn_csr_bwd.hpp's over ElemF32 (V4: 16-byte lanes, or
// V1) and the entry point is attn_csr_entry.hpp's bwd_entry over the same policy (its refusals, the choice of the lane width,
// the overlap check and the two parameter blocks); what stands here is the export, its name and its two tags.
#include "../attn_csr_entry.hpp"
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
    return bwd_entry<ElemF32>("attn_csr_bwd_f32", "attn_csr_bwd_row<f32,G%d,V%d,C%d>", "attn_csr_bwd_col<f32,G%d,V%d,C%d>", stream, H, M, K, nnz,
                              rowPtrs, colIdxs, tRowPtrs, tColIdxs, perm, Q, q_head_stride, ldq, Kmat, k_head_stride, ldk, D, V, v_head_stride, ldv,
                              Dv, scale, bias, bias_head_stride, out, out_head_stride, ldo, lse, grad_out, g_head_stride, ldg, delta, 0, dQ,
                              dq_head_stride, lddq, dK, dk_head_stride, lddk, dV, dv_head_stride, lddv);
}
