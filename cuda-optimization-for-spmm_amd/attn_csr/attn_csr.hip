// libmispmm_attn_csr.so: fused attention on a CSR pattern in fp32 (include/mispmm_attn_csr.h) -- scores, row softmax and the
// product with V in ONE launch for all heads.  Neither the scores nor the weights are written; per row only out and, where
// asked for, a log-sum-exp.  The kernel is attn_csr_fwd.hpp's over ElemF32 (V4: 16-byte lanes, or V1) and the entry point is
// attn_csr_entry.hpp's fwd_entry over the same policy (its refusals, the choice of the lane width and the parameter block);
// what stands here is the export, its name and its tag.
// The sources lie outside csrc/, fused/ and rows_bf16/: the census tests hold those directories and their libraries to their
// records.
#include "attn_csr_entry.hpp"
#include "mispmm_attn_csr.h"

using namespace mispmm;

extern "C" int mispmm_attn_csr_f32(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                   const uint32_t *colIdxs, const float *Q, uint64_t q_head_stride, uint32_t ldq, const float *Kmat,
                                   uint64_t k_head_stride, uint32_t ldk, uint32_t D, const float *V, uint64_t v_head_stride, uint32_t ldv,
                                   uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, float *out,
                                   uint64_t out_head_stride, uint32_t ldo, float *lse) {
    return fwd_entry<ElemF32>("attn_csr_f32", "attn_csr<f32,G%d,V%d,C%d>", stream, H, M, K, nnz, rowPtrs, colIdxs, Q, q_head_stride, ldq, Kmat,
                              k_head_stride, ldk, D, V, v_head_stride, ldv, Dv, scale, bias, bias_head_stride, out, out_head_stride, ldo, 0, lse);
}
