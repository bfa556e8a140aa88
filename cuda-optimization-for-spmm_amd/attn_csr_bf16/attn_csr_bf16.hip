// libmispmm_attn_csr_bf16.so: fused attention on a CSR pattern with Q, K and V in bf16 (include/mispmm_attn_csr_bf16.h) --
// scores, row softmax and the product with V in ONE launch for all heads, fp32 arithmetic on the exactly widened operands;
// out in fp32, or that fp32 result rounded once to bf16 (a wave-uniform branch of the store: no instances of its own).
// The kernel is attn_csr/attn_csr_fwd.hpp's over ElemBf16 (V8: 16-byte lanes, or V1) and the entry point is
// attn_csr/attn_csr_entry.hpp's fwd_entry over the same policy (its refusals, the choice of the lane width and the parameter
// block); what stands here is the export, its name and its tag.
// The sources lie outside csrc/, fused/, rows_bf16/ and attn_csr/: the census tests hold those directories and their
// libraries to their records.
#include "../attn_csr/attn_csr_entry.hpp"
#include "mispmm_attn_csr_bf16.h"

using namespace mispmm;

extern "C" int mispmm_attn_csr_bf16(mispmm_stream_t stream, uint32_t H, uint32_t M, uint32_t K, uint32_t nnz, const uint32_t *rowPtrs,
                                    const uint32_t *colIdxs, const uint16_t *Q, uint64_t q_head_stride, uint32_t ldq, const uint16_t *Kmat,
                                    uint64_t k_head_stride, uint32_t ldk, uint32_t D, const uint16_t *V, uint64_t v_head_stride, uint32_t ldv,
                                    uint32_t Dv, float scale, const float *bias, uint64_t bias_head_stride, void *out,
                                    uint64_t out_head_stride, uint32_t ldo, int out_bf16, float *lse) {
    return fwd_entry<ElemBf16>("attn_csr_bf16", "attn_csr_bf16<G%d,V%d,C%d>", stream, H, M, K, nnz, rowPtrs, colIdxs, Q, q_head_stride, ldq, Kmat,
                               k_head_stride, ldk, D, V, v_head_stride, ldv, Dv, scale, bias, bias_head_stride, out, out_head_stride, ldo, out_bf16,
                               lse);
}
