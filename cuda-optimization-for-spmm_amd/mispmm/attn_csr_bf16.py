"""Fused attention on a CSR pattern with q, k and v in bf16 (mispmm_attn_csr_bf16, libmispmm_attn_csr_bf16.so) and its fused
backward (mispmm_attn_csr_bf16_bwd, libmispmm_attn_csr_bf16_bwd.so) on torch tensors: the bf16 kind of mispmm._attn_csr, the one
front of the family, which holds the operand contract and the plumbing to the C ABI.  A module of its own: the table of
tests/_ops_contract.py lists the public functions of mispmm/ops.py, and these are not among them.

bf16 operands are int16 tensors of bf16 bits (the convention of ops.spmm_csr_bf16; torch_tensor.view(torch.int16) of a
bfloat16 tensor is one).  What the C ABI cannot see -- a dtype, a rank, a shape, a stride it would read as unsigned -- is
refused with a ValueError that names the operand, before any call into a library, on tensors of any device; only then: there
is no CPU path."""
from . import _attn_csr

MAX_WIDTH = _attn_csr.MAX_WIDTH     # D and Dv: 1 up to this (mispmm_attn_csr_bf16.h)


def attention_csr_bf16(a, q, k, v, scale=None, bias=None, out_bf16=False, return_lse=False, out=None, lse=None, stream=None):
    """Fused attention on a CSR pattern for bf16 q, k and v (mispmm_attn_csr_bf16): for every head, out = softmax over each
    row's stored entries of (scale * <q_r, k_c> + bias), times v -- one launch for all heads, fp32 arithmetic on the exactly
    widened operands, no fp32 copy of q, k or v and neither the scores nor the weights written.  On operands whose scores are
    exact in fp32 the result is ops.attention_csr's on ops.bf16_to_f32 of q, k, v, bit for bit.
    a: a float32 DeviceCSR [M x K] (index arrays used, values unread); q: [M, D], k: [K, D], v: [K, Dv] int16 tensors of bf16
    bits, or [H, ...] with any head and row strides and unit column stride (a permuted [M, H, D]; k, v expanded over the heads
    for multi-query attention); D and Dv from 1 to 256.  scale defaults to D ** -0.5.  bias: float32 [nnz], shared by the
    heads, or [H, nnz], in A's entry order, added to the scaled scores, -Inf = masked.  Returns out, [M, Dv] or [H, M, Dv]:
    float32, or with out_bf16 an int16 tensor of bf16 bits, the same fp32 result rounded once to nearest even.  With
    return_lse (out, lse), lse the float32 [M] or [H, M] log-sum-exp of each row.  out= and lse= take the results where given:
    out of the result's shape and of the dtype out_bf16 names, with unit column stride; lse contiguous.
    16-byte lanes (tag V8) need D, Dv and every row and head stride in multiples of 8 and 16-byte aligned bases; everything
    else runs on element lanes (V1)."""
    return _attn_csr.forward("attention_csr_bf16", _attn_csr.BF16, a, q, k, v, scale, bias, out_bf16, return_lse, out, lse, stream)


def attention_csr_bf16_bwd(a, at, perm, q, k, v, out, lse, grad_out, scale=None, bias=None, need=(True, True, True), grads_bf16=True,
                           dq=None, dk=None, dv=None, delta=None, stream=None):
    """Fused backward of attention_csr_bf16 (mispmm_attn_csr_bf16_bwd, libmispmm_attn_csr_bf16_bwd.so): (dq, dk, dv) for every
    head in at most two launches, reading bf16 -- fp32 arithmetic on the exactly widened operands, no fp32 copy of q, k, v or
    grad_out, and the scores, the weights and their gradients never written.  On element lanes (V1) the result is
    ops.attention_csr_bwd's on ops.bf16_to_f32 of the operands, bit for bit.
    a: the forward's float32 DeviceCSR; at, perm: A^T's pattern and the permutation of its entries (csr_transpose;
    TrainableCSR.tpattern / .perm32()), perm an integer device tensor (int64 is converted to 32 bits here), read only with a
    bias.  q, k, v, scale, bias: as in the forward, q, k, v int16 tensors of bf16 bits.  out, lse: the FLOAT32 out and lse the
    forward returned.  grad_out: an int16 tensor of bf16 bits of out's shape (a float32 grad_out is not built).  2-D or
    [H, ...] operands with any head and row strides and unit column stride.  need: which of (dq, dk, dv) to compute; the
    others come back None and their work is skipped.  grads_bf16: the gradients are int16 tensors of bf16 bits, the fp32
    accumulators rounded once to nearest even (the default), or float32.  dk and dv are [H, K, ...] also where k and v are one
    head expanded over all.  dq= / dk= / dv= take the gradients where given, of the dtype grads_bf16 names.  delta: a contiguous
    float32 workspace of lse's shape, allocated here unless given; needed for dq and dk.
    16-byte lanes (tag V8) need D, Dv and every row and head stride of q, k, v and grad_out in multiples of 8, those of out in
    multiples of 4, those of the gradients asked for in multiples of 8 (bf16) or 4 (float32), and 16-byte aligned bases;
    everything else runs on element lanes (V1)."""
    return _attn_csr.backward("attention_csr_bf16_bwd", _attn_csr.BF16, a, at, perm, q, k, v, out, lse, grad_out, scale, bias, need, grads_bf16,
                              dq, dk, dv, delta, stream)
