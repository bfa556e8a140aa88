"""The bias gradient of fused attention on a CSR pattern (mispmm_attn_csr_dbias_f32 / _bf16, libmispmm_attn_csr_dbias.so) on
torch tensors: the third entry of mispmm._attn_csr, the one front of the family, for its two kinds of operands.  A
module of its own, as mispmm/attn_csr_bf16.py and mispmm/sddmm_bf16.py are: the table of tests/_ops_contract.py lists the
public functions of mispmm/ops.py, and these are not among them.

The operand contract is that of ops.attention_csr_bwd and attn_csr_bf16.attention_csr_bf16_bwd: what the C ABI cannot see -- a
dtype, a rank, a shape, a stride it would read as unsigned -- is refused here with a ValueError that names the operand, before
any call into a library (mispmm._attn_csr holds the checks)."""
from . import _attn_csr


def attention_csr_dbias(a, q, k, v, out, lse, grad_out, scale=None, bias=None, dbias=None, stream=None):
    """The gradient of ops.attention_csr with respect to its bias (mispmm_attn_csr_dbias_f32): for every head and every stored
    entry e of row r, dbias[e] = P[e] (<grad_out[r], v[c]> - <grad_out[r], out[r]>) with P from the stored lse -- ONE launch for
    all heads, the scores and the weights never written.  It is the row pass of ops.attention_csr_bwd without its dq:
    dbias * scale is that pass's dS bit for bit.  Runs alone: no workspace, any order relative to attention_csr_bwd.
    a: the forward's float32 DeviceCSR; q, k, v, scale, bias: as in the forward; out, lse: what the forward returned; grad_out:
    float32 of out's shape.  2-D or [H, ...] operands with any head and row strides and unit column stride (a permuted
    [M, H, D]; k, v expanded over the heads).  bias=None: the gradient with respect to the scores' additive term all the same.
    Returns float32 [nnz] for 2-D operands and [H, nnz] for 3-D ones: ALWAYS per head -- for a bias shared by the heads, sum
    over dim 0.  dbias= takes the result where given (unit stride along the entries, heads that do not overlap)."""
    return _attn_csr.dbias("mispmm_attn_csr_dbias_f32", _attn_csr.F32, a, q, k, v, out, lse, grad_out, scale, bias, dbias, stream)


def attention_csr_dbias_bf16(a, q, k, v, out, lse, grad_out, scale=None, bias=None, dbias=None, stream=None):
    """The same for attn_csr_bf16.attention_csr_bf16 (mispmm_attn_csr_dbias_bf16): q, k, v and grad_out are int16 tensors of
    bf16 bits, widened exactly in the kernel; out and lse are the FLOAT32 ones the forward returned; bias and the result are
    float32.  On element lanes (V1) the result is attention_csr_dbias's on ops.bf16_to_f32 of the operands, bit for bit; on
    16-byte lanes a lane's dot-product chain covers 8 columns against 4."""
    return _attn_csr.dbias("mispmm_attn_csr_dbias_bf16", _attn_csr.BF16, a, q, k, v, out, lse, grad_out, scale, bias, dbias, stream)
