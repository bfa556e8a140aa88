"""The bias gradient of fused attention on a CSR pattern (mispmm_attn_csr_dbias_f32 / _bf16, libmispmm_attn_csr_dbias.so) on
torch tensors: thin plumbing from device memory and streams to the C ABI, as mispmm.ops, whose private helpers it uses.  A
module of its own, as mispmm/attn_csr_bf16.py and mispmm/sddmm_bf16.py are: the table of tests/_ops_contract.py lists the
public functions of mispmm/ops.py, and these are not among them.

The operand contract is that of ops.attention_csr_bwd and attn_csr_bf16.attention_csr_bf16_bwd: what the C ABI cannot see -- a
dtype, a rank, a shape, a stride it would read as unsigned -- is refused here with a ValueError that names the operand, before
any call into a library.  The checks read attributes only: no synchronisation, no allocation, no copy."""
import torch

from .attn_csr_bf16 import _bias_head, _operand, _result
from .ops import _p, _require_gpu, _stream_ptr

_F32 = (torch.float32, "a float32 tensor")
_BF16 = (torch.int16, "an int16 tensor of bf16 bits")


def _dbias(name, kind, a, q, k, v, out, lse, grad_out, scale, bias, dbias, stream):
    from . import capi_attn_csr_dbias
    if a.data.dtype != torch.float32:
        raise ValueError(f"{name} takes a float32 DeviceCSR")
    q3, ldq, q_head = _operand(q, a.num_rows, None, "q", *kind)
    heads = q3.shape[0]
    k3, ldk, k_head = _operand(k, a.num_cols, heads, "k", *kind)
    v3, ldv, v_head = _operand(v, a.num_cols, heads, "v", *kind)
    if len({q.dim(), k.dim(), v.dim(), out.dim(), grad_out.dim()}) != 1:
        raise ValueError("q, k, v, out and grad_out must all be 2-D or all [H, ...]")
    batched = q.dim() == 3
    if k3.shape[2] != q3.shape[2]:
        raise ValueError(f"q and k must have the same number of columns, not {q3.shape[2]} and {k3.shape[2]}")
    d, dvw = q3.shape[2], v3.shape[2]
    o3, ldo, o_head = _result(out, (heads, a.num_rows, dvw), batched, "out")
    g3, ldg, g_head = _result(grad_out, (heads, a.num_rows, dvw), batched, "grad_out", *kind)
    rows_shape = (heads, a.num_rows) if batched else (a.num_rows,)
    if lse.dtype != torch.float32 or tuple(lse.shape) != rows_shape or not lse.is_contiguous():
        raise ValueError(f"lse must be a contiguous float32 tensor of shape {rows_shape}, not {lse.dtype} {tuple(lse.shape)} with strides "
                         f"{tuple(lse.stride())}")
    bias_head = _bias_head(a, bias, heads)
    shape = (heads, a.nnz) if batched else (a.nnz,)
    if dbias is not None:
        if dbias.dtype != torch.float32:
            raise ValueError(f"dbias must be a float32 tensor, not {dbias.dtype}")
        if tuple(dbias.shape) != shape:
            raise ValueError(f"dbias must have shape {shape}, not {tuple(dbias.shape)}")
        if a.nnz > 1 and dbias.stride(-1) != 1:
            raise ValueError(f"dbias must have unit stride along the entries, not {dbias.stride(-1)}")
        if batched and heads > 1 and dbias.stride(0) < a.nnz:
            raise ValueError(f"dbias must not overlap its own heads (head stride {dbias.stride(0)} < {a.nnz} entries): it is per head")
    if scale is None:
        scale = d ** -0.5
    # every defect of an operand is named above, on tensors of any device; only then: there is no CPU path
    _require_gpu(a.row_ptrs, q, k, v, out, lse, grad_out, bias, dbias)
    if dbias is None:
        dbias = torch.empty(shape, dtype=torch.float32, device=q.device)
    dbias_head = dbias.stride(0) if batched and heads > 1 else a.nnz
    capi_attn_csr_dbias.check(getattr(capi_attn_csr_dbias.lib(), name)(
        _stream_ptr(stream), heads, a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs), _p(q3), q_head, ldq, _p(k3), k_head, ldk, d,
        _p(v3), v_head, ldv, dvw, float(scale), _p(bias), bias_head, _p(o3), o_head, ldo, _p(lse), _p(g3), g_head, ldg, _p(dbias), dbias_head))
    return dbias


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
    return _dbias("mispmm_attn_csr_dbias_f32", _F32, a, q, k, v, out, lse, grad_out, scale, bias, dbias, stream)


def attention_csr_dbias_bf16(a, q, k, v, out, lse, grad_out, scale=None, bias=None, dbias=None, stream=None):
    """The same for attn_csr_bf16.attention_csr_bf16 (mispmm_attn_csr_dbias_bf16): q, k, v and grad_out are int16 tensors of
    bf16 bits, widened exactly in the kernel; out and lse are the FLOAT32 ones the forward returned; bias and the result are
    float32.  On element lanes (V1) the result is attention_csr_dbias's on ops.bf16_to_f32 of the operands, bit for bit; on
    16-byte lanes a lane's dot-product chain covers 8 columns against 4."""
    return _dbias("mispmm_attn_csr_dbias_bf16", _BF16, a, q, k, v, out, lse, grad_out, scale, bias, dbias, stream)
