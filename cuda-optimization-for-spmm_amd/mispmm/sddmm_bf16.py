"""SDDMM on a CSR pattern with x and y in bf16 (mispmm_sddmm_csr_bf16, libmispmm_sddmm_bf16.so) on torch tensors: thin
plumbing from device memory and streams to the C ABI, as mispmm.ops, whose private helpers it uses.  A module of its own:
the table of tests/_ops_contract.py lists the public functions of mispmm/ops.py, and this one is not among them.

bf16 operands are int16 tensors of bf16 bits (the convention of ops.spmm_csr_bf16; torch_tensor.view(torch.int16) of a
bfloat16 tensor is one).  The operand contract is that of the ops entry points: what the C ABI cannot see -- a dtype, a rank,
a shape, a stride it would read as unsigned -- is refused here with a ValueError that names the operand, before any call into
a library.  The checks read attributes only: no synchronisation, no allocation, no copy."""
import torch

from .ops import _acc_mode, _p, _require_gpu, _stream_ptr


def _operand(t, rows, what, of):
    """Row stride of a [rows, N] int16 operand of bf16 bits with unit column stride whose rows do not overlap."""
    if t.dtype != torch.int16:
        raise ValueError(f"{what} must be an int16 tensor of bf16 bits, not {t.dtype}")
    if t.dim() != 2 or t.shape[0] != rows:
        raise ValueError(f"{of}: {what} must be [{rows}, N], not {tuple(t.shape)}")
    width = t.shape[1]
    if width > 1 and t.stride(1) != 1:
        raise ValueError(f"{what} must have unit column stride, not {t.stride(1)}")
    if any(s < 0 for s in t.stride()):
        raise ValueError(f"{what} must not have a negative stride: {tuple(t.stride())}")
    ld = t.stride(0) if rows > 1 else max(width, t.stride(0))
    if ld < width:
        raise ValueError(f"{what} must not overlap its own rows (row stride {ld} < {width} columns), e.g. an expanded tensor")
    return ld


def sddmm_csr_bf16(a, x_bf16, y_bf16, out_bf16=False, out=None, acc="reference", stream=None):
    """out[e] = <x[row(e), :], y[col(e), :]> for every stored entry e of a (mispmm_sddmm_csr_bf16): the sampled dense-dense
    product on A's pattern for bf16 operands in ONE launch, fp32 or fp64 arithmetic on the exactly widened elements, no fp32
    copy of x or y.  acc="reference": an fp64 fused chain per lane, rounded to fp32 once -- the correctly rounded exact sum
    wherever that sum fits 53 bits; acc="fast": fp32 fused chains (include/mispmm_sddmm_bf16.h, NUMERICS).
    a: a DeviceCSR [M x K] of any value dtype (index arrays used, values unread); x_bf16: [M, N], y_bf16: [K, N] int16
    tensors of bf16 bits with unit column stride and any row stride >= N.  Returns [nnz] in A's storage order: float32, or
    with out_bf16 an int16 tensor of bf16 bits, the same fp32 result rounded once to nearest even.  out= takes the result
    where given: contiguous, nnz elements, of the dtype out_bf16 names.
    16-byte lanes (tag V8) need N and both row strides in multiples of 8 and 16-byte aligned bases; everything else runs on
    element lanes (V1)."""
    from . import capi_sddmm_bf16
    of = f"A is {a.num_rows} x {a.num_cols}"
    ldx = _operand(x_bf16, a.num_rows, "x_bf16", of)
    ldy = _operand(y_bf16, a.num_cols, "y_bf16", of)
    n = x_bf16.shape[1]
    if y_bf16.shape[1] != n:
        raise ValueError(f"x_bf16 and y_bf16 must have the same number of columns, not {n} and {y_bf16.shape[1]}")
    dtype = torch.int16 if out_bf16 else torch.float32
    words = "an int16 tensor of bf16 bits (out_bf16=True)" if out_bf16 else "a float32 tensor (out_bf16=False)"
    if out is not None:
        if out.dtype != dtype:
            raise ValueError(f"out must be {words}, not {out.dtype}")
        if out.dim() != 1 or out.shape[0] != a.nnz or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous 1-D tensor of the {a.nnz} entries of A, not {tuple(out.shape)} with strides "
                             f"{tuple(out.stride())}")
    mode = _acc_mode(acc)
    # every defect of an operand is named above, on tensors of any device; only then: there is no CPU path
    _require_gpu(a.row_ptrs, x_bf16, y_bf16, out)
    if out is None:
        out = torch.empty(a.nnz, dtype=dtype, device=x_bf16.device)
    capi_sddmm_bf16.check(capi_sddmm_bf16.lib().mispmm_sddmm_csr_bf16(
        _stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs), _p(x_bf16), ldx, _p(y_bf16), ldy, n, _p(out),
        1 if out_bf16 else 0, mode))
    return out
