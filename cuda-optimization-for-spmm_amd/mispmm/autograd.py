"""Autograd for the CSR product: C = A @ B with A's values and B both trainable.

    a = TrainableCSR.from_host(csr)                    # patterns of A and A^T on the device, once
    w = torch.nn.Parameter(a.values)                   # A's values, in storage order
    c = spmm(a, w, b)                                  # forward: ops.spmm_csr
    c.sum().backward()                                 # w.grad: SDDMM on A's pattern; b.grad: the product with A^T

Both gradients are library kernels: grad_values[e] = <grad_C[row(e), :], B[col(e), :]> is ops.sddmm_csr, grad_B = A^T grad_C
is ops.spmm_csr on the transposed pattern with A's values gathered through the transpose's permutation, so the two stay tied
to one set of values.  float32 and float64; no double backward."""
import dataclasses
from dataclasses import dataclass

import torch
from torch.autograd.function import once_differentiable

from . import ops


@dataclass
class TrainableCSR:
    fwd: ops.DeviceCSR          # A's pattern (its data: the values at upload; spmm() multiplies by the values it is given)
    tpattern: ops.DeviceCSR     # A^T's pattern
    perm: torch.Tensor          # int64, device: entry t of A^T is entry perm[t] of A
    values: torch.Tensor        # a device copy of csr.data for the caller to wrap as a parameter

    @staticmethod
    def from_host(csr, device="cuda", dtype=torch.float32):
        """Both patterns are uploaded without a plan order (a plan permutes the values); the uniform-row hint and the span
        list index the arrays as they are and stay."""
        t_csr, perm = ops.csr_transpose(csr)
        fwd = ops.DeviceCSR.from_host(csr, device=device, plan=False, dtype=dtype)
        tpattern = ops.DeviceCSR.from_host(t_csr, device=device, plan=False, dtype=dtype)
        perm_dev = torch.from_numpy(perm.astype("int64")).to(device)
        return TrainableCSR(fwd, tpattern, perm_dev, fwd.data.clone())


class _SpmmCsr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, b, a, acc):
        ctx.a, ctx.acc = a, acc
        ctx.save_for_backward(values, b)
        return ops.spmm_csr(dataclasses.replace(a.fwd, data=values.detach().contiguous()), b.detach(), acc=acc)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_c):
        values, b = ctx.saved_tensors
        a, n = ctx.a, grad_c.shape[1]
        # e.g. C.sum().backward() hands in an expanded scalar, strides (0, 0)
        if grad_c.stride(1) != 1 or grad_c.stride(0) < n:
            grad_c = grad_c.contiguous()
        grad_values = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_values = ops.sddmm_csr(a.fwd, grad_c, b, acc=ctx.acc)
        if ctx.needs_input_grad[1]:
            grad_b = ops.spmm_csr(dataclasses.replace(a.tpattern, data=values[a.perm]), grad_c, acc=ctx.acc)
        return grad_values, grad_b, None, None


def spmm(a, values, b, acc="reference"):
    """C = A @ B, differentiable in `values` (A's entries in storage order, a.fwd.nnz of them) and in `b` ([K, N], row-major
    with unit column stride).  a: TrainableCSR; values and b device tensors of a's dtype.  A gradient is computed only for
    the inputs that require one."""
    ops._require_gpu(a.fwd.row_ptrs, values, b)
    dtype = a.fwd.data.dtype
    if values.dtype != dtype or b.dtype != dtype:
        raise ValueError(f"values and b must be {dtype}, like the matrix")
    if values.dim() != 1 or values.shape[0] != a.fwd.nnz:
        raise ValueError(f"values must hold the {a.fwd.nnz} entries of A")
    return _SpmmCsr.apply(values, b, a, acc)
