"""Autograd for the CSR product, for attention on a CSR pattern (SDDMM, row softmax, product) and for the bf16 block-sparse
(BSR) product.  C = A @ B with A's values and B both trainable:

    a = TrainableCSR.from_host(csr)                    # patterns of A and A^T on the device, once
    w = torch.nn.Parameter(a.values)                   # A's values, in storage order
    c = spmm(a, w, b)                                  # forward: ops.spmm_csr
    c.sum().backward()                                 # w.grad: SDDMM on A's pattern; b.grad: the product with A^T

Both gradients are library kernels: grad_values[e] = <grad_C[row(e), :], B[col(e), :]> is ops.sddmm_csr, grad_B = A^T grad_C
is ops.spmm_csr on the transposed pattern with A's values gathered through the transpose's permutation, so the two stay tied
to one set of values.  float32 and float64; no double backward.

The same pattern carries an attention layer (GAT, graph transformers, masked attention on a fixed pattern):

    scores = sddmm(a, q * scale, k)                    # ops.sddmm_csr; backward: two products, with A's and A^T's pattern
    p = edge_softmax(a, scores)                        # ops.softmax_csr over every row's entries; backward: ops.softmax_csr_bwd
    out = spmm(a, p, v)                                # the product above
    out = sparse_attention(a, q, k, v)                 # the three lines as one call

Every step and every gradient is a library kernel; a mask is a -Inf score.  The block-sparse product:

    a = TrainableBSR.from_host(bsr)                    # 16 x 16 or 32 x 32 blocks: block patterns of A and A^T, once
    w = torch.nn.Parameter(a.blocks)                   # A's blocks in bfloat16, in storage order
    c = spmm_bsr(a, w, b)                              # forward: ops.spmm_bsr_bf16 (MFMA), b bfloat16
    c.sum().backward()                                 # w.grad: ops.sddmm_bsr_bf16; b.grad: ops.spmm_bsr_bf16 on A^T's pattern

Both gradients come back in bfloat16.  The CSR product with fp32 values and the activations in bfloat16:

    a = TrainableCSR.from_host(csr)                    # float32
    c = spmm_bf16(a, w, b)                             # forward: ops.spmm_csr_bf16, b bfloat16, c bfloat16 or float32
    c.sum().backward()                                 # b.grad (bfloat16): the same kernel on A^T; w.grad: ops.sddmm_csr, widened

    out = sparse_attention(a, q, k, v, fused=True)     # float32: one launch for all heads (ops.attention_csr), [H, ...] operands
    out = sparse_attention(a, q, k, v, fused=True, fused_backward=True)   # ... and the backward in at most two (ops.attention_csr_bwd)

    out = sparse_attention_bf16(a, q, k, v)            # bfloat16 q, k, v: one launch (attn_csr_bf16.attention_csr_bf16); the
                                                       # backward is ops.attention_csr_bwd on the widened operands

    out = sparse_attention(a, q, k, v, bias=b, bias_grad=True, fused=True, fused_backward=True)   # a TRAINED bias over A's entries
                                                       # ([nnz] or [H, nnz]): b.grad by one more launch for all heads
                                                       # (attn_csr_dbias.attention_csr_dbias); every other path takes the keyword too

Not built: COO / ELL patterns, bf16 for the softmax on a CSR pattern (SDDMM has it: sddmm_bf16.sddmm_csr_bf16, which
spmm_bf16(sddmm="bf16") uses), a head-summed bias gradient from the kernel (a bias shared by the heads gets the per-head result
summed by torch), the column-compacted block layouts (their tiles are built on the host from the values), a device kernel for
the blocks[perm] transpose."""
import dataclasses
from dataclasses import dataclass

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import ops


@dataclass
class TrainableCSR:
    fwd: ops.DeviceCSR          # A's pattern (its data: the values at upload; spmm() multiplies by the values it is given)
    tpattern: ops.DeviceCSR     # A^T's pattern
    perm: torch.Tensor          # int64, device: entry t of A^T is entry perm[t] of A
    values: torch.Tensor        # a device copy of csr.data for the caller to wrap as a parameter

    _perm32: tuple = dataclasses.field(default=None, repr=False, compare=False)   # (perm it was made from, its int32 copy)

    def perm32(self):
        """perm as the 32-bit array the fused attention backward reads: converted once per perm tensor, then kept."""
        if self._perm32 is None or self._perm32[0] is not self.perm:
            self._perm32 = (self.perm, self.perm.to(torch.int32).contiguous())
        return self._perm32[1]

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


class _SddmmCsr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, a, acc):
        ctx.a, ctx.acc = a, acc
        ctx.save_for_backward(x, y)
        return ops.sddmm_csr(a.fwd, x.detach(), y.detach(), acc=acc)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        a = ctx.a
        g = g.contiguous()
        grad_x = grad_y = None
        if ctx.needs_input_grad[0]:       # dX[r] = sum over row r of g[e] Y[col(e)]:  (A's pattern, values g) @ Y
            grad_x = ops.spmm_csr(dataclasses.replace(a.fwd, data=g), y, acc=ctx.acc)
        if ctx.needs_input_grad[1]:       # dY[c] = sum over column c of g[e] X[row(e)]:  (A^T's pattern, values g[perm]) @ X
            grad_y = ops.spmm_csr(dataclasses.replace(a.tpattern, data=g[a.perm]), x, acc=ctx.acc)
        return grad_x, grad_y, None, None


def _check_operand(t, rows, dtype, what):
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, like the matrix")
    if t.dim() != 2 or t.shape[0] != rows:
        raise ValueError(f"{what} must be [{rows}, N], not {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{what} must have unit column stride")


def sddmm(a, x, y, acc="reference"):
    """scores[e] = <x[row(e), :], y[col(e), :]> for every stored entry e of A, differentiable in x ([M, N]) and y ([K, N]).
    a: TrainableCSR (its values are not read); the forward is ops.sddmm_csr, each gradient one ops.spmm_csr with the incoming
    gradient as A's values -- on A's pattern for x, on A^T's for y -- and is computed only if its input requires one."""
    ops._require_gpu(a.fwd.row_ptrs, x, y)
    dtype = a.fwd.data.dtype
    _check_operand(x, a.fwd.num_rows, dtype, "x")
    _check_operand(y, a.fwd.num_cols, dtype, "y")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x and y must have the same number of columns, not {x.shape[1]} and {y.shape[1]}")
    return _SddmmCsr.apply(x, y, a, acc)


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, a, acc):
        p = ops.softmax_csr(a.fwd, scores.detach().contiguous(), acc=acc)
        ctx.a, ctx.acc = a, acc
        ctx.save_for_backward(p)
        return p

    @staticmethod
    @once_differentiable
    def backward(ctx, dp):
        (p,) = ctx.saved_tensors
        return ops.softmax_csr_bwd(ctx.a.fwd, p, dp.contiguous(), acc=ctx.acc), None, None


def edge_softmax(a, scores, acc="reference"):
    """The softmax of every row of A over its stored entries (ops.softmax_csr), differentiable in `scores` (a.fwd.nnz
    elements in storage order).  a: TrainableCSR.  The result is saved; the backward is ops.softmax_csr_bwd on it."""
    ops._require_gpu(a.fwd.row_ptrs, scores)
    if scores.dtype != a.fwd.data.dtype:
        raise ValueError(f"scores must be {a.fwd.data.dtype}, like the matrix")
    if scores.dim() != 1 or scores.shape[0] != a.fwd.nnz:
        raise ValueError(f"scores must hold the {a.fwd.nnz} entries of A")
    return _EdgeSoftmax.apply(scores, a, acc)


def _bias_grad(per_head, bias):
    """The gradient of `bias` from the per-head result ([nnz] for 2-D operands, [H, nnz]): a bias shared by the heads gets the
    heads' sum (one torch.sum), any other one the result in its own shape.  float32 throughout."""
    if per_head.dim() == 2 and bias.dim() == 1:
        return torch.sum(per_head, dim=0)
    return per_head.reshape(bias.shape)


# ---- what the fused attention on a CSR pattern, float32 and bfloat16, checks and does alike
def _of_dtype(t, dtype, what, like=None):
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}" + (like or f", not {t.dtype}"))


def _check_fused_qkv(a, q, k, v, dtype, like=None):
    """q, k and v of a fused call: all 2-D or all [H, ...] of `dtype`, the rows of A's pattern, q's heads, k of q's width."""
    if {t.dim() for t in (q, k, v)} not in ({2}, {3}):
        raise ValueError(f"q, k and v must all be 2-D or all [H, ...], not {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    for t, rows, what in ((q, a.fwd.num_rows, "q"), (k, a.fwd.num_cols, "k"), (v, a.fwd.num_cols, "v")):
        _of_dtype(t, dtype, what, like)
        if t.shape[-2] != rows or t.shape[:-2] != q.shape[:-2]:
            raise ValueError(f"{what} must be [{rows}, N] or [H, {rows}, N] with q's H, not {tuple(t.shape)}")
    if q.shape[-1] != k.shape[-1]:
        raise ValueError(f"q and k must have the same number of columns, not {q.shape[-1]} and {k.shape[-1]}")


def _bias_gate(bias, bias_grad, dtype, like=None):
    """A bias is a constant of `dtype` -- one that requires a gradient is refused -- unless bias_grad; a constant is detached."""
    if bias is None:
        return None
    if bias.requires_grad and not bias_grad:
        raise ValueError("bias is a constant: it gets no gradient and must not require one")
    _of_dtype(bias, dtype, "bias", like)
    return bias if bias.requires_grad else bias.detach()


def _dense_grad(grad_out):
    """grad_out as the library reads it: unit column stride, rows and heads that do not overlap -- else a contiguous copy
    (out.sum().backward() hands in an expanded scalar)."""
    if grad_out.stride(-1) != 1 or grad_out.stride(-2) < grad_out.shape[-1] or (grad_out.dim() == 3 and grad_out.stride(0) < 1):
        return grad_out.contiguous()
    return grad_out


def _lse_backward(ctx, bwd, dbias, q, k, v, out, lse, grad_out, **kw):
    """The tail of a backward that reads the saved out and lse: ONE `bwd` call if any of q, k, v needs a gradient, with `need`
    set from them (kw: further keywords of `bwd`), and one `dbias` call if the bias does.  Returns ((dq, dk, dv), grad_bias),
    None where not asked for."""
    a, needs = ctx.a, ctx.needs_input_grad
    grads, grad_bias = (None, None, None), None
    if any(needs[:3]):
        grads = bwd(a.fwd, a.tpattern, a.perm32(), q, k, v, out, lse, grad_out, scale=ctx.scale, bias=ctx.bias, need=tuple(needs[:3]), **kw)
    if needs[5]:
        grad_bias = _bias_grad(dbias(a.fwd, q, k, v, out, lse, grad_out, ctx.scale, ctx.bias), ctx.bias)
    return grads, grad_bias


class _FusedSparseAttention(torch.autograd.Function):
    """The forward in one launch for all heads (ops.attention_csr).  q, k, v are saved and the weights are not: the backward
    recomputes the scores and P head by head with the FAST kernels of the four-launch forward and runs its gradient chain, so
    the gradients are those of the unfused acc="fast" call, head by head, bit for bit.  The chain's ds (ops.softmax_csr_bwd) is
    the head's bias gradient: returned where the bias requires one (sparse_attention hands in a bias that does only with
    bias_grad=True)."""
    @staticmethod
    def forward(ctx, q, k, v, a, scale, bias):
        q, k, v = q.detach(), k.detach(), v.detach()
        bias = None if bias is None else bias.detach()
        ctx.a, ctx.scale, ctx.bias = a, scale, bias
        ctx.save_for_backward(q, k, v)
        return ops.attention_csr(a.fwd, q, k, v, scale=scale, bias=bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        a, needs, scale, bias = ctx.a, ctx.needs_input_grad, ctx.scale, ctx.bias
        if not any(needs[:3]) and not needs[5]:
            return (None,) * 6
        q, k, v = ctx.saved_tensors
        heads = [None] if q.dim() == 2 else range(q.shape[0])
        grads = ([], [], [])
        grads_b = []
        for h in heads:
            qh, kh, vh, gh = (t if h is None else t[h] for t in (q, k, v, grad_out))
            bh = bias if bias is None or bias.dim() == 1 else bias[h]
            gh = _dense_grad(gh)
            qs = qh * scale
            s = ops.sddmm_csr(a.fwd, qs, kh, acc="fast")
            p = ops.softmax_csr(a.fwd, s if bh is None else s + bh, acc="fast")
            grad_q = grad_k = grad_v = None
            if needs[2]:
                grad_v = ops.spmm_csr(dataclasses.replace(a.tpattern, data=p[a.perm]), gh, acc="fast")
            if needs[0] or needs[1] or needs[5]:
                dp = ops.sddmm_csr(a.fwd, gh, vh, acc="fast")
                ds = ops.softmax_csr_bwd(a.fwd, p, dp, acc="fast")
                grads_b.append(ds)
                if needs[0]:
                    grad_q = ops.spmm_csr(dataclasses.replace(a.fwd, data=ds), kh, acc="fast") * scale
                if needs[1]:
                    grad_k = ops.spmm_csr(dataclasses.replace(a.tpattern, data=ds[a.perm]), qs, acc="fast")
            for held, grad in zip(grads, (grad_q, grad_k, grad_v)):
                held.append(grad)
        merged = [None if held[0] is None else (held[0] if q.dim() == 2 else torch.stack(held)) for held in grads]
        grad_bias = _bias_grad(grads_b[0] if q.dim() == 2 else torch.stack(grads_b), bias) if needs[5] else None
        return (*merged, None, None, grad_bias)


class _FusedSparseAttentionFusedBwd(torch.autograd.Function):
    """Forward and backward fused (ops.attention_csr with its lse, ops.attention_csr_bwd): q, k, v, out and lse are saved, and
    the backward is ONE call, at most two launches for all heads, with `need` set from the inputs that require a gradient.  A
    bias that requires a gradient gets it by one launch more (attn_csr_dbias.attention_csr_dbias), made only then; the backward
    call is skipped where q, k and v need nothing."""
    @staticmethod
    def forward(ctx, q, k, v, a, scale, bias):
        q, k, v = q.detach(), k.detach(), v.detach()
        bias = None if bias is None else bias.detach()
        out, lse = ops.attention_csr(a.fwd, q, k, v, scale=scale, bias=bias, return_lse=True)
        ctx.a, ctx.scale, ctx.bias = a, scale, bias
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        from . import attn_csr_dbias
        needs = ctx.needs_input_grad
        if not any(needs[:3]) and not needs[5]:
            return (None,) * 6
        grads, grad_bias = _lse_backward(ctx, ops.attention_csr_bwd, attn_csr_dbias.attention_csr_dbias, *ctx.saved_tensors, _dense_grad(grad_out))
        return (*grads, None, None, grad_bias)


def _fused_sparse_attention(a, q, k, v, scale, bias, fused_backward=False):
    dtype = a.fwd.data.dtype
    if dtype != torch.float32:
        raise ValueError("fused=True takes a float32 matrix: the fused kernel has one arithmetic, fp32")
    _check_fused_qkv(a, q, k, v, dtype, ", like the matrix")
    for t, what in ((q, "q"), (k, "k"), (v, "v")):
        if t.shape[-1] > 1 and t.stride(-1) != 1:
            raise ValueError(f"{what} must have unit column stride")
    heads = q.shape[0] if q.dim() == 3 else 1
    if bias is not None and tuple(bias.shape) not in ((a.fwd.nnz,), (heads, a.fwd.nnz)):
        raise ValueError(f"bias must be [{a.fwd.nnz}] or [{heads}, {a.fwd.nnz}], not {tuple(bias.shape)}")
    if scale is None:
        scale = q.shape[-1] ** -0.5
    if fused_backward:
        return _FusedSparseAttentionFusedBwd.apply(q, k, v, a, float(scale), bias)
    return _FusedSparseAttention.apply(q, k, v, a, float(scale), bias)


def sparse_attention(a, q, k, v, scale=None, acc="reference", bias=None, fused=False, fused_backward=False, bias_grad=False):
    """Attention on A's pattern: row r attends to the columns A stores in row r.

        scores = sddmm(a, q * scale, k)        # [nnz]   <q_r, k_c> for every stored (r, c)
        p = edge_softmax(a, scores)            # [nnz]   softmax over each row's entries
        out = spmm(a, p, v)                    # [M, Dv] sum over the row of p[e] v[col(e)]

    a: TrainableCSR [M x K] (its values are not read); q: [M, D], k: [K, D], v: [K, Dv] device tensors of a's dtype (float32
    or float64), unit column stride.  scale defaults to D ** -0.5 and is applied to q by a torch multiply.  Differentiable in
    q, k and v; a row of A without entries gives a zero row.
    bias: a tensor of a's dtype over A's entries ([nnz]), added to the scores by a torch add before the softmax; -Inf = a
    masked entry.  It is a constant: one that requires a gradient is refused -- unless bias_grad=True (below).
    fused=True (float32 only; off by default): the forward is ONE launch for all heads (ops.attention_csr: online softmax in
    fp32, the scale applied to the scores by the kernel's fma, neither scores nor P written); q, k, v may then be [H, M, D] /
    [H, K, D] / [H, K, Dv] with any head and row strides and out is [H, M, Dv]; bias [nnz] or [H, nnz]; acc is not read: the
    kernel has one arithmetic, the FAST one.  out differs from the unfused result by roundings and is held to the same
    tolerance.  q, k, v are saved and P is not: the backward recomputes the scores and P per head with the FAST kernels
    (ops.sddmm_csr on q * scale, a torch add of the bias, ops.softmax_csr) and runs the chain above, so the gradients are the
    unfused acc="fast" path's, head by head, bit for bit.  Without bias and fused the call is what it always was.
    fused_backward=True (needs fused=True; off by default): the forward also returns its log-sum-exp and q, k, v, out and lse
    are saved; the backward is ONE ops.attention_csr_bwd call, at most two launches for all heads (a row pass for dq, a column
    pass on A^T's pattern for dk and dv), nothing recomputed through memory, work for inputs that need no gradient skipped.
    Its gradients are not the chain's bits -- P comes from the stored lse and the softmax backward's row term from
    <grad_out, out> -- and are held to derived tolerances (include/mispmm_attn_csr_bwd.h, NUMERICS).
    bias_grad=True (off by default): a bias that requires a gradient is accepted and gets one; the gradients of q, k and v are
    the same bits as with a constant bias.  Unfused: the torch add differentiates it.  fused=True: the recomputing backward's
    ds of each head (ops.softmax_csr_bwd) IS that head's bias gradient and is returned.  fused_backward=True: one launch more
    for all heads (attn_csr_dbias.attention_csr_dbias, include/mispmm_attn_csr_dbias.h), made only where the bias needs a
    gradient; ops.attention_csr_bwd is skipped where nothing else does.  A bias [nnz] shared by H heads gets the heads' sum (one
    torch.sum over the per-head result)."""
    if fused_backward and not fused:
        raise ValueError("fused_backward=True needs fused=True: the fused backward reads the fused forward's out and lse")
    ops._require_gpu(a.fwd.row_ptrs, q, k, v, bias)
    bias = _bias_gate(bias, bias_grad, a.fwd.data.dtype, ", like the matrix")
    if fused:
        return _fused_sparse_attention(a, q, k, v, scale, bias, fused_backward)
    dtype = a.fwd.data.dtype
    _check_operand(q, a.fwd.num_rows, dtype, "q")
    _check_operand(k, a.fwd.num_cols, dtype, "k")
    _check_operand(v, a.fwd.num_cols, dtype, "v")
    if q.shape[1] != k.shape[1]:
        raise ValueError(f"q and k must have the same number of columns, not {q.shape[1]} and {k.shape[1]}")
    if scale is None:
        scale = q.shape[1] ** -0.5
    if bias is None:
        return spmm(a, edge_softmax(a, sddmm(a, q * scale, k, acc=acc), acc=acc), v, acc=acc)
    if bias.dim() != 1 or bias.shape[0] != a.fwd.nnz:
        raise ValueError(f"bias must hold the {a.fwd.nnz} entries of A, not {tuple(bias.shape)}")
    return spmm(a, edge_softmax(a, sddmm(a, q * scale, k, acc=acc) + bias, acc=acc), v, acc=acc)


@dataclass
class TrainableBSR:
    fwd: ops.DeviceBSR          # A's block pattern (index arrays used; spmm_bsr() multiplies by the blocks it is given)
    tpattern: ops.DeviceBSR     # A^T's block pattern
    perm: torch.Tensor          # int64, device: block t of A^T is block perm[t] of A, its inner axes swapped
    blocks: torch.Tensor        # bfloat16 [num_blocks, bS, bS]: bsr.data rounded to nearest even, for the caller to wrap as a parameter

    _perm32: tuple = dataclasses.field(default=None, repr=False, compare=False)   # (perm it was made from, its int32 copy)

    def perm32(self):
        """perm as the int32 array the fused attention backward reads: converted once per perm tensor, then kept."""
        if self._perm32 is None or self._perm32[0] is not self.perm:
            self._perm32 = (self.perm, self.perm.to(torch.int32).contiguous())
        return self._perm32[1]

    @staticmethod
    def from_host(bsr, device="cuda"):
        if bsr.block_row_size != bsr.block_col_size or bsr.block_row_size not in (16, 32):
            raise ValueError(f"the bf16 block product takes 16 x 16 or 32 x 32 blocks, not {bsr.block_row_size} x {bsr.block_col_size}")
        t_bsr, perm = ops.bsr_transpose(bsr)
        bs = bsr.block_row_size
        blocks = torch.from_numpy(np.ascontiguousarray(bsr.data, dtype=np.float32).reshape(bsr.num_blocks, bs, bs)).to(torch.bfloat16)
        return TrainableBSR(ops.DeviceBSR.from_host(bsr, device=device), ops.DeviceBSR.from_host(t_bsr, device=device),
                            torch.from_numpy(perm.astype("int64")).to(device), blocks.to(device))


def _bits(t):
    return t.view(torch.int16)


class _SpmmBsrBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, blocks, b, a, out_bf16):
        ctx.a = a
        ctx.save_for_backward(blocks, b)
        c = ops.spmm_bsr_bf16(a.fwd, _bits(blocks.detach().contiguous()), _bits(b.detach()), out_bf16=out_bf16)
        return c.view(torch.bfloat16) if out_bf16 else c

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_c):
        blocks, b = ctx.saved_tensors
        a = ctx.a
        grad_c = grad_c.contiguous()           # e.g. C.sum().backward() hands in an expanded scalar, strides (0, 0)
        g = ops.f32_to_bf16(grad_c) if grad_c.dtype == torch.float32 else _bits(grad_c)
        grad_blocks = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_blocks = ops.sddmm_bsr_bf16(a.fwd, g, _bits(b), out_bf16=True).view(torch.bfloat16)
        if ctx.needs_input_grad[1]:
            t_blocks = blocks.detach()[a.perm].transpose(1, 2).contiguous()
            grad_b = ops.spmm_bsr_bf16(a.tpattern, _bits(t_blocks), g, out_bf16=True).view(torch.bfloat16)
        return grad_blocks, grad_b, None, None


def spmm_bsr(a, blocks, b, out_dtype=torch.float32):
    """C = A @ B on the bf16 MFMA kernels, differentiable in `blocks` ([num_blocks, bS, bS] bfloat16, A's blocks in storage
    order -- every element of a stored block is a parameter, its zeros included) and in `b` ([K, N] bfloat16, N a multiple of
    4).  a: TrainableBSR; out_dtype: torch.float32 or torch.bfloat16.  The forward is ops.spmm_bsr_bf16, bit for bit.  The
    backward makes grad_C contiguous and, where C is float32, rounds it to bfloat16 (to nearest even) first: both gradient
    kernels take bf16 operands.  grad_blocks = ops.sddmm_bsr_bf16(A's pattern, grad_C, B), grad_B = ops.spmm_bsr_bf16 on A^T's
    pattern with the blocks gathered through the transpose's permutation; both are accumulated in fp32, rounded once and
    returned as bfloat16.  A gradient is computed only for the inputs that require one."""
    ops._require_gpu(a.fwd.block_row_ptrs, blocks, b)
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16, not {out_dtype}")
    if blocks.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        raise ValueError("blocks and b must be torch.bfloat16")
    bs = a.fwd.block_row_size
    if tuple(blocks.shape) != (a.fwd.num_blocks, bs, bs):
        raise ValueError(f"blocks must hold the {a.fwd.num_blocks} blocks of A as [{a.fwd.num_blocks}, {bs}, {bs}], not {tuple(blocks.shape)}")
    if b.dim() != 2 or b.shape[0] != a.fwd.num_cols:
        raise ValueError(f"A has {a.fwd.num_cols} columns: b must be [{a.fwd.num_cols}, N], not {tuple(b.shape)}")
    if b.shape[1] % 4 != 0:
        raise ValueError(f"the bf16 block product takes N in multiples of 4, not {b.shape[1]}")
    if not b.is_contiguous():
        raise ValueError("b must be contiguous")
    return _SpmmBsrBf16.apply(blocks, b, a, out_dtype == torch.bfloat16)


# ---- attention on a block pattern in bf16: SDDMM (fp32 scores), row softmax (bf16 P), product
def _check_block_array(a, t, what):
    bs = a.fwd.block_row_size
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be torch.float32")
    if tuple(t.shape) != (a.fwd.num_blocks, bs, bs):
        raise ValueError(f"{what} must hold the {a.fwd.num_blocks} blocks of A as [{a.fwd.num_blocks}, {bs}, {bs}], not {tuple(t.shape)}")


def _check_out_dtype(out_dtype):
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16, not {out_dtype}")
    return out_dtype == torch.bfloat16


class _BlockSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, a, scale, mask, out_bf16):
        p = ops.softmax_bsr(a.fwd, scores.detach().contiguous(), scale=scale, mask=mask, out_bf16=out_bf16)
        ctx.a, ctx.scale = a, scale
        ctx.save_for_backward(p)
        return p.view(torch.bfloat16) if out_bf16 else p

    @staticmethod
    @once_differentiable
    def backward(ctx, dp):
        (p,) = ctx.saved_tensors
        return ops.softmax_bsr_bwd(ctx.a.fwd, p, dp.float().contiguous(), scale=ctx.scale), None, None, None, None


def block_softmax(a, scores, scale=1.0, mask=None, out_dtype=torch.float32):
    """The softmax of every matrix row of A over the elements of its stored blocks (ops.softmax_bsr), of scale * scores + mask,
    differentiable in `scores` ([num_blocks, bS, bS] float32 in A's block order); `mask` (float32, the same shape, -Inf = masked)
    is a constant.  a: TrainableBSR; out_dtype: torch.float32 or torch.bfloat16.  The result is saved in the out type; the
    backward is ops.softmax_bsr_bwd on it, with the incoming gradient widened to float32 and a float32 result."""
    ops._require_gpu(a.fwd.block_row_ptrs, scores, mask)
    out_bf16 = _check_out_dtype(out_dtype)
    _check_block_array(a, scores, "scores")
    if mask is not None:
        _check_block_array(a, mask, "mask")
        mask = mask.detach().contiguous()
    return _BlockSoftmax.apply(scores, a, float(scale), mask, out_bf16)


class _BlockSparseAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, a, scale, mask, out_bf16):
        q, k, v = q.detach(), k.detach(), v.detach()
        s = ops.sddmm_bsr_bf16(a.fwd, _bits(q), _bits(k))
        p = ops.softmax_bsr(a.fwd, s, scale=scale, mask=mask, out_bf16=True)
        out = ops.spmm_bsr_bf16(a.fwd, p, _bits(v), out_bf16=out_bf16)
        ctx.a, ctx.scale = a, scale
        ctx.save_for_backward(q, k, v, p)
        return out.view(torch.bfloat16) if out_bf16 else out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q, k, v, p = ctx.saved_tensors
        return (*_attention_grads(ctx.a, q, k, v, p, grad_out, ctx.scale, ctx.needs_input_grad), None, None, None, None)


def _attention_grads(a, q, k, v, p, grad_out, scale, needs):
    """(grad_q, grad_k, grad_v) of one head, bfloat16 or None where `needs` says so: the gradient chain block_sparse_attention
    documents, on the bf16 weights p ([num_blocks, bS, bS] int16 bits)."""
    grad_out = grad_out.contiguous()           # e.g. out.sum().backward() hands in an expanded scalar, strides (0, 0)
    g = ops.f32_to_bf16(grad_out) if grad_out.dtype == torch.float32 else _bits(grad_out)
    transposed = lambda blocks: blocks[a.perm].transpose(1, 2).contiguous()   # noqa: E731  A's blocks as A^T's
    grad_q = grad_k = grad_v = None
    if needs[2]:
        grad_v = ops.spmm_bsr_bf16(a.tpattern, transposed(p), g, out_bf16=True).view(torch.bfloat16)
    if needs[0] or needs[1]:
        dp = ops.sddmm_bsr_bf16(a.fwd, g, _bits(v))
        ds = ops.softmax_bsr_bwd(a.fwd, p, dp, scale=scale, out_bf16=True)
        if needs[0]:
            grad_q = ops.spmm_bsr_bf16(a.fwd, ds, _bits(k), out_bf16=True).view(torch.bfloat16)
        if needs[1]:
            grad_k = ops.spmm_bsr_bf16(a.tpattern, transposed(ds), _bits(q), out_bf16=True).view(torch.bfloat16)
    return grad_q, grad_k, grad_v


class _FusedBlockSparseAttention(torch.autograd.Function):
    """The forward in one launch for all heads (ops.attention_bsr_bf16).  q, k, v are saved and the weights are not: the
    backward recomputes S and P head by head with the kernels of the three-launch forward -- to the bits that forward would
    have saved -- and runs its gradient chain."""
    @staticmethod
    def forward(ctx, q, k, v, a, scale, mask, out_bf16, fused_backward=False):
        q, k, v = q.detach(), k.detach(), v.detach()
        ctx.a, ctx.scale, ctx.mask, ctx.fused_backward = a, scale, mask, fused_backward
        if fused_backward:                     # the backward kernels read the forward's out and its log-sum-exp
            out, lse = ops.attention_bsr_bf16(a.fwd, _bits(q), _bits(k), _bits(v), scale=scale, mask=mask, out_bf16=out_bf16, return_lse=True)
            ctx.save_for_backward(q, k, v, out, lse)
            return out.view(torch.bfloat16) if out_bf16 else out
        out = ops.attention_bsr_bf16(a.fwd, _bits(q), _bits(k), _bits(v), scale=scale, mask=mask, out_bf16=out_bf16)
        ctx.save_for_backward(q, k, v)
        return out.view(torch.bfloat16) if out_bf16 else out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        a, needs = ctx.a, ctx.needs_input_grad
        if not any(needs[:3]):
            return (None,) * 8
        if ctx.fused_backward:
            q, k, v, out, lse = ctx.saved_tensors
            grad_out = grad_out.contiguous()       # e.g. out.sum().backward() hands in an expanded scalar
            g = ops.f32_to_bf16(grad_out) if grad_out.dtype == torch.float32 else _bits(grad_out)
            grads = ops.attention_bsr_bwd_bf16(a.fwd, a.tpattern, a.perm32(), _bits(q), _bits(k), _bits(v), out, lse, g, scale=ctx.scale,
                                               mask=ctx.mask, grads_bf16=True, need=tuple(needs[:3]))
            return (*(None if x is None else x.view(torch.bfloat16) for x in grads), None, None, None, None, None)
        q, k, v = ctx.saved_tensors
        heads = [None] if q.dim() == 2 else range(q.shape[0])
        grads = ([], [], [])
        for h in heads:
            qh, kh, vh, gh = (t if h is None else t[h] for t in (q, k, v, grad_out))
            qh, kh, vh = qh.contiguous(), kh.contiguous(), vh.contiguous()
            s = ops.sddmm_bsr_bf16(a.fwd, _bits(qh), _bits(kh))
            p = ops.softmax_bsr(a.fwd, s, scale=ctx.scale, mask=ctx.mask, out_bf16=True)
            for held, grad in zip(grads, _attention_grads(a, qh, kh, vh, p, gh, ctx.scale, needs)):
                held.append(grad)
        merged = [None if held[0] is None else (held[0] if q.dim() == 2 else torch.stack(held)) for held in grads]
        return (*merged, None, None, None, None, None)


def block_sparse_attention(a, q, k, v, scale=None, mask=None, out_dtype=torch.float32, fused=False, fused_backward=False):
    """Attention on A's block pattern in bf16: matrix row r attends to the columns of the blocks A stores in r's block row.

        S = ops.sddmm_bsr_bf16(q, k)                               # fp32 [num_blocks, bS, bS]: <q_r, k_c>, fp32 accumulation
        P = ops.softmax_bsr(S, scale, mask, out_bf16=True)         # softmax of scale * S + mask per matrix row, bf16
        out = ops.spmm_bsr_bf16(P, v)                              # [M, Dv], fp32 accumulation

    a: TrainableBSR [M x K] (its values are not read); q: [M, D], k: [K, D], v: [K, Dv], bfloat16 and contiguous, D and Dv
    multiples of 4.  scale defaults to D ** -0.5 and is applied inside the softmax kernel, to the fp32 scores: q is not rounded
    again.  mask: float32 [num_blocks, bS, bS], added to the scaled scores, -Inf = masked (e.g. above the diagonal of the
    diagonal blocks for a block-causal pattern); a constant.  out_dtype: torch.float32 or torch.bfloat16.
    One autograd.Function, so that no bf16 intermediate is widened on the way.  Roundings: the scores stay fp32; P is the fp32
    softmax rounded to bf16 once (to nearest even) and is what the product multiplies by and what the backward reads; out is
    the fp32 sum, rounded once if bfloat16.  Backward: grad_out is made contiguous and, where float32, rounded to bf16 first
    (every kernel here takes bf16 operands); dV = ops.spmm_bsr_bf16 on A^T's pattern with P's blocks gathered through the
    transpose's permutation; dP = ops.sddmm_bsr_bf16(grad_out, v) in fp32; dS = ops.softmax_bsr_bwd(P, dP, scale) rounded to
    bf16 once; dQ = ops.spmm_bsr_bf16(dS, k); dK = ops.spmm_bsr_bf16 on A^T's pattern with dS's blocks gathered likewise and q.
    The three gradients are fp32 sums rounded once and returned as bfloat16.  Each gradient, and each kernel behind it, runs
    only if its input requires it.  A block row of A without blocks gives zero rows.
    fused=True: the forward is ONE launch for all heads (ops.attention_bsr_bf16: online softmax, neither S nor P written);
    q, k, v may then be [H, M, D] / [H, K, D] / [H, K, Dv] with any head and row strides (last dimension contiguous) and out
    is [H, M, Dv]; D and Dv multiples of 8 up to 128.  out differs from the unfused result by roundings (the weights are
    normalised by the sum of their bf16 values) and is held to the same tolerance.  q, k, v are saved and P is not: the
    backward recomputes S and P per head with ops.sddmm_bsr_bf16 / ops.softmax_bsr and runs the chain above unchanged, so the
    gradients are the unfused path's, bit for bit.  fused=False is the three-launch path, unchanged.
    fused_backward=True (only with fused=True; off by default): the forward also keeps its per-row log-sum-exp and saves q, k,
    v, out and lse; the backward makes grad_out contiguous, rounds a float32 grad_out to bf16 as above and is ONE
    ops.attention_bsr_bwd_bf16 call for all heads -- at most two launches, S, P, dP and dS never written -- asking only for the
    gradients autograd needs.  The gradients are bfloat16; they differ from the chain's by roundings (P is recomputed as
    exp(z - lse) in fp32 and dS uses delta = <grad_out, out> in place of <P, dP>) and are held to the derived tolerance of
    include/mispmm_attn_bwd.h."""
    ops._require_gpu(a.fwd.block_row_ptrs, q, k, v, mask)
    out_bf16 = _check_out_dtype(out_dtype)
    if fused_backward and not fused:
        raise ValueError("fused_backward=True is the backward of the fused forward: it needs fused=True")
    if fused:
        return _fused_block_sparse_attention(a, q, k, v, scale, mask, out_bf16, bool(fused_backward))
    for t, rows, what in ((q, a.fwd.num_rows, "q"), (k, a.fwd.num_cols, "k"), (v, a.fwd.num_cols, "v")):
        if t.dtype != torch.bfloat16:
            raise ValueError(f"{what} must be torch.bfloat16")
        if t.dim() != 2 or t.shape[0] != rows:
            raise ValueError(f"{what} must be [{rows}, N], not {tuple(t.shape)}")
        if t.shape[1] % 4 != 0:
            raise ValueError(f"the bf16 block product takes widths in multiples of 4: {what} has {t.shape[1]} columns")
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
    if q.shape[1] != k.shape[1]:
        raise ValueError(f"q and k must have the same number of columns, not {q.shape[1]} and {k.shape[1]}")
    if mask is not None:
        _check_block_array(a, mask, "mask")
        mask = mask.detach().contiguous()
    if scale is None:
        scale = q.shape[1] ** -0.5
    return _BlockSparseAttention.apply(q, k, v, a, float(scale), mask, out_bf16)


def _fused_block_sparse_attention(a, q, k, v, scale, mask, out_bf16, fused_backward=False):
    dims = {t.dim() for t in (q, k, v)}
    if dims not in ({2}, {3}):
        raise ValueError(f"q, k and v must all be 2-D or all [H, ...], not {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    for t, rows, what in ((q, a.fwd.num_rows, "q"), (k, a.fwd.num_cols, "k"), (v, a.fwd.num_cols, "v")):
        if t.dtype != torch.bfloat16:
            raise ValueError(f"{what} must be torch.bfloat16")
        if t.shape[-2] != rows or t.shape[:-2] != q.shape[:-2]:
            raise ValueError(f"{what} must be [{rows}, N] or [H, {rows}, N] with q's H, not {tuple(t.shape)}")
        if t.shape[-1] == 0 or t.shape[-1] % 8 != 0 or t.shape[-1] > ops.ATTN_MAX_WIDTH:
            raise ValueError(f"the fused attention kernel takes widths in multiples of 8 up to {ops.ATTN_MAX_WIDTH}: {what} has "
                             f"{t.shape[-1]} columns")
        if t.stride(-1) != 1:
            raise ValueError(f"{what} must have a contiguous last dimension")
    if q.shape[-1] != k.shape[-1]:
        raise ValueError(f"q and k must have the same number of columns, not {q.shape[-1]} and {k.shape[-1]}")
    if mask is not None:
        _check_block_array(a, mask, "mask")
        mask = mask.detach().contiguous()
    if scale is None:
        scale = q.shape[-1] ** -0.5
    return _FusedBlockSparseAttention.apply(q, k, v, a, float(scale), mask, out_bf16, fused_backward)


# ---- the CSR product with B in bf16 (ops.spmm_csr_bf16): fp32 values, bf16 activations
class _SpmmCsrBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, b, a, out_bf16, acc, sddmm):
        ctx.a, ctx.acc, ctx.sddmm = a, acc, sddmm
        ctx.save_for_backward(values, b)
        c = ops.spmm_csr_bf16(dataclasses.replace(a.fwd, data=values.detach().contiguous()), _bits(b.detach()), out_bf16=out_bf16, acc=acc)
        return c.view(torch.bfloat16) if out_bf16 else c

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_c):
        values, b = ctx.saved_tensors
        a = ctx.a
        grad_c = grad_c.contiguous()           # e.g. C.sum().backward() hands in an expanded scalar, strides (0, 0)
        g = ops.f32_to_bf16(grad_c) if grad_c.dtype == torch.float32 else _bits(grad_c)
        grad_values = grad_b = None
        if ctx.needs_input_grad[0]:
            if ctx.sddmm == "bf16":
                from . import sddmm_bf16
                grad_values = sddmm_bf16.sddmm_csr_bf16(a.fwd, g, _bits(b), acc=ctx.acc)
            else:
                grad_values = ops.sddmm_csr(a.fwd, ops.bf16_to_f32(g), ops.bf16_to_f32(_bits(b)), acc=ctx.acc)
        if ctx.needs_input_grad[1]:
            t = dataclasses.replace(a.tpattern, data=values.detach()[a.perm])
            grad_b = ops.spmm_csr_bf16(t, g, out_bf16=True, acc=ctx.acc).view(torch.bfloat16)
        return grad_values, grad_b, None, None, None, None


def spmm_bf16(a, values, b, out_dtype=torch.bfloat16, acc="fast", sddmm="f32"):
    """C = A @ B with the activations in bfloat16, differentiable in `values` (float32, A's entries in storage order) and in
    `b` ([K, N] bfloat16, unit column stride, any row stride).  a: a float32 TrainableCSR; out_dtype: torch.bfloat16 or
    torch.float32.  The forward is ops.spmm_csr_bf16, bit for bit (acc="reference": the CSR rule, a double sum).  The
    backward makes grad_C contiguous and, where C is float32, rounds it to bfloat16 (to nearest even) once, as spmm_bsr does.
    grad_b is the same kernel on A^T's pattern with values[a.perm] and comes back in bfloat16; grad_values is float32 and
    comes by the path `sddmm` names.  "f32" (the default): ops.sddmm_csr on grad_C and b widened to float32 (exact) by two
    ops.bf16_to_f32 launches.  "bf16": sddmm_bf16.sddmm_csr_bf16 on the bf16 grad_C and b themselves, one launch and no
    float32 copy of either; with acc="reference" it has the default path's bits wherever the exact sums fit 53 bits, with
    acc="fast" the order of its additions is its own on 16-byte lanes (include/mispmm_sddmm_bf16.h).  A gradient is computed
    only for the inputs that require one."""
    ops._require_gpu(a.fwd.row_ptrs, values, b)
    out_bf16 = _check_out_dtype(out_dtype)
    if a.fwd.data.dtype != torch.float32 or values.dtype != torch.float32:
        raise ValueError("spmm_bf16 takes a float32 matrix and float32 values")
    if b.dtype != torch.bfloat16:
        raise ValueError("b must be torch.bfloat16")
    if values.dim() != 1 or values.shape[0] != a.fwd.nnz:
        raise ValueError(f"values must hold the {a.fwd.nnz} entries of A")
    if b.dim() != 2 or b.shape[0] != a.fwd.num_cols:
        raise ValueError(f"A has {a.fwd.num_cols} columns: b must be [{a.fwd.num_cols}, N], not {tuple(b.shape)}")
    if b.shape[1] > 1 and b.stride(1) != 1:
        raise ValueError("b must have unit column stride")
    if acc not in ("reference", "fast"):
        raise ValueError(f"acc must be 'reference' or 'fast', not {acc!r}")
    if sddmm not in ("f32", "bf16"):
        raise ValueError(f"sddmm must be 'f32' or 'bf16', not {sddmm!r}")
    return _SpmmCsrBf16.apply(values, b, a, out_bf16, acc, sddmm)


# ---- fused attention on a CSR pattern with the activations in bf16 (attn_csr_bf16.attention_csr_bf16)
def _bf16_forward(ctx, q, k, v, a, scale, bias):
    """The forward of both Functions below: one launch for all heads, reading bf16; q, k, v, the fp32 out and lse are saved and
    the fp32 out returned."""
    from . import attn_csr_bf16
    q, k, v = q.detach(), k.detach(), v.detach()
    bias = None if bias is None else bias.detach()
    out, lse = attn_csr_bf16.attention_csr_bf16(a.fwd, _bits(q), _bits(k), _bits(v), scale=scale, bias=bias, return_lse=True)
    ctx.a, ctx.scale, ctx.bias = a, scale, bias
    ctx.save_for_backward(q, k, v, out, lse)
    return out


class _SparseAttentionBf16(torch.autograd.Function):
    """The forward in one launch for all heads, reading bf16 (fp32 out and lse); q, k, v, out and lse are saved.  The backward
    is ops.attention_csr_bwd on the widened q, k, v with the saved fp32 out and lse, every gradient rounded once.  A bias that
    requires a gradient gets it in fp32 by attn_csr_dbias.attention_csr_dbias on the same widened operands."""
    @staticmethod
    def forward(ctx, q, k, v, a, scale, bias, out_bf16):
        out = _bf16_forward(ctx, q, k, v, a, scale, bias)
        return ops.f32_to_bf16(out).view(torch.bfloat16) if out_bf16 else out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        from . import attn_csr_dbias
        needs = ctx.needs_input_grad
        if not any(needs[:3]) and not needs[5]:
            return (None,) * 7
        q, k, v, out, lse = ctx.saved_tensors
        if grad_out.dtype == torch.bfloat16:
            grad_out = ops.bf16_to_f32(_bits(grad_out))            # exact; a view that is not contiguous is copied there
        else:
            grad_out = _dense_grad(grad_out)
        qf, kf, vf = (ops.bf16_to_f32(_bits(t)) for t in (q, k, v))
        grads, grad_bias = _lse_backward(ctx, ops.attention_csr_bwd, attn_csr_dbias.attention_csr_dbias, qf, kf, vf, out, lse, grad_out)
        return (*(None if g is None else ops.f32_to_bf16(g).view(torch.bfloat16) for g in grads), None, None, grad_bias, None)


class _SparseAttentionBf16FusedBwd(torch.autograd.Function):
    """The same forward with a bfloat16 result; the backward is ONE attn_csr_bf16.attention_csr_bf16_bwd call on the saved q, k,
    v, fp32 out and lse and the bfloat16 grad_out: at most two launches for all heads, nothing widened or narrowed through
    memory, `need` set from the inputs that require a gradient.  A bias that requires a gradient gets it in fp32 by one launch
    more that reads bf16 itself (attn_csr_dbias.attention_csr_dbias_bf16)."""
    @staticmethod
    def forward(ctx, q, k, v, a, scale, bias):
        return ops.f32_to_bf16(_bf16_forward(ctx, q, k, v, a, scale, bias)).view(torch.bfloat16)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        from . import attn_csr_bf16, attn_csr_dbias
        needs = ctx.needs_input_grad
        if not any(needs[:3]) and not needs[5]:
            return (None,) * 6
        q, k, v, out, lse = ctx.saved_tensors
        grads, grad_bias = _lse_backward(ctx, attn_csr_bf16.attention_csr_bf16_bwd, attn_csr_dbias.attention_csr_dbias_bf16, _bits(q), _bits(k),
                                         _bits(v), out, lse, _bits(_dense_grad(grad_out)), grads_bf16=True)
        return (*(None if g is None else g.view(torch.bfloat16) for g in grads), None, None, grad_bias)


def sparse_attention_bf16(a, q, k, v, scale=None, bias=None, out_dtype=torch.bfloat16, fused_backward=False, bias_grad=False):
    """Attention on A's pattern with the activations in bfloat16: row r attends to the columns A stores in row r, one launch
    for all heads (attn_csr_bf16.attention_csr_bf16: fp32 arithmetic on the exactly widened operands, online softmax, neither
    scores nor weights written, no fp32 copy of q, k or v).
    a: a float32 TrainableCSR [M x K] (its values are not read); q: [M, D], k: [K, D], v: [K, Dv] torch.bfloat16 device
    tensors, or [H, ...] with any head and row strides and unit column stride; D and Dv from 1 to 256.  scale defaults to
    D ** -0.5.  bias: a float32 tensor over A's entries, [nnz] or [H, nnz], added to the scaled scores, -Inf = a masked entry;
    a constant: one that requires a gradient is refused -- unless bias_grad=True (below).  out_dtype: torch.bfloat16 (the default) or torch.float32.  The
    kernel is always asked for its fp32 out and lse, which the backward reads; a bfloat16 result is ops.f32_to_bf16 of that
    out -- ONE extra elementwise launch, the same single rounding to nearest even the kernel's own bf16 store makes.
    Differentiable in q, k and v.  The backward is DEFINED as ops.attention_csr_bwd (at most two launches for all heads) on
    ops.bf16_to_f32 of q, k and v with the saved fp32 out and lse; grad_out is widened exactly where it is bfloat16 and used as
    it is where float32; work for inputs that need no gradient is skipped; every gradient is rounded once by ops.f32_to_bf16
    and comes back in bfloat16 (the three widenings and their fp32 copies are the cost of this one).
    fused_backward=True (needs out_dtype=torch.bfloat16; off by default): the backward is ONE
    attn_csr_bf16.attention_csr_bf16_bwd call on the saved q, k, v, fp32 out and lse and the bfloat16 grad_out -- at most two
    launches for all heads that read bf16 themselves and round each gradient once at the store; a grad_out that is not
    unit-stride with rows that do not overlap is made contiguous first.  On 16-byte lanes its gradients are not the default
    backward's bits (a lane's dot-product chain covers 8 columns against 4) and are held to the same derived tolerances.
    Not built: a fused backward for a float32 grad_out, which is why the keyword is refused with out_dtype=torch.float32.
    bias_grad=True (off by default): a bias that requires a gradient is accepted and gets one, in float32, by one launch more
    for all heads, made only then: attn_csr_dbias.attention_csr_dbias on the widened operands the default backward holds, or
    with fused_backward=True attn_csr_dbias.attention_csr_dbias_bf16, which reads bf16 itself.  The backward call proper is
    skipped where q, k and v need nothing; their gradients are the same bits as with a constant bias.  A bias [nnz] shared by
    H heads gets the heads' sum (one torch.sum over the per-head result)."""
    if fused_backward and out_dtype == torch.float32:
        raise ValueError("fused_backward=True needs out_dtype=torch.bfloat16: with a float32 out, grad_out would be float32, and the fused "
                         "bf16 backward reads a bfloat16 grad_out")
    ops._require_gpu(a.fwd.row_ptrs, q, k, v, bias)
    out_bf16 = _check_out_dtype(out_dtype)
    if a.fwd.data.dtype != torch.float32:
        raise ValueError("sparse_attention_bf16 takes a float32 matrix")
    _check_fused_qkv(a, q, k, v, torch.bfloat16)
    bias = _bias_gate(bias, bias_grad, torch.float32)
    if scale is None:
        scale = q.shape[-1] ** -0.5
    if fused_backward:
        return _SparseAttentionBf16FusedBwd.apply(q, k, v, a, float(scale), bias)
    return _SparseAttentionBf16.apply(q, k, v, a, float(scale), bias, out_bf16)
