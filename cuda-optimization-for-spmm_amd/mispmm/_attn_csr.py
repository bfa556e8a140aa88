"""The one front of the fused attention on a CSR pattern: forward, backward and bias gradient, for float32 operands and for
int16 tensors of bf16 bits.  ops.attention_csr / attention_csr_bwd, attn_csr_bf16.attention_csr_bf16 / _bwd and the two
functions of attn_csr_dbias are a few lines each over forward(), backward() and dbias() here, with the kind that names their
dtype, the words for it and their library.

The operand contract is that of the ops entry points: what the C ABI cannot see -- a dtype, a rank, a shape, a stride it would
read as unsigned -- is refused here with a ValueError that names the operand, before any call into a library.  The checks read
attributes only (dtype, shape, dim(), stride(), unsqueeze, is_cuda): no synchronisation, no allocation, no copy.  Only after
every defect is named: there is no CPU path (ops._require_gpu); only after that are the results and workspaces not given
allocated and an int64 perm converted.  ops._require_gpu, ops._p, ops._stream_ptr and each capi module's lib() and check are
looked up at call time, through their modules: the tests replace them by attribute."""
import importlib
from typing import NamedTuple

import torch

from . import ops

MAX_WIDTH = ops.ATTN_CSR_MAX_WIDTH     # D and Dv: 1 up to this (mispmm_attn_csr.h, mispmm_attn_csr_bf16.h)


class Kind(NamedTuple):
    dtype: torch.dtype      # of q, k, v and of the backward's grad_out
    words: str              # ... as a refusal names it
    narrows: bool           # the exports take out_bf16 / grads_bf16: a result may be bf16
    fwd: tuple              # (capi module, symbol) of the forward,
    bwd: tuple              # of the backward
    dbias: tuple            # and of the bias gradient


F32 = Kind(torch.float32, "a float32 tensor", False, ("capi_attn_csr", "mispmm_attn_csr_f32"),
           ("capi_attn_csr_bwd", "mispmm_attn_csr_bwd_f32"), ("capi_attn_csr_dbias", "mispmm_attn_csr_dbias_f32"))
BF16 = Kind(torch.int16, "an int16 tensor of bf16 bits", True, ("capi_attn_csr_bf16", "mispmm_attn_csr_bf16"),
            ("capi_attn_csr_bf16_bwd", "mispmm_attn_csr_bf16_bwd"), ("capi_attn_csr_dbias", "mispmm_attn_csr_dbias_bf16"))


def _call(export, *args):
    capi = importlib.import_module(f"{__package__}.{export[0]}")
    capi.check(getattr(capi.lib(), export[1])(*args))


def _operand(t, rows, heads, what, kind):
    """(t as [H, rows, width], row stride, head stride) of an operand given as [rows, width] or [H, rows, width]."""
    if t.dtype != kind.dtype:
        raise ValueError(f"{what} must be {kind.words}, not {t.dtype}")
    if t.dim() not in (2, 3):
        raise ValueError(f"{what} must be [{rows}, width] or [H, {rows}, width], not {tuple(t.shape)}")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.shape[1] != rows or (heads is not None and t.shape[0] != heads):
        raise ValueError(f"{what} must be [{rows}, width] or [{'H' if heads is None else heads}, {rows}, width], not {tuple(t.shape)}")
    width = t.shape[2]
    if width == 0 or width > MAX_WIDTH:
        raise ValueError(f"the fused CSR attention kernel takes widths from 1 to {MAX_WIDTH}: {what} has {width} columns")
    if width > 1 and t.stride(2) != 1:
        raise ValueError(f"{what} must have unit column stride, not {t.stride(2)}")
    if any(s < 0 for s in t.stride()):
        raise ValueError(f"{what} must not have a negative stride: {tuple(t.stride())}")
    ld = t.stride(1) if rows > 1 else max(width, t.stride(1))
    if ld < width:
        raise ValueError(f"{what} must not overlap its own rows (row stride {ld} < {width} columns), e.g. an expanded tensor")
    return t, ld, (t.stride(0) if t.shape[0] > 1 else 0)


def _f32_pattern(name, a):
    if a.data.dtype != torch.float32:
        raise ValueError(f"{name} takes a float32 DeviceCSR")


def _qkv(kind, a, q, k, v, *like_q):
    """_operand of q, k and v for the pattern a (k and v of q's heads, k of q's width); like_q: the further operands that are
    2-D or [H, ...] as q is.  Returns the three triples and whether the operands are [H, ...]."""
    q3 = _operand(q, a.num_rows, None, "q", kind)
    heads = q3[0].shape[0]
    k3 = _operand(k, a.num_cols, heads, "k", kind)
    v3 = _operand(v, a.num_cols, heads, "v", kind)
    if like_q:
        if len({t.dim() for t in (q, k, v, *like_q)}) != 1:
            raise ValueError("q, k, v, out and grad_out must all be 2-D or all [H, ...]")
    elif q.dim() != k.dim() or q.dim() != v.dim():
        raise ValueError(f"q, k and v must all be 2-D or all [H, ...], not {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if k3[0].shape[2] != q3[0].shape[2]:
        raise ValueError(f"q and k must have the same number of columns, not {q3[0].shape[2]} and {k3[0].shape[2]}")
    return q3, k3, v3, q.dim() == 3


def _bias_head(a, bias, heads):
    """Head stride of a float32 bias in a's entry order, [nnz] or [H, nnz]; 0: one bias for all heads, or none."""
    if bias is None:
        return 0
    if bias.dtype != torch.float32:
        raise ValueError(f"bias must be a float32 tensor, not {bias.dtype}")
    if tuple(bias.shape) not in ((a.nnz,), (heads, a.nnz)):
        raise ValueError(f"bias must have shape ({a.nnz},) or ({heads}, {a.nnz}), not {tuple(bias.shape)}")
    if a.nnz > 1 and bias.stride(-1) != 1:
        raise ValueError(f"bias must have unit stride along the entries, not {bias.stride(-1)}")
    if bias.dim() != 2 or heads == 1:
        return 0
    if bias.stride(0) < 0:
        raise ValueError("bias must not have a negative head stride")
    return bias.stride(0)


def _per_row(t, shape, what):
    """lse or delta: one float32 per (head, row), contiguous."""
    if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor of shape {shape}, not {t.dtype} {tuple(t.shape)} with strides "
                         f"{tuple(t.stride())}")


def _result(t, shape, batched, what, dtype=torch.float32, words="a float32 tensor"):
    """(t as [H, rows, width], row stride, head stride) of a tensor of the result's shape that the backward reads or writes."""
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {words}, not {t.dtype}")
    if t.dim() != (3 if batched else 2) or tuple((t if batched else t.unsqueeze(0)).shape) != shape:
        raise ValueError(f"{what} must have shape {shape if batched else shape[1:]}, not {tuple(t.shape)}")
    t3 = t if batched else t.unsqueeze(0)
    if shape[2] > 1 and t3.stride(2) != 1:
        raise ValueError(f"{what} must have unit column stride, not {t3.stride(2)}")
    if any(s < 0 for s in t3.stride()):
        raise ValueError(f"{what} must not have a negative stride: {tuple(t3.stride())}")
    if shape[1] > 1 and t3.stride(1) < shape[2]:
        raise ValueError(f"{what} must not overlap its own rows (row stride {t3.stride(1)} < {shape[2]} columns), e.g. an expanded tensor")
    return t3, (t3.stride(1) if shape[1] > 1 else max(shape[2], t3.stride(1))), (t3.stride(0) if shape[0] > 1 else 0)


def _written(kind, narrow, flag):
    """(dtype, words, the C argument) of a result that the keyword `flag` narrows to bf16; the float32 exports have no such
    argument and write float32."""
    if not kind.narrows:
        return torch.float32, "a float32 tensor", ()
    if narrow:
        return torch.int16, f"an int16 tensor of bf16 bits ({flag}=True)", (1,)
    return torch.float32, f"a float32 tensor ({flag}=False)", (0,)


def forward(name, kind, a, q, k, v, scale, bias, out_bf16, return_lse, out, lse, stream):
    _f32_pattern(name, a)
    (q3, ldq, q_head), (k3, ldk, k_head), (v3, ldv, v_head), batched = _qkv(kind, a, q, k, v)
    heads, d, dv = q3.shape[0], q3.shape[2], v3.shape[2]
    bias_head = _bias_head(a, bias, heads)
    if scale is None:
        scale = d ** -0.5
    shape = (heads, a.num_rows, dv)
    o_dtype, o_words, narrow = _written(kind, out_bf16, "out_bf16")
    out3 = None
    if out is not None:
        if out.dtype != o_dtype:
            raise ValueError(f"out must be {o_words}, not {out.dtype}")
        if out.dim() != q.dim() or tuple((out if batched else out.unsqueeze(0)).shape) != shape:
            raise ValueError(f"out must be {o_words} of shape {shape if batched else shape[1:]}, not {tuple(out.shape)}")
        out3 = out if batched else out.unsqueeze(0)
        if (dv > 1 and out3.stride(2) != 1) or any(s < 0 for s in out3.stride()) or (shape[1] > 1 and out3.stride(1) < dv) \
                or (heads > 1 and out3.stride(0) < 1):
            raise ValueError(f"out must have unit column stride and rows and heads that do not overlap, not strides {tuple(out.stride())}")
    lse_shape = (heads, a.num_rows) if batched else (a.num_rows,)
    if lse is not None:
        _per_row(lse, lse_shape, "lse")
    # every defect of an operand is named above, on tensors of any device; only then: there is no CPU path
    ops._require_gpu(a.row_ptrs, q, k, v, bias, out, lse)
    if out3 is None:
        out3 = torch.empty(shape, dtype=o_dtype, device=q.device)
    if lse is None and return_lse:
        lse = torch.empty(lse_shape, dtype=torch.float32, device=q.device)
    ldo = out3.stride(1) if shape[1] > 1 else max(dv, out3.stride(1))
    o_head = out3.stride(0) if heads > 1 else 0
    _p = ops._p
    _call(kind.fwd, ops._stream_ptr(stream), heads, a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs), _p(q3), q_head, ldq,
          _p(k3), k_head, ldk, d, _p(v3), v_head, ldv, dv, float(scale), _p(bias), bias_head, _p(out3), o_head, ldo, *narrow, _p(lse))
    result = out if out is not None else (out3 if batched else out3[0])
    return (result, lse) if return_lse else result


def _reads(kind, a, q, k, v, out, lse, grad_out, scale, bias):
    """What the backward and the bias gradient both read, checked: the C arguments from the pattern to grad_out's row stride,
    then (heads, d, dv, batched, the shape of lse)."""
    (q3, ldq, q_head), (k3, ldk, k_head), (v3, ldv, v_head), batched = _qkv(kind, a, q, k, v, out, grad_out)
    heads, d, dv = q3.shape[0], q3.shape[2], v3.shape[2]
    o3, ldo, o_head = _result(out, (heads, a.num_rows, dv), batched, "out")
    g3, ldg, g_head = _result(grad_out, (heads, a.num_rows, dv), batched, "grad_out", kind.dtype, kind.words)
    rows_shape = (heads, a.num_rows) if batched else (a.num_rows,)
    _per_row(lse, rows_shape, "lse")
    bias_head = _bias_head(a, bias, heads)
    if scale is None:
        scale = d ** -0.5
    _p = ops._p
    args = (_p(q3), q_head, ldq, _p(k3), k_head, ldk, d, _p(v3), v_head, ldv, dv, float(scale), _p(bias), bias_head, _p(o3), o_head, ldo,
            _p(lse), _p(g3), g_head, ldg)
    return args, heads, d, dv, batched, rows_shape


def backward(name, kind, a, at, perm, q, k, v, out, lse, grad_out, scale, bias, need, grads_bf16, dq, dk, dv, delta, stream):
    _f32_pattern(name, a)
    if (at.num_rows, at.num_cols, at.nnz) != (a.num_cols, a.num_rows, a.nnz):
        raise ValueError(f"at must be the pattern of A^T: {a.num_cols} x {a.num_rows} with {a.nnz} entries")
    reads, heads, d, dvw, batched, rows_shape = _reads(kind, a, q, k, v, out, lse, grad_out, scale, bias)
    if len(need) != 3:
        raise ValueError("need holds three flags: (dq, dk, dv)")
    if perm is not None:
        if perm.dtype not in (torch.int32, torch.int64) or perm.numel() != a.nnz:
            raise ValueError(f"perm must hold {a.nnz} int32 or int64 entry numbers, not {perm.numel()} of {perm.dtype}")
    elif bias is not None and (need[1] or need[2]):
        raise ValueError("with a bias, dk and dv need perm")
    g_dtype, g_words, narrow = _written(kind, grads_bf16, "grads_bf16")
    grads = []
    for wanted, given, rows, width, what in ((need[0], dq, a.num_rows, d, "dq"), (need[1], dk, a.num_cols, d, "dk"), (need[2], dv, a.num_cols, dvw, "dv")):
        if wanted and given is not None:
            _result(given, (heads, rows, width), batched, what, g_dtype, g_words)
        grads.append((wanted, given, (heads, rows, width), what))
    if (need[0] or need[1]) and delta is not None:
        _per_row(delta, rows_shape, "delta")
    # every defect of an operand is named above, on tensors of any device; only then: there is no CPU path
    ops._require_gpu(a.row_ptrs, at.row_ptrs, perm, q, k, v, out, lse, grad_out, bias, dq, dk, dv, delta)
    if perm is not None:
        perm = (perm.to(torch.int32) if perm.dtype == torch.int64 else perm).contiguous()
    placed = []
    for wanted, given, shape, what in grads:
        if not wanted:
            placed.append((None, None, 0, 0))
            continue
        if given is None:
            given = torch.empty(shape if batched else shape[1:], dtype=g_dtype, device=q.device)
        placed.append((given, *_result(given, shape, batched, what, g_dtype, g_words)))
    if (need[0] or need[1]) and delta is None:
        delta = torch.empty(rows_shape, dtype=torch.float32, device=q.device)
    (rq, q_out, lddq, dq_head), (rk, k_out, lddk, dk_head), (rv, v_out, lddv, dv_head) = placed
    _p = ops._p
    _call(kind.bwd, ops._stream_ptr(stream), heads, a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs), _p(at.row_ptrs),
          _p(at.col_idxs), _p(perm), *reads, _p(delta), *narrow, _p(q_out), dq_head, lddq, _p(k_out), dk_head, lddk, _p(v_out), dv_head, lddv)
    return rq, rk, rv


def dbias(name, kind, a, q, k, v, out, lse, grad_out, scale, bias, dbias, stream):
    _f32_pattern(name, a)
    reads, heads, _, _, batched, _ = _reads(kind, a, q, k, v, out, lse, grad_out, scale, bias)
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
    # every defect of an operand is named above, on tensors of any device; only then: there is no CPU path
    ops._require_gpu(a.row_ptrs, q, k, v, out, lse, grad_out, bias, dbias)
    if dbias is None:
        dbias = torch.empty(shape, dtype=torch.float32, device=q.device)
    dbias_head = dbias.stride(0) if batched and heads > 1 else a.nnz
    _p = ops._p
    _call(kind.dbias, ops._stream_ptr(stream), heads, a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs), *reads, _p(dbias),
          dbias_head)
    return dbias
