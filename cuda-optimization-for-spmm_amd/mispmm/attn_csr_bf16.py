"""Fused attention on a CSR pattern with q, k and v in bf16 (mispmm_attn_csr_bf16, libmispmm_attn_csr_bf16.so) and its fused
backward (mispmm_attn_csr_bf16_bwd, libmispmm_attn_csr_bf16_bwd.so) on torch tensors: thin plumbing from device memory and streams to the C ABI, as mispmm.ops, whose private helpers it uses.  A module of its own:
the table of tests/_ops_contract.py lists the public functions of mispmm/ops.py, and these are not among them.

bf16 operands are int16 tensors of bf16 bits (the convention of ops.spmm_csr_bf16; torch_tensor.view(torch.int16) of a
bfloat16 tensor is one).  The operand contract is that of the ops entry points: what the C ABI cannot see -- a dtype, a rank,
a shape, a stride it would read as unsigned -- is refused here with a ValueError that names the operand, before any call into
a library.  The checks read attributes only: no synchronisation, no allocation, no copy."""
import torch

from . import ops
from .ops import _p, _require_gpu, _stream_ptr

MAX_WIDTH = ops.ATTN_CSR_MAX_WIDTH     # D and Dv: 1 up to this (mispmm_attn_csr_bf16.h)


def _operand(t, rows, heads, what, dtype=torch.int16, words="an int16 tensor of bf16 bits"):
    """(t as [H, rows, width], row stride, head stride) of an operand given as [rows, width] or [H, rows, width]."""
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {words}, not {t.dtype}")
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
    from . import capi_attn_csr_bf16
    if a.data.dtype != torch.float32:
        raise ValueError("attention_csr_bf16 takes a float32 DeviceCSR")
    q3, ldq, q_head = _operand(q, a.num_rows, None, "q")
    heads = q3.shape[0]
    k3, ldk, k_head = _operand(k, a.num_cols, heads, "k")
    v3, ldv, v_head = _operand(v, a.num_cols, heads, "v")
    if q.dim() != k.dim() or q.dim() != v.dim():
        raise ValueError(f"q, k and v must all be 2-D or all [H, ...], not {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    batched = q.dim() == 3
    if k3.shape[2] != q3.shape[2]:
        raise ValueError(f"q and k must have the same number of columns, not {q3.shape[2]} and {k3.shape[2]}")
    d, dv = q3.shape[2], v3.shape[2]
    bias_head = _bias_head(a, bias, heads)
    if scale is None:
        scale = d ** -0.5
    shape = (heads, a.num_rows, dv)
    o_dtype = torch.int16 if out_bf16 else torch.float32
    o_words = f"out must be {'an int16 tensor of bf16 bits (out_bf16=True)' if out_bf16 else 'a float32 tensor (out_bf16=False)'}"
    out3 = None
    if out is not None:
        if out.dtype != o_dtype:
            raise ValueError(f"{o_words}, not {out.dtype}")
        if out.dim() != q.dim() or tuple((out if batched else out.unsqueeze(0)).shape) != shape:
            raise ValueError(f"{o_words} of shape {shape if batched else shape[1:]}, not {tuple(out.shape)}")
        out3 = out if batched else out.unsqueeze(0)
        if (dv > 1 and out3.stride(2) != 1) or any(s < 0 for s in out3.stride()) or (shape[1] > 1 and out3.stride(1) < dv) \
                or (heads > 1 and out3.stride(0) < 1):
            raise ValueError(f"out must have unit column stride and rows and heads that do not overlap, not strides {tuple(out.stride())}")
    lse_shape = (heads, a.num_rows) if batched else (a.num_rows,)
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != lse_shape or not lse.is_contiguous()):
        raise ValueError(f"lse must be a contiguous float32 tensor of shape {lse_shape}, not {lse.dtype} {tuple(lse.shape)} with strides "
                         f"{tuple(lse.stride())}")
    # every defect of an operand is named above, on tensors of any device; only then: there is no CPU path
    _require_gpu(a.row_ptrs, q, k, v, bias, out, lse)
    if out3 is None:
        out3 = torch.empty(shape, dtype=o_dtype, device=q.device)
    if lse is None and return_lse:
        lse = torch.empty(lse_shape, dtype=torch.float32, device=q.device)
    ldo = out3.stride(1) if shape[1] > 1 else max(dv, out3.stride(1))
    o_head = out3.stride(0) if heads > 1 else 0
    capi_attn_csr_bf16.check(capi_attn_csr_bf16.lib().mispmm_attn_csr_bf16(
        _stream_ptr(stream), heads, a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs), _p(q3), q_head, ldq, _p(k3), k_head, ldk, d,
        _p(v3), v_head, ldv, dv, float(scale), _p(bias), bias_head, _p(out3), o_head, ldo, 1 if out_bf16 else 0, _p(lse)))
    result = out if out is not None else (out3 if batched else out3[0])
    return (result, lse) if return_lse else result


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
    from . import capi_attn_csr_bf16_bwd
    if a.data.dtype != torch.float32:
        raise ValueError("attention_csr_bf16_bwd takes a float32 DeviceCSR")
    if (at.num_rows, at.num_cols, at.nnz) != (a.num_cols, a.num_rows, a.nnz):
        raise ValueError(f"at must be the pattern of A^T: {a.num_cols} x {a.num_rows} with {a.nnz} entries")
    q3, ldq, q_head = _operand(q, a.num_rows, None, "q")
    heads = q3.shape[0]
    k3, ldk, k_head = _operand(k, a.num_cols, heads, "k")
    v3, ldv, v_head = _operand(v, a.num_cols, heads, "v")
    if len({q.dim(), k.dim(), v.dim(), out.dim(), grad_out.dim()}) != 1:
        raise ValueError("q, k, v, out and grad_out must all be 2-D or all [H, ...]")
    batched = q.dim() == 3
    if k3.shape[2] != q3.shape[2]:
        raise ValueError(f"q and k must have the same number of columns, not {q3.shape[2]} and {k3.shape[2]}")
    d, dvw = q3.shape[2], v3.shape[2]
    o3, ldo, o_head = _result(out, (heads, a.num_rows, dvw), batched, "out")
    g3, ldg, g_head = _result(grad_out, (heads, a.num_rows, dvw), batched, "grad_out", torch.int16, "an int16 tensor of bf16 bits")
    rows_shape = (heads, a.num_rows) if batched else (a.num_rows,)
    if lse.dtype != torch.float32 or tuple(lse.shape) != rows_shape or not lse.is_contiguous():
        raise ValueError(f"lse must be a contiguous float32 tensor of shape {rows_shape}, not {lse.dtype} {tuple(lse.shape)} with strides "
                         f"{tuple(lse.stride())}")
    bias_head = _bias_head(a, bias, heads)
    if len(need) != 3:
        raise ValueError("need holds three flags: (dq, dk, dv)")
    if perm is not None:
        if perm.dtype not in (torch.int32, torch.int64) or perm.numel() != a.nnz:
            raise ValueError(f"perm must hold {a.nnz} int32 or int64 entry numbers, not {perm.numel()} of {perm.dtype}")
    elif bias is not None and (need[1] or need[2]):
        raise ValueError("with a bias, dk and dv need perm")
    if scale is None:
        scale = d ** -0.5
    g_dtype = torch.int16 if grads_bf16 else torch.float32
    g_words = "an int16 tensor of bf16 bits (grads_bf16=True)" if grads_bf16 else "a float32 tensor (grads_bf16=False)"
    grads = []
    for wanted, given, rows, width, what in ((need[0], dq, a.num_rows, d, "dq"), (need[1], dk, a.num_cols, d, "dk"), (need[2], dv, a.num_cols, dvw, "dv")):
        if wanted and given is not None:
            _result(given, (heads, rows, width), batched, what, g_dtype, g_words)
        grads.append((wanted, given, (heads, rows, width), what))
    if (need[0] or need[1]) and delta is not None and (delta.dtype != torch.float32 or tuple(delta.shape) != rows_shape or not delta.is_contiguous()):
        raise ValueError(f"delta must be a contiguous float32 tensor of shape {rows_shape}, not {delta.dtype} {tuple(delta.shape)} with strides "
                         f"{tuple(delta.stride())}")
    # every defect of an operand is named above, on tensors of any device; only then: there is no CPU path
    _require_gpu(a.row_ptrs, at.row_ptrs, perm, q, k, v, out, lse, grad_out, bias, dq, dk, dv, delta)
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
    capi_attn_csr_bf16_bwd.check(capi_attn_csr_bf16_bwd.lib().mispmm_attn_csr_bf16_bwd(
        _stream_ptr(stream), heads, a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs), _p(at.row_ptrs), _p(at.col_idxs), _p(perm),
        _p(q3), q_head, ldq, _p(k3), k_head, ldk, d, _p(v3), v_head, ldv, dvw, float(scale), _p(bias), bias_head, _p(o3), o_head, ldo, _p(lse),
        _p(g3), g_head, ldg, _p(delta), 1 if grads_bf16 else 0, _p(q_out), dq_head, lddq, _p(k_out), dk_head, lddk, _p(v_out), dv_head, lddv))
    return rq, rk, rv
