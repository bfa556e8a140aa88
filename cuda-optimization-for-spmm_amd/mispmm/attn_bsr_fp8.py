"""The fused block-sparse attention forward with Q, K and V in fp8 (OCP e4m3, torch.float8_e4m3fn) on MFMA
(mispmm_attn_bsr_fp8, libmispmm_attn_fp8.so) on torch tensors: thin plumbing from device memory and streams to the C ABI, as
mispmm.ops, whose private helpers it uses.  A module of its own: the table of tests/_ops_contract.py lists the public
functions of mispmm/ops.py, and these are not among them.

fp8 operands are torch.float8_e4m3fn tensors or their bytes as torch.uint8; the former are viewed as uint8, never copied."""
import torch

from .bsr_fp8 import E4M3_MAX, _bytes
from .ops import _block_array, _flat, _p, _require_gpu, _square_blocks, _stream_ptr

MAX_WIDTH = 128        # D (in multiples of 16) and Dv (in multiples of 8) up to this (include/mispmm_attn_fp8.h)


def _operand(t, rows, heads, what):
    """(t's bytes as [H, rows, width], row stride, head stride) of an e4m3 operand given as [rows, width] or [H, rows, width]."""
    t = _bytes(t, what)
    if t.dim() not in (2, 3):
        raise ValueError(f"{what} must be [{rows}, width] or [H, {rows}, width], not {tuple(t.shape)}")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.shape[1] != rows or (heads is not None and t.shape[0] != heads):
        raise ValueError(f"{what} must be [{rows}, width] or [{'H' if heads is None else heads}, {rows}, width], not {tuple(t.shape)}")
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError(f"{what} must have a contiguous last dimension")
    width = t.shape[2]
    ld = t.stride(1) if rows > 1 else max(width, t.stride(1))
    if ld < width or any(s < 0 for s in t.stride()):
        raise ValueError(f"{what} must not overlap its own rows (row stride {ld} < {width} columns), e.g. an expanded tensor")
    return t, ld, (t.stride(0) if t.shape[0] > 1 else 0)


def _head_scale(s, what, heads, device):
    """A per-head scale as the kernel reads it: None, a float32 device tensor of `heads` elements, or one made of a float."""
    if s is None:
        return None
    if isinstance(s, (int, float)):
        return torch.full((heads,), float(s), dtype=torch.float32, device=device)
    _require_gpu(s)
    _flat(s, what, torch.float32, heads)
    return s


def _fp8_args(a, q, k, v, q_scale, k_scale, v_scale, scale, mask, out_bf16, return_lse, out, lse, stream, shared_kv=False):
    """The checks and the operand preparation of both fp8 fronts: (call, result, lse, H, Hkv, Dv), call(entry, *more) making the
    C call.  shared_kv: k and v may hold Hkv heads with H % Hkv == 0 (2-D beside a 3-D q: Hkv = 1), and k_scale and
    v_scale Hkv elements; otherwise Hkv == H."""
    _require_gpu(a.block_row_ptrs, q, k, v, mask, out, lse)
    _square_blocks(a)
    bs = a.block_row_size
    if (q.dim() != k.dim() and not (shared_kv and q.dim() == 3 and k.dim() == 2)) or k.dim() != v.dim():
        raise ValueError(f"q, k and v must all be 2-D or all [H, ...], not {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    batched = q.dim() == 3
    q3, ldq, q_head = _operand(q, a.num_rows, None, "q")
    heads = q3.shape[0]
    k3, ldk, k_head = _operand(k, a.num_cols, None if shared_kv else heads, "k")
    kv_heads = k3.shape[0]
    if kv_heads == 0 or heads % kv_heads != 0:
        raise ValueError(f"the {heads} heads of q must be a multiple of the {kv_heads} heads of k and v")
    v3, ldv, v_head = _operand(v, a.num_cols, kv_heads, "v")
    d, dv = q3.shape[2], v3.shape[2]
    if k3.shape[2] != d:
        raise ValueError(f"q and k must have the same number of columns, not {d} and {k3.shape[2]}")
    for width, step, what in ((d, 16, "D"), (dv, 8, "Dv")):
        if width == 0 or width % step != 0 or width > MAX_WIDTH:
            raise ValueError(f"the fp8 fused attention kernel takes {what} in multiples of {step} up to {MAX_WIDTH}, not {width}")
    if mask is not None:
        _block_array(a, mask, (torch.float32,), "mask")
    scales = [_head_scale(s, what, n, q.device) for s, what, n in ((q_scale, "q_scale", heads), (k_scale, "k_scale", kv_heads),
                                                                   (v_scale, "v_scale", kv_heads))]
    if scale is None:
        scale = d ** -0.5
    dtype = torch.int16 if out_bf16 else torch.float32
    shape = (heads, a.num_rows, dv)
    if out is None:
        out3 = torch.empty(shape, dtype=dtype, device=q.device)
    else:
        out3 = out if batched else out.unsqueeze(0)
        if out.dtype != dtype or tuple(out3.shape) != shape or (dv > 1 and out3.stride(2) != 1) or out3.stride(1) < dv:
            raise ValueError(f"out must be a {dtype} tensor of shape {shape if batched else shape[1:]} with a contiguous last dimension")
    lse_shape = (heads, a.num_rows) if batched else (a.num_rows,)
    if lse is None and return_lse:
        lse = torch.empty(lse_shape, dtype=torch.float32, device=q.device)
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != lse_shape or not lse.is_contiguous()):
        raise ValueError(f"lse must be a contiguous float32 tensor of shape {lse_shape}")
    def call(entry, *more):
        """entry(the arguments of mispmm_attn_bsr_fp8 in its order, *more); the scales made of a float live until it returns."""
        return entry(_stream_ptr(stream), heads, a.num_rows // bs, a.num_cols, bs, a.num_blocks, _p(a.block_row_ptrs), _p(a.block_col_idxs),
                     _p(q3), ldq, q_head, _p(k3), ldk, k_head, _p(v3), ldv, v_head, d, dv, _p(mask), float(scale), _p(scales[0]), _p(scales[1]),
                     _p(scales[2]), _p(out3), out3.stride(1), out3.stride(0) if heads > 1 else 0, int(bool(out_bf16)), _p(lse), *more)
    return call, (out if out is not None else (out3 if batched else out3[0])), lse, heads, kv_heads, dv


def attention_bsr_fp8(a, q, k, v, q_scale=None, k_scale=None, v_scale=None, scale=None, mask=None, out_bf16=False, return_lse=False,
                      out=None, lse=None, stream=None):
    """Fused block-sparse attention forward on e4m3 operands (mispmm_attn_bsr_fp8): for every head, out = v_scale * softmax over
    each matrix row of (scale * q_scale * k_scale * q k^T + mask) on A's stored blocks, times v -- one launch for all heads.
    a: DeviceBSR [M x K] of 16 x 16 or 32 x 32 blocks (index arrays used); q: [M, D], k: [K, D], v: [K, Dv]
    torch.float8_e4m3fn tensors or their uint8 bytes, or [H, ...] with any head and row strides whose last dimension is
    contiguous (e.g. a permuted [M, H, D]) and that meet the header's alignment; D a multiple of 16 and Dv of 8, up to 128.
    q_scale, k_scale, v_scale: one scale per head, a float32 device tensor of H elements (what quantize_heads returned) or a
    Python float, finite and > 0; None is no multiply.  scale defaults to D ** -0.5; mask: float32 [num_blocks, bS, bS], -Inf =
    masked.  Returns out, [M, Dv] or [H, M, Dv], float32 or int16 bf16 bits with out_bf16; with return_lse (out, lse).  out=
    and lse= take the results where given: out of the result's shape with a contiguous last dimension, lse contiguous."""
    from . import capi_attn_fp8
    call, result, lse, _, _, _ = _fp8_args(a, q, k, v, q_scale, k_scale, v_scale, scale, mask, out_bf16, return_lse, out, lse, stream)
    capi_attn_fp8.check(call(capi_attn_fp8.lib().mispmm_attn_bsr_fp8))
    return (result, lse) if return_lse else result


def quantize_heads(x):
    """(x / scale as torch.float8_e4m3fn, scale): one float32 scale per head of x [H, rows, width] (a 2-D x is one head), the
    head's absmax brought to 448, the largest e4m3 number; an all-zero head gets scale 1.  Plain torch on x's device: a
    convenience, not a kernel."""
    if x.dim() not in (2, 3) or not x.is_floating_point():
        raise ValueError(f"x must be a 2-D or 3-D floating-point tensor, not {x.dtype} {tuple(x.shape)}")
    x3 = (x if x.dim() == 3 else x.unsqueeze(0)).to(torch.float32)
    absmax = x3.abs().amax(dim=(1, 2))
    scale = torch.where(absmax > 0, absmax / E4M3_MAX, torch.ones_like(absmax))
    # the clamp: the cast does not saturate, and x / scale may round a hair above 448
    q = (x3 / scale[:, None, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return (q if x.dim() == 3 else q[0]), scale
