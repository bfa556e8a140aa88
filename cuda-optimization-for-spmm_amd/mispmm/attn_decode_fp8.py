"""Decode attention on a paged fp8 (e4m3) KV cache (mispmm_attn_decode_fp8, libmispmm_attn_fp8_decode.so): one query token per
sequence, H query heads over Hkv K / V heads, each sequence with its own list of cache pages and its own length.  Two launches:
a partial kernel in which (sequence, KV head, segment of the page list) is one wave that holds the H / Hkv query heads of the KV
group as rows of ONE MFMA tile -- K and V are read once per KV head, not once per query head -- and a combine kernel that merges
the segments' online-softmax states in a fixed order.  include/mispmm_attn_fp8_decode.h states the contract.  Thin plumbing, as
mispmm.attn_bsr_fp8_split, whose private helpers it uses."""
import torch

from .attn_bsr_fp8 import MAX_WIDTH, _bytes, _head_scale, _operand
from .attn_bsr_fp8_split import MAX_SPLITS, MIN_STEPS, TARGET_WAVES, _check_splits
from .ops import _flat, _p, _require_gpu, _stream_ptr

MAX_GROUP = 16         # query heads to a KV head: the rows of one MFMA tile


def default_splits(batch, kv_heads, num_pages, page_size):
    """The splits attention_decode_fp8 picks when it is given none: from the sizes alone, no device read.  The rule and the
    constants of attn_bsr_fp8_split.default_splits with batch * kv_heads waves in place of units * H:
    S = clamp(min(TARGET_WAVES // (B * Hkv), mean_steps // MIN_STEPS), 1, 64), a step being 32 keys of the mean sequence."""
    mean_steps = num_pages // (max(1, batch) * (2 if page_size == 16 else 1))
    return max(1, min(TARGET_WAVES // max(1, batch * kv_heads), mean_steps // MIN_STEPS, MAX_SPLITS))


def workspace_bytes(batch, heads, kv_group, dv, splits):
    from . import capi_attn_fp8_decode
    return int(capi_attn_fp8_decode.lib().mispmm_attn_decode_fp8_workspace(batch, heads, kv_group, dv, splits))


def attention_decode_fp8(page_ptrs, page_idxs, page_size, q, k, v, seq_lens=None, q_scale=None, k_scale=None, v_scale=None, scale=None,
                         out_bf16=False, return_lse=False, splits=None, out=None, lse=None, workspace=None, stream=None):
    """out[b, h] = v_scale * softmax(scale * q_scale * k_scale * q[b, h] K_b^T) V_b over the keys of sequence b, K_b and V_b of KV
    head h // (H // Hkv).  page_ptrs: int32 [B + 1], page_idxs: int32 [pages]: sequence b's keys are the page_size (16 or 32)
    rows of each cache page page_idxs[page_ptrs[b]:page_ptrs[b + 1]], in order -- what DeviceBSR.block_row_ptrs /
    block_col_idxs hold; sequences may share pages.  seq_lens: int32 [B] or None; the keys at positions >= seq_lens[b] are
    masked and the bytes behind them are never looked at (a page's tail may be uninitialised); None: every listed page is full.
    q: [B, H, D]; k: [Hkv, rows, D], v: [Hkv, rows, Dv] (2-D: Hkv = 1), rows a multiple of page_size, page p being rows
    p * page_size ..: torch.float8_e4m3fn tensors or their uint8 bytes with a contiguous last dimension and any other strides
    that meet the header's alignment (a cache stored [pages, page_size, Hkv, D] is a permuted view).  H // Hkv <= 16.
    q_scale: H elements or a float; k_scale, v_scale: Hkv elements or a float; None is no multiply.  scale defaults to
    D ** -0.5.  splits: 1 .. 64, or None for default_splits().  workspace: a uint8 device tensor of at least
    workspace_bytes(B, H, H // Hkv, Dv, splits) bytes, 16-byte aligned; allocated here unless given.  Returns out [B, H, Dv],
    float32 or int16 bf16 bits with out_bf16; with return_lse (out, lse [B, H]).  A sequence without unmasked keys gives +0
    and lse = -inf.  The same splits give the same bits run to run."""
    from . import capi_attn_fp8_decode
    splits = _check_splits(splits)
    _require_gpu(page_ptrs, page_idxs, seq_lens, q, k, v, out, lse, workspace)
    if page_size not in (16, 32):
        raise ValueError(f"page_size must be 16 or 32, not {page_size!r}")
    q = _bytes(q, "q")
    if q.dim() != 3 or (q.shape[2] > 1 and q.stride(2) != 1):
        raise ValueError(f"q must be [B, H, D] with a contiguous last dimension, not {tuple(q.shape)} with strides {tuple(q.stride())}")
    batch, heads, d = q.shape
    if k.dim() not in (2, 3) or k.dim() != v.dim():
        raise ValueError(f"k and v must both be [rows, width] or both [Hkv, rows, width], not {tuple(k.shape)}, {tuple(v.shape)}")
    rows = k.shape[-2]
    if rows % page_size != 0:
        raise ValueError(f"the {rows} rows of k must be a multiple of the page size {page_size}")
    k3, ldk, k_head = _operand(k, rows, None, "k")
    kv_heads = k3.shape[0]
    if kv_heads == 0 or heads % kv_heads != 0:
        raise ValueError(f"the {heads} heads of q must be a multiple of the {kv_heads} heads of k and v")
    group = heads // kv_heads
    if group > MAX_GROUP:
        raise ValueError(f"at most {MAX_GROUP} query heads to a K / V head, not {group}")
    v3, ldv, v_head = _operand(v, rows, kv_heads, "v")
    dv = v3.shape[2]
    if k3.shape[2] != d:
        raise ValueError(f"q and k must have the same number of columns, not {d} and {k3.shape[2]}")
    for width, step, what in ((d, 16, "D"), (dv, 8, "Dv")):
        if width == 0 or width % step != 0 or width > MAX_WIDTH:
            raise ValueError(f"the fp8 decode attention kernel takes {what} in multiples of {step} up to {MAX_WIDTH}, not {width}")
    _flat(page_ptrs, "page_ptrs", torch.int32, batch + 1)
    _flat(page_idxs, "page_idxs", torch.int32, page_idxs.numel())
    if seq_lens is not None:
        _flat(seq_lens, "seq_lens", torch.int32, batch)
    ldq, q_head = (q.stride(0) if batch > 1 else max(d, q.stride(0))), (q.stride(1) if heads > 1 else 0)
    if ldq < d or (heads > 1 and q_head < d):
        raise ValueError(f"q must not overlap its own rows (strides {tuple(q.stride())} for {d} columns), e.g. an expanded tensor")
    scales = [_head_scale(s, what, n, q.device) for s, what, n in ((q_scale, "q_scale", heads), (k_scale, "k_scale", kv_heads),
                                                                   (v_scale, "v_scale", kv_heads))]
    if scale is None:
        scale = d ** -0.5
    dtype, shape = (torch.int16 if out_bf16 else torch.float32), (batch, heads, dv)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=q.device)
    elif out.dtype != dtype or tuple(out.shape) != shape or (dv > 1 and out.stride(2) != 1) or (batch > 1 and out.stride(0) < dv) or \
            (heads > 1 and out.stride(1) < dv):
        raise ValueError(f"out must be a {dtype} tensor of shape {shape} with a contiguous last dimension")
    if lse is None and return_lse:
        lse = torch.empty(shape[:2], dtype=torch.float32, device=q.device)
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != shape[:2] or not lse.is_contiguous()):
        raise ValueError(f"lse must be a contiguous float32 tensor of shape {shape[:2]}")
    if splits is None:
        splits = default_splits(batch, kv_heads, page_idxs.numel(), page_size)
    need = workspace_bytes(batch, heads, group, dv, splits)
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)    # never a null pointer: the entry point refuses one
    elif workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"workspace must be a contiguous 1-D uint8 tensor of at least {need} bytes")
    capi_attn_fp8_decode.check(capi_attn_fp8_decode.lib().mispmm_attn_decode_fp8(
        _stream_ptr(stream), batch, heads, rows, page_size, page_idxs.numel(), _p(page_ptrs), _p(page_idxs), _p(seq_lens), _p(q), ldq, q_head,
        _p(k3), ldk, k_head, _p(v3), ldv, v_head, d, dv, float(scale), _p(scales[0]), _p(scales[1]), _p(scales[2]), _p(out),
        out.stride(0) if batch > 1 else max(dv, out.stride(0)), out.stride(1) if heads > 1 else 0, int(bool(out_bf16)), _p(lse), group, splits,
        _p(workspace), workspace.numel()))
    return (out, lse) if return_lse else out
