"""The fused block-sparse attention forward on e4m3 operands with every block row split over several waves and K / V heads
shared by groups of query heads (mispmm_attn_bsr_fp8_split, libmispmm_attn_fp8_split.so): two launches -- a partial kernel in
which (head, 16-row unit, segment of the block row) is one wave, and a combine kernel that merges the segments' online-softmax
states in a fixed order.  For what an fp8 KV cache is read at -- few query rows against very many keys, several query heads
over fewer K / V heads (grouped-query attention) -- where attn_bsr_fp8.attention_bsr_fp8, one wave per 16 rows walking the
whole block row alone and one K / V head per query head, leaves the card idle or needs K and V repeated.
include/mispmm_attn_fp8_split.h states the merge."""
import torch

from . import attn_bsr_fp8
from .ops import _p, _require_gpu

MAX_SPLITS = 64
# the default rule: the constants of attn_bsr_split, kept (item 35 says on what basis): fill
# TARGET_WAVES waves, and leave every segment at least MIN_STEPS 32-key steps of the mean block row
TARGET_WAVES = 1024
MIN_STEPS = 4


def default_splits(a, heads):
    """The splits attention_bsr_fp8_split picks when it is given none: from the pattern's sizes alone, no device read.
    S = clamp(min(TARGET_WAVES // (units * H), mean_steps // MIN_STEPS), 1, 64), H the query heads."""
    bs = a.block_row_size
    units = max(1, a.num_rows // 16)
    block_rows = max(1, a.num_rows // bs)
    mean_steps = a.num_blocks // (block_rows * (2 if bs == 16 else 1))
    return max(1, min(TARGET_WAVES // (units * max(1, heads)), mean_steps // MIN_STEPS, MAX_SPLITS))


def _check_splits(splits):
    if splits is None:
        return None
    if isinstance(splits, bool) or not isinstance(splits, int) or not 1 <= splits <= MAX_SPLITS:
        raise ValueError(f"splits must be None or an integer from 1 to {MAX_SPLITS}, not {splits!r}")
    return splits


def workspace_bytes(a, heads, dv, splits):
    from . import capi_attn_fp8_split
    return int(capi_attn_fp8_split.lib().mispmm_attn_bsr_fp8_split_workspace(heads, a.num_rows // a.block_row_size, a.block_row_size, dv, splits))


def attention_bsr_fp8_split(a, q, k, v, q_scale=None, k_scale=None, v_scale=None, scale=None, mask=None, out_bf16=False, return_lse=False,
                            splits=None, out=None, lse=None, workspace=None, stream=None):
    """attn_bsr_fp8.attention_bsr_fp8 -- its operands, its results, its special values -- with every block row dealt to `splits`
    waves, and with k and v of Hkv heads where H % Hkv == 0: query head h reads K / V head h // (H // Hkv).  A 2-D k and v
    beside a 3-D q is Hkv = 1.  k_scale and v_scale: Hkv elements or a float; q_scale: H elements or a float.
    splits: 1 .. 64, or None for default_splits(); where that rule gives 1 AND Hkv == H the call IS attention_bsr_fp8 (one
    launch, no workspace) -- with shared KV heads it always runs the split entry, which alone indexes them -- while an explicit
    splits=1 runs the two launches and, at Hkv == H, returns the one-launch kernel's bits.  workspace: a uint8 device tensor of
    at least workspace_bytes(a, H, Dv, splits) bytes, 16-byte aligned; allocated here (torch.empty) unless given.  The same
    splits give the same bits run to run; different splits differ by roundings."""
    from . import capi_attn_fp8_split
    splits = _check_splits(splits)
    _require_gpu(workspace)
    call, result, lse, heads, kv_heads, dv = attn_bsr_fp8._fp8_args(a, q, k, v, q_scale, k_scale, v_scale, scale, mask, out_bf16, return_lse, out,
                                                                    lse, stream, shared_kv=True)
    if splits is None:
        splits = default_splits(a, heads)
        if splits == 1 and kv_heads == heads:
            from . import capi_attn_fp8
            capi_attn_fp8.check(call(capi_attn_fp8.lib().mispmm_attn_bsr_fp8))
            return (result, lse) if return_lse else result
    need = workspace_bytes(a, heads, dv, splits)
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)    # never a null pointer: the entry point refuses one
    elif workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"workspace must be a contiguous 1-D uint8 tensor of at least {need} bytes")
    capi_attn_fp8_split.check(call(capi_attn_fp8_split.lib().mispmm_attn_bsr_fp8_split, heads // kv_heads, splits, _p(workspace), workspace.numel()))
    return (result, lse) if return_lse else result
