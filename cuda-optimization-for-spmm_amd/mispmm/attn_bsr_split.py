"""Fused block-sparse attention forward in bf16 with every block row split over several waves (mispmm_attn_bsr_split_bf16,
libmispmm_attn_split.so): two launches -- a partial kernel in which (head, 16-row unit, segment of the block row) is one wave,
and a combine kernel that merges the segments' online-softmax states in a fixed order.  For few rows against very many keys
(decoding, chunked prefill against a long context) and for one head of a ragged pattern, where ops.attention_bsr_bf16 -- one
wave per 16 rows, walking the whole block row alone -- leaves the card idle.  include/mispmm_attn_split.h states the merge."""
import torch

from . import ops

MAX_SPLITS = 64
# the default rule (from profiles/attn_split/probe.json): fill TARGET_WAVES waves, and leave every
# segment at least MIN_STEPS 32-key steps of the mean block row
TARGET_WAVES = 1024          # 256 CUs x 4 SIMDs x 1 wave: at M = 64, H = 8 and 2048 steps, 1024 waves (S = 32) beat 2048 (S = 64)
MIN_STEPS = 4                # not resolved by the kept run: no shape of it has few units AND short rows


def default_splits(a, heads):
    """The splits attention_bsr_split_bf16 picks when it is given none: from the pattern's sizes alone, no device read.
    S = clamp(min(TARGET_WAVES // (units * H), mean_steps // MIN_STEPS), 1, 64); 1 means the one-wave kernel."""
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
    from . import capi_attn_split
    return int(capi_attn_split.lib().mispmm_attn_bsr_split_workspace(heads, a.num_rows // a.block_row_size, a.block_row_size, dv, splits))


def attention_bsr_split_bf16(a, q, k, v, scale=None, mask=None, out_bf16=False, return_lse=False, splits=None, out=None, lse=None,
                             workspace=None, stream=None):
    """ops.attention_bsr_bf16 -- its operands, its results, its special values -- with every block row dealt to `splits` waves.
    splits: 1 .. 64, or None for default_splits(); where that rule gives 1 the call IS ops.attention_bsr_bf16 (one launch, no
    workspace), while an explicit splits=1 runs the two launches and returns the one-wave kernel's bits.  workspace: a uint8
    device tensor of at least workspace_bytes(a, H, Dv, splits) bytes, 16-byte aligned; allocated here (torch.empty) unless
    given.  The same splits give the same bits run to run; different splits differ by roundings."""
    from . import capi_attn_split
    splits = _check_splits(splits)
    if splits is None:
        ops._require_gpu(a.block_row_ptrs, q)
        splits = default_splits(a, q.shape[0] if q.dim() == 3 else 1)
        if splits == 1:
            return ops.attention_bsr_bf16(a, q, k, v, scale=scale, mask=mask, out_bf16=out_bf16, return_lse=return_lse, out=out, lse=lse,
                                          stream=stream)
    ops._require_gpu(workspace)
    args, result, lse, heads, dv = ops._attn_bsr_args(a, q, k, v, scale, mask, out_bf16, return_lse, out, lse, stream)
    need = workspace_bytes(a, heads, dv, splits)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    elif workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous():
        raise ValueError(f"workspace must be a contiguous 1-D uint8 tensor of at least {need} bytes")
    capi_attn_split.check(capi_attn_split.lib().mispmm_attn_bsr_split_bf16(*args, splits, ops._p(workspace), workspace.numel()))
    return (result, lse) if return_lse else result
