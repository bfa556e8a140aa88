"""Fused attention forward on a CSR pattern with every long row split over several lane groups (mispmm_attn_csr_split_f32 /
_bf16, libmispmm_attn_csr_split.so): two launches -- a partial kernel in which (head, row, segment of the row) is one lane group,
and a combine kernel that merges the segments' online-softmax states in a fixed order.  For few rows against very many keys
(decoding, chunked prefill against a long context) and for a pattern whose longest row decides the tail, where
ops.attention_csr / attn_csr_bf16.attention_csr_bf16 -- one lane group per row, walking the whole row alone -- leave the card
idle.  include/mispmm_attn_csr_split.h states the segments and the merge.  The operand contract is mispmm._attn_csr's."""
import torch

from . import _attn_csr, ops

MAX_SPLITS = 256
# the default rule (from profiles/attn_csr_split/probe.json): fill TARGET_WAVES waves' worth of lane
# groups, and leave every segment at least MIN_BATCHES batches of 8 entries of the mean row
TARGET_WAVES = 1024          # 256 CUs x 4 SIMDs x 1 wave: at M = 64 x 8192 keys and H = 8 the rule's S (8, 16, 4, 8) is the fastest
                             # measured in all four shapes, and 512 would cost 269 against 153 us; at H = 1 it overshoots by one
                             # doubling (3 to 39 % of a time 11 to 15 times under one launch)
MIN_BATCHES = 4              # not resolved by the kept run, which holds it fixed; also the default of the min_batches keyword

_EXPORTS = {_attn_csr.F32: ("capi_attn_csr_split", "mispmm_attn_csr_split_f32"),
            _attn_csr.BF16: ("capi_attn_csr_split", "mispmm_attn_csr_split_bf16")}


def _group(width, vec):
    """Lanes per (head, row) the library picks for max(D, Dv) = width at `vec` columns a lane (pick_group)."""
    need = -(-width // vec)
    return next((g for g in (8, 16, 32) if g >= need), 64)


def default_splits(a, heads, width, min_batches=MIN_BATCHES, wide=4):
    """The splits the fronts pick when given none: from the pattern's sizes alone, no device read.
    S = clamp(min(T // (M * H), mean_batches // min_batches), 1, 256), T = TARGET_WAVES * 64 // G lane groups, G the group of
    `width` = max(D, Dv) at 16-byte lanes (wide: 4 columns of float32, 8 of bf16); 1 means the one-launch kernel.  The mean
    cannot see one long row in a matrix of short ones: such a caller passes splits= explicitly."""
    rows = max(1, a.num_rows)
    target = TARGET_WAVES * 64 // _group(width, wide)
    mean_batches = a.nnz // (8 * rows)
    return max(1, min(target // (rows * max(1, heads)), mean_batches // min_batches, MAX_SPLITS))


def _check_splits(splits):
    if splits is None:
        return None
    if isinstance(splits, bool) or not isinstance(splits, int) or not 1 <= splits <= MAX_SPLITS:
        raise ValueError(f"splits must be None or an integer from 1 to {MAX_SPLITS}, not {splits!r}")
    return splits


def workspace_bytes(a, heads, dv, splits):
    from . import capi_attn_csr_split
    return int(capi_attn_csr_split.lib().mispmm_attn_csr_split_workspace(heads, a.num_rows, dv, splits))


def _split(name, kind, one_launch, a, q, k, v, scale, bias, out_bf16, return_lse, splits, min_batches, out, lse, workspace, stream):
    splits = _check_splits(splits)
    if isinstance(min_batches, bool) or not isinstance(min_batches, int) or min_batches < 1:
        raise ValueError(f"min_batches must be a positive integer, not {min_batches!r}")
    if splits is None:      # the front's first operand checks come before the rule reads a shape: the same first refusal on both paths
        _attn_csr._f32_pattern(name, a)
        (q3, _, _), _, (v3, _, _), _ = _attn_csr._qkv(kind, a, q, k, v)
        splits = default_splits(a, q3.shape[0], max(q3.shape[2], v3.shape[2]), min_batches, 8 if kind.narrows else 4)
        if splits == 1:
            return one_launch()
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous()):
        raise ValueError("workspace must be a contiguous 1-D uint8 tensor of at least workspace_bytes(a, H, Dv, splits) bytes")
    args, result, lse, heads, dv = _attn_csr._forward_args(name, kind, a, q, k, v, scale, bias, out_bf16, return_lse, out, lse, stream,
                                                           also=(workspace,))
    if workspace is None:
        workspace = torch.empty(workspace_bytes(a, heads, dv, splits), dtype=torch.uint8, device=q.device)
    _attn_csr._call(_EXPORTS[kind], *args, splits, min_batches, ops._p(workspace), workspace.numel())
    return (result, lse) if return_lse else result


def attention_csr_split(a, q, k, v, scale=None, bias=None, return_lse=False, splits=None, min_batches=MIN_BATCHES, out=None, lse=None,
                        workspace=None, stream=None):
    """ops.attention_csr -- its operands, its results, its special values -- with every row of at least 2 * min_batches batches
    of 8 entries dealt to up to `splits` lane groups, each holding at least min_batches batches.  splits: 1 .. 256, or None for
    default_splits(); where that rule gives 1 the call IS ops.attention_csr (one launch, no workspace), while an explicit
    splits=1 runs the two launches and returns the one-launch kernel's bits, as every shorter row does at any splits.  The rule
    works from the MEAN row and cannot see one long row in a matrix of short ones: such a caller passes splits= explicitly.
    workspace: a contiguous 1-D uint8 device tensor of at least workspace_bytes(a, H, Dv, splits) bytes, 16-byte aligned;
    allocated here (torch.empty) unless given.  The same (splits, min_batches) give the same bits run to run; different ones
    differ by roundings."""
    return _split("attention_csr_split", _attn_csr.F32,
                  lambda: ops.attention_csr(a, q, k, v, scale=scale, bias=bias, return_lse=return_lse, out=out, lse=lse, stream=stream),
                  a, q, k, v, scale, bias, False, return_lse, splits, min_batches, out, lse, workspace, stream)


def attention_csr_split_bf16(a, q, k, v, scale=None, bias=None, out_bf16=False, return_lse=False, splits=None, min_batches=MIN_BATCHES,
                             out=None, lse=None, workspace=None, stream=None):
    """attn_csr_bf16.attention_csr_bf16 (q, k, v int16 tensors of bf16 bits; out float32, or with out_bf16 bf16 bits) with long
    rows split as attention_csr_split splits them: the same keywords, the same rule, the same bits at splits=1."""
    from . import attn_csr_bf16
    return _split("attention_csr_split_bf16", _attn_csr.BF16,
                  lambda: attn_csr_bf16.attention_csr_bf16(a, q, k, v, scale=scale, bias=bias, out_bf16=out_bf16, return_lse=return_lse, out=out,
                                                           lse=lse, stream=stream),
                  a, q, k, v, scale, bias, out_bf16, return_lse, splits, min_batches, out, lse, workspace, stream)
