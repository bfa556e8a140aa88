"""The block-sparse product with A's blocks and B in fp8 (OCP e4m3, torch.float8_e4m3fn) on MFMA (mispmm_bsr_fp8,
libmispmm_bsr_fp8.so) on torch tensors: thin plumbing from device memory and streams to the C ABI, as mispmm.ops, whose
private helpers it uses.  A module of its own: the table of tests/_ops_contract.py lists the public functions of
mispmm/ops.py, and these are not among them.

fp8 operands are torch.float8_e4m3fn tensors or their bytes as torch.uint8; the former are viewed as uint8, never copied."""
import torch

from .ops import _dense, _dense_out, _flat, _p, _require_gpu, _stream_ptr

E4M3_MAX = 448.0


def _bytes(t, what):
    """t as uint8: an e4m3 tensor viewed, a uint8 tensor as it is."""
    if t.dtype == torch.float8_e4m3fn:
        return t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise ValueError(f"{what} must be a torch.float8_e4m3fn tensor or its bytes as torch.uint8, not {t.dtype}")
    return t


def _scale(t, what, count):
    if t is not None:
        _flat(t, what, torch.float32, count)
    return t


def spmm_bsr_fp8(a, blocks_fp8, b_fp8, row_scale=None, col_scale=None, out_bf16=False, out=None, stream=None):
    """C = diag(row_scale) (A @ B) diag(col_scale) on v_mfma_f32_16x16x32_fp8_fp8 in ONE launch (mispmm_bsr_fp8).
    a: DeviceBSR [M x K] of 16 x 16 or 32 x 32 blocks (index arrays used); blocks_fp8: A's blocks, a contiguous tensor of
    num_blocks * bS * bS e4m3 values in A's block order; b_fp8: [K, N] e4m3, unit column stride, any row stride of at least N;
    N and both row strides in multiples of 8.  row_scale [M], col_scale [N]: contiguous float32 or None -- what quantize_rows
    returned for A's rows and B's columns; None is no multiply.  Returns [M, N] float32, or int16 bf16 bits with out_bf16:
    fl(fl(acc * row_scale[i]) * col_scale[j]) with acc the fp32 sum (include/mispmm_bsr_fp8.h, NUMERICS).  out= takes the
    result where given: that shape and dtype, unit column stride, any row stride of at least N."""
    from . import capi_bsr_fp8
    blocks = _bytes(blocks_fp8, "blocks_fp8")
    b = _bytes(b_fp8, "b_fp8")
    _require_gpu(a.block_row_ptrs, blocks, b, row_scale, col_scale, out)
    bs = a.block_row_size
    if a.block_col_size != bs:
        raise ValueError(f"blocks must be square, not {bs} x {a.block_col_size}")
    _flat(blocks, "blocks_fp8", torch.uint8, a.num_blocks * bs * bs)
    ldb = _dense(b, "b_fp8", torch.uint8, a.num_cols)
    n = b.shape[1]
    _scale(row_scale, "row_scale", a.num_rows)
    _scale(col_scale, "col_scale", n)
    out, ldc = _dense_out(out, a.num_rows, n, b, torch.int16 if out_bf16 else torch.float32)
    capi_bsr_fp8.check(capi_bsr_fp8.lib().mispmm_bsr_fp8(
        _stream_ptr(stream), a.num_rows // bs, a.num_cols, bs, a.num_blocks, _p(a.block_row_ptrs), _p(a.block_col_idxs), _p(blocks), _p(b), n,
        ldb, _p(row_scale), _p(col_scale), _p(out), ldc, int(bool(out_bf16))))
    return out


def quantize_rows(x):
    """(x / scale as torch.float8_e4m3fn, scale): one float32 scale per row of the 2-D x, the row's absmax brought to 448, the
    largest e4m3 number; an all-zero row gets scale 1.  Plain torch on x's device: a convenience, not a kernel.  B's columns
    go through a transpose: q, s = quantize_rows(b.t()); b_fp8, col_scale = q.t().contiguous(), s."""
    if x.dim() != 2 or not x.is_floating_point():
        raise ValueError(f"x must be a 2-D floating-point tensor, not {x.dtype} {tuple(x.shape)}")
    x = x.to(torch.float32)
    absmax = x.abs().amax(dim=1)
    scale = torch.where(absmax > 0, absmax / E4M3_MAX, torch.ones_like(absmax))
    # the clamp: the cast does not saturate, and x / scale may round a hair above 448
    return (x / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn), scale
