"""The fp8 (OCP e4m3) block-sparse product on column-compacted strips in step slots (mispmm_bsrc_slots_fp8,
libmispmm_bsrc_fp8.so): the layout of ops.DeviceBSRCSlots with A's values and B as e4m3 bytes, on torch tensors.  Thin
plumbing as mispmm.bsr_fp8, whose byte and scale helpers it uses beside the private ones of mispmm.ops.  A module of its own:
the table of tests/_ops_contract.py lists the public functions of mispmm/ops.py, and these are not among them."""
import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import formats
from .bsr_fp8 import E4M3_MAX, _bytes, _scale
from .ops import _dense, _dense_out, _dev_u32, _p, _require_gpu, _stream_ptr, check_host


@dataclass
class DeviceBSRCSlotsFP8:
    """16-row strips of a BSR matrix of 16 x 16 or 32 x 32 blocks, column-compacted, in fixed step slots, values in e4m3
    (mispmm_bsr_compact_slots_fp8_host): one workgroup per strip."""
    num_rows: int
    num_cols: int
    num_steps: int           # extent of cols / tiles: 4 slots per strip + extra steps
    used_steps: int          # steps that hold values (MFMA K steps executed)
    extra_ptrs: torch.Tensor
    cols: torch.Tensor
    tiles: torch.Tensor      # uint8 e4m3 bytes, [num_steps, 16, 32]
    row_scale: Optional[torch.Tensor] = None   # from_host: the float32 scale of every matrix row, for spmm_bsrc_slots_fp8

    @staticmethod
    def from_blocks(bsr, blocks_fp8, device="cuda", check=True):
        """bsr: a host formats.BSR used for its pattern (its data is not read); blocks_fp8: num_blocks * bS * bS e4m3 values
        on the host, torch.float8_e4m3fn or their bytes as torch.uint8, in bsr's block order."""
        from . import capi_bsrc_fp8 as cb
        blocks = _bytes(blocks_fp8, "blocks_fp8")
        bs = bsr.block_row_size
        if bsr.block_col_size != bs:
            raise ValueError(f"blocks must be square, not {bs} x {bsr.block_col_size}")
        if blocks.is_cuda or not blocks.is_contiguous() or blocks.numel() != bsr.num_blocks * bs * bs:
            raise ValueError(f"blocks_fp8 must be a contiguous host tensor of {bsr.num_blocks * bs * bs} elements, not "
                             f"{tuple(blocks.shape)} on {blocks.device}")
        u32 = formats.as_u32 if check else (lambda _, x: np.ascontiguousarray(x, dtype=np.uint32).reshape(-1))
        ptrs, idxs = u32("blockRowPtrs", bsr.block_row_ptrs), u32("blockColIdxs", bsr.block_col_idxs)
        if ptrs.size != bsr.num_block_rows + 1:
            raise ValueError(f"bsr check: blockRowPtrs holds {ptrs.size} entries, M / bR + 1 = {bsr.num_block_rows + 1} are needed")
        data = blocks.numpy().reshape(-1)
        n, used = ctypes.c_uint32(0), ctypes.c_uint32(0)
        head = (bsr.num_block_rows, bsr.num_cols, bs, bsr.num_blocks, ptrs.ctypes.data, idxs.ctypes.data, data.ctypes.data,
                ctypes.byref(n), ctypes.byref(used))
        cb.check(cb.lib().mispmm_bsr_compact_slots_fp8_host(*head, None, None, None))     # the structure is checked here
        ep = np.empty(bsr.num_rows // 16 + 1, dtype=np.uint32)
        cl = np.empty(max(1, n.value) * 32, dtype=np.uint32)
        tl = np.empty(max(1, n.value) * 512, dtype=np.uint8)
        cb.check(cb.lib().mispmm_bsr_compact_slots_fp8_host(*head, ep.ctypes.data, cl.ctypes.data, tl.ctypes.data))
        return DeviceBSRCSlotsFP8(bsr.num_rows, bsr.num_cols, n.value, used.value, _dev_u32(ep, device), _dev_u32(cl, device),
                                  torch.from_numpy(tl).view(-1, 16, 32).to(device))

    @staticmethod
    def from_host(bsr, device="cuda", check=True):
        """Quantises bsr's float blocks per MATRIX row by bsr_fp8.quantize_rows' rule -- the row's absmax over all its blocks
        brought to 448, an all-zero row scaled by 1 -- and keeps the scales as row_scale."""
        if check:
            check_host(bsr)
        q, scale = quantize_bsr_rows(bsr)
        a = DeviceBSRCSlotsFP8.from_blocks(bsr, q, device, check=False)
        a.row_scale = scale.to(device)
        return a

    def operand_bytes(self):
        """Bytes of A one product must read: every slot's column list, the tiles of the used steps, the extra pointers."""
        return self.num_steps * 128 + self.used_steps * 512 + (self.num_rows // 16 + 1) * 4


def quantize_bsr_rows(bsr):
    """(blocks [num_blocks, bR, bC] as torch.float8_e4m3fn, scale [M] float32) of a host formats.BSR with float blocks: one
    scale per MATRIX row, over all the blocks of its block row, by bsr_fp8.quantize_rows' rule.  Plain torch on the host."""
    nbr, br = bsr.num_block_rows, bsr.block_row_size
    data = torch.from_numpy(np.ascontiguousarray(bsr.data, dtype=np.float32)).reshape(-1, br, bsr.block_col_size)
    brow = torch.from_numpy(np.repeat(np.arange(nbr), np.diff(np.asarray(bsr.block_row_ptrs).astype(np.int64))))
    absmax = torch.zeros((nbr, br)).scatter_reduce_(0, brow[:, None].expand(-1, br), data.abs().amax(dim=2), "amax")
    scale = torch.where(absmax > 0, absmax / E4M3_MAX, torch.ones_like(absmax))
    return (data / scale[brow][:, :, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn), scale.reshape(-1)


def spmm_bsrc_slots_fp8(a, b_fp8, row_scale=None, col_scale=None, out_bf16=False, out=None, stream=None):
    """C = diag(row_scale) (A @ B) diag(col_scale) on v_mfma_f32_16x16x32_fp8_fp8 in ONE launch (mispmm_bsrc_slots_fp8).
    a: DeviceBSRCSlotsFP8 [M x K]; b_fp8, row_scale (a.row_scale after from_host), col_scale, out_bf16 and out as
    bsr_fp8.spmm_bsr_fp8 takes them; None is no multiply.  Returns [M, N] float32, or int16 bf16 bits with out_bf16:
    fl(fl(acc * row_scale[i]) * col_scale[j]) with acc the fp32 sum (include/mispmm_bsrc_fp8.h, NUMERICS)."""
    from . import capi_bsrc_fp8 as cb
    b = _bytes(b_fp8, "b_fp8")
    _require_gpu(a.extra_ptrs, b, row_scale, col_scale, out)
    ldb = _dense(b, "b_fp8", torch.uint8, a.num_cols)
    n = b.shape[1]
    _scale(row_scale, "row_scale", a.num_rows)
    _scale(col_scale, "col_scale", n)
    out, ldc = _dense_out(out, a.num_rows, n, b, torch.int16 if out_bf16 else torch.float32)
    cb.check(cb.lib().mispmm_bsrc_slots_fp8(_stream_ptr(stream), a.num_rows // 16, a.num_cols, a.num_steps, _p(a.extra_ptrs), _p(a.cols),
                                            _p(a.tiles), _p(b), n, ldb, _p(row_scale), _p(col_scale), _p(out), ldc, int(bool(out_bf16))))
    return out
