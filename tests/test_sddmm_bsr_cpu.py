"""The block SDDMM and the transposed block pattern on a machine WITHOUT a GPU: ops.bsr_transpose against the dense transpose,
mispmm_sddmm_bsr_bf16's argument validation (which happens before any device work) and the Python layer's refusal of CPU
tensors."""
import ctypes

import numpy as np
import pytest

from mispmm import capi, formats, ops

from _sddmm_bsr_ref import RAGGED16_COUNTS, RAGGED32_COUNTS, block_rows, pattern

PATTERNS = ["ragged16", "ragged32", "ACTIVSg10K"]


def _canonical(bsr):
    """The dense form without the zeros between blocks: (block row, block column, block), sorted by coordinate.  No pattern
    here repeats a block coordinate, so two BSRs have one dense form exactly when these agree (ACTIVSg10K's dense form itself
    is 1.6 GB)."""
    rows, cols = block_rows(bsr), np.asarray(bsr.block_col_idxs, dtype=np.int64)
    key = rows * (bsr.num_cols // bsr.block_col_size) + cols
    assert np.unique(key).shape[0] == key.shape[0]
    order = np.argsort(key)
    return rows[order], cols[order], np.asarray(bsr.data)[order]


def test_patterns_cover_what_they_claim():
    for name, counts, bs, odd in (("ragged16", RAGGED16_COUNTS, 16, (3, 5)), ("ragged32", RAGGED32_COUNTS, 32, (2,))):
        p = pattern(name)
        ptrs = p.block_row_ptrs.astype(np.int64)
        assert np.diff(ptrs).tolist() == counts and p.block_row_size == p.block_col_size == bs
        assert p.data.shape == (p.num_blocks, bs, bs) and 0 in counts
        unsorted = [r for r in range(len(counts)) if np.any(np.diff(p.block_col_idxs[ptrs[r]:ptrs[r + 1]].astype(np.int64)) < 0)]
        assert tuple(unsorted) == odd
    assert RAGGED16_COUNTS[-1] == 0 and max(RAGGED16_COUNTS) > 4        # an empty last row; more blocks than a workgroup has waves
    big = pattern("ACTIVSg10K")
    assert big.block_row_size == 16 and big.num_rows == 20000 and big.num_blocks > 16000


@pytest.mark.parametrize("name", PATTERNS)
def test_bsr_transpose_is_the_transposed_matrix(name):
    a = pattern(name)
    t, perm = ops.bsr_transpose(a)
    assert (t.num_rows, t.num_cols, t.block_row_size, t.block_col_size) == (a.num_cols, a.num_rows, a.block_col_size, a.block_row_size)
    assert t.num_blocks == a.num_blocks and t.nnz == a.nnz
    assert perm.dtype == np.uint32 and np.array_equal(np.sort(perm), np.arange(a.num_blocks))          # a permutation
    assert np.array_equal(t.data, np.asarray(a.data)[perm.astype(np.int64)].transpose(0, 2, 1))        # block t = block perm[t], swapped
    if name != "ACTIVSg10K":
        assert np.array_equal(t.to_dense(), a.to_dense().T)
    rows, cols, blocks = _canonical(a)
    order = np.argsort(cols * (a.num_rows // a.block_row_size) + rows)                                 # A's blocks in A^T's coordinate order
    t_rows, t_cols, t_blocks = _canonical(t)
    assert np.array_equal(t_rows, cols[order]) and np.array_equal(t_cols, rows[order])
    assert np.array_equal(t_blocks, blocks[order].transpose(0, 2, 1))
    # a block row of A^T lists ascending source block rows: the sort is stable
    ptrs = t.block_row_ptrs.astype(np.int64)
    src = t.block_col_idxs.astype(np.int64)
    same_row = np.ones(src.shape[0] - 1, bool)                                                         # is block i + 1 in block i's row?
    starts = ptrs[1:-1]
    same_row[starts[(starts > 0) & (starts < src.shape[0])] - 1] = False
    assert np.all(np.diff(src)[same_row] > 0)
    assert np.array_equal(block_rows(a)[perm.astype(np.int64)], src)


@pytest.mark.parametrize("name", PATTERNS)
def test_bsr_transpose_twice_restores_the_matrix(name):
    a = pattern(name)
    t, _ = ops.bsr_transpose(a)
    back, _ = ops.bsr_transpose(t)
    assert (back.num_rows, back.num_cols) == (a.num_rows, a.num_cols)
    assert np.array_equal(back.block_row_ptrs, a.block_row_ptrs)
    for got, want in zip(_canonical(back), _canonical(a)):
        assert np.array_equal(got, want)
    if name == "ACTIVSg10K":    # its block rows ascend in column, so the storage order itself comes back
        assert np.array_equal(back.block_col_idxs, a.block_col_idxs) and np.array_equal(back.data, a.data)


def test_sddmm_bsr_validates_before_any_device_work():
    l = capi.lib()
    call = l.mispmm_sddmm_bsr_bf16
    one = ctypes.c_void_p(16)   # never dereferenced: every call below must return from validation
    #           stream Mb  K  bS nb rowPtrs colIdxs X  ldx  Y  ldy  N  out  out_bf16
    assert call(None, 4, 64, 16, 1, None, one, one, 8, one, 8, 8, one, 0) == capi.ERR_INVALID_ARG
    assert call(None, 4, 64, 16, 1, one, None, one, 8, one, 8, 8, one, 0) == capi.ERR_INVALID_ARG
    assert call(None, 4, 64, 16, 1, one, one, None, 8, one, 8, 8, one, 1) == capi.ERR_INVALID_ARG
    assert call(None, 4, 64, 16, 1, one, one, one, 8, None, 8, 8, one, 0) == capi.ERR_INVALID_ARG
    assert call(None, 4, 64, 16, 1, one, one, one, 8, one, 8, 8, None, 1) == capi.ERR_INVALID_ARG
    assert b"null" in l.mispmm_last_error()
    assert call(None, 4, 64, 16, 1, one, one, one, 7, one, 8, 8, one, 0) == capi.ERR_INVALID_ARG        # ldx < N
    assert call(None, 4, 64, 32, 1, one, one, one, 8, one, 7, 8, one, 1) == capi.ERR_INVALID_ARG        # ldy < N
    assert b"leading dimension" in l.mispmm_last_error()
    assert call(None, 4, 72, 16, 1, one, one, one, 8, one, 8, 8, one, 0) == capi.ERR_INVALID_ARG        # K % bS
    assert call(None, 4, 80, 32, 1, one, one, one, 8, one, 8, 8, one, 0) == capi.ERR_INVALID_ARG
    assert b"multiple of the block size" in l.mispmm_last_error()
    for bs in (0, 1, 8, 17, 48, 64):
        assert call(None, 4, 64 * 3, bs, 1, one, one, one, 8, one, 8, 8, one, 0) == capi.ERR_UNSUPPORTED
        assert b"16x16 or 32x32" in l.mispmm_last_error()
    big = (1 << 31) // (64 * 2)                                                                          # 64 rows * ld * 2 bytes = 2 GiB
    assert call(None, 4, 64, 16, 1, one, one, one, 8, one, big, 8, one, 0) == capi.ERR_UNSUPPORTED       # Y
    assert call(None, 4, 64, 16, 1, one, one, one, big, one, 8, 8, one, 1) == capi.ERR_UNSUPPORTED       # X: 4 block rows of 16
    assert call(None, 2, 64, 32, 1, one, one, one, big, one, 8, 8, one, 1) == capi.ERR_UNSUPPORTED       # X: 2 block rows of 32
    assert b"2 GiB" in l.mispmm_last_error()
    assert call(None, 0xFFFFFFFF, 64, 32, 1, one, one, one, 0xFFFFFFFF, one, 8, 8, one, 0) == capi.ERR_UNSUPPORTED   # no 64-bit wrap
    assert call(None, 4, 64, 16, 0, one, None, one, 8, one, 8, 8, None, 0) == capi.OK                    # numBlocks == 0: a no-op
    assert call(None, 0, 64, 16, 0, None, None, None, 8, None, 8, 8, None, 1) == capi.OK                 # numBlockRows == 0


def test_python_layer_without_a_gpu():
    torch = pytest.importorskip("torch")
    from mispmm import autograd                      # imports without a GPU
    bsr = pattern("ragged16")
    a = ops.DeviceBSR.from_host(bsr, device="cpu")
    x, y = torch.zeros((bsr.num_rows, 8), dtype=torch.int16), torch.zeros((bsr.num_cols, 8), dtype=torch.int16)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.sddmm_bsr_bf16(a, x, y)
    t = autograd.TrainableBSR.from_host(bsr, device="cpu")
    assert t.perm.dtype == torch.int64 and t.blocks.dtype == torch.bfloat16 and tuple(t.blocks.shape) == (bsr.num_blocks, 16, 16)
    assert (t.tpattern.num_rows, t.tpattern.num_cols, t.tpattern.num_blocks) == (bsr.num_cols, bsr.num_rows, bsr.num_blocks)
    assert np.array_equal(t.blocks.float().numpy(), bsr.data)               # small integers: bf16 numbers already
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.spmm_bsr(t, t.blocks, torch.zeros((bsr.num_cols, 8), dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        autograd.TrainableBSR.from_host(formats.BSR(8, 8, 16, 4, 4, np.array([0, 1, 1], np.uint32), np.array([0], np.uint32),
                                                    np.zeros((1, 4, 4), np.float32)), device="cpu")
