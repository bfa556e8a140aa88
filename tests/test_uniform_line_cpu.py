"""CPU half of tests/test_gpu_uniform_line.py: what its operands (tests/_uniform_line_cases.py) promise, shown with the oracle
alone, and the host-side rule that keeps a launch away from the straight-line body."""
import ctypes
import os

import numpy as np
import pytest

from mispmm import capi, formats

import _adversarial as adv
import _fma_chain as fc
import _uniform_line_cases as cases
from _bits import assert_same_bits


def test_generators_give_uniform_rows_over_the_whole_column_range():
    for width in cases.WIDTHS:
        for m in cases.ROW_COUNTS:
            csr = cases.uniform_csr(m, 40, width, 100 * width + m)
            assert csr.num_rows == m and np.array_equal(csr.row_ptrs, np.arange(m + 1, dtype=np.uint32) * width)
            cols = csr.col_idxs.reshape(m, width).astype(np.int64)
            assert np.all(np.diff(cols, axis=1) > 0) or m == 1 or width == 40     # ascending, distinct
            assert cols.min() == 0 and cols.max() == 39
        small = cases.uniform_csr(9, width, width, 300 + width)                   # K as small as the row: every B row, every row
        assert np.array_equal(small.col_idxs.reshape(9, width), np.tile(np.arange(width, dtype=np.uint32), (9, 1)))
    big = cases.uniform_csr(33, cases.BIG_K, 14, 414)
    assert big.col_idxs.min() == 0 and big.col_idxs.max() == cases.BIG_K - 1 and cases.BIG_K * 256 > (4 << 20)


@pytest.mark.parametrize("width", [10, 14])
def test_padded_ell_has_every_real_length(width):
    csr = cases.padded_ell_csr(width, 500 + width)
    lens = np.diff(csr.row_ptrs.astype(np.int64))
    assert set(lens.tolist()) == set(range(width + 1)) and lens[0] == 0 and lens[-1] == 0
    ellc = formats.csr_to_ell_colmajor(csr)
    rp, _, _ = fc.ell_colmajor_rows(ellc)
    assert np.array_equal(np.diff(rp.astype(np.int64)), lens)


@pytest.mark.parametrize("width", cases.WIDTHS)
def test_fast_corpus_is_sharp(oracle, width):
    """On the FAST operands an unfused chain and a reversed chain each differ from the contract's chain in their bits."""
    csr = cases.uniform_csr(9, 40, width, 600 + width)
    assert fc.corpus_is_sharp(fc.csr_rows(csr), cases.dense_b(40, 128))


def test_adversarial_rows_have_their_closed_forms(oracle):
    """The oracle alone reproduces what the construction promises, and the same rows summed in fp32 would not."""
    csr, b, expect = cases.adversarial(128)
    assert csr.num_rows == 19 and np.isnan(b[0]).all() and not np.any(csr.col_idxs == 0)
    ref = oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b)
    assert sorted(expect) == list(range(13))
    for r, want in expect.items():
        assert_same_bits(ref[r], want, f"adversarial row {r}")
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[13:]).all()
    narrow = fc.chain_unfused(csr.row_ptrs, csr.col_idxs, csr.data, b)           # fp32 product, fp32 sum
    full = np.abs(adv.pattern_row(128)) == 1                                     # 3e38 + 3e38 overflows fp32 where |pattern| is 1
    assert np.isinf(narrow[0][full]).all() and np.all(narrow[2] == 0) and np.all(narrow[4] == 0)
    assert not np.signbit(ref[11]).any() and not np.signbit(ref[12]).any()


def test_fallback_rule_keeps_large_arrays_on_the_rolling_body():
    """row_line_fits: both arrays of A and all of C below 2 GiB (32-bit buffer offsets whose bit 31 marks a dropped access)."""
    tune = os.path.join(os.path.dirname(capi.LIB_PATH), "libmispmm_tune.so")
    assert os.path.exists(tune), "run `make -C cuda-optimization-for-spmm_amd tune`"
    lib = ctypes.CDLL(tune)
    fits = lib.mispmm_debug_row_line_fits
    fits.argtypes = [ctypes.c_uint32] * 3
    fits.restype = ctypes.c_int
    assert fits(25605, 14, 128) == 1 and fits(1, 9, 4) == 1
    m = (1 << 29) // 14                                        # M * 14 * 4 just below 2^31
    assert m * 14 * 4 <= 0x7FFFFFFF and fits(m, 14, 1) == 1
    assert fits(m + 1, 14, 1) == 0                             # nnz * 4 past the offset range
    assert fits((1 << 28), 9, 1) == 0                          # far past it (the product does not wrap)
    assert fits(1 << 20, 9, 512) == 0 and fits((1 << 20) - 1, 9, 512) == 1       # C of 2 GiB / just below
