"""fp64 without a GPU: `cuspmm --cpu-only --dtype fp64` against the numpy restatement of the contract (tests/_ref64.py), the
fp64 host helpers against their fp32 twins, argument validation of the new entry points, and _ref64 itself on rows derived
by hand."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from _ref64 import (assert_same_bits64, bsr_rows, coo_rows, ell_colmajor_rows, random_f64, ref_rows,
                    ref_rows_accumulate)
from mispmm import capi, datasets, formats, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-optimization-for-spmm_amd", "cuspmm")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run_cli(*args, check=True):
    p = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)
    if check:
        assert p.returncode == 0, p.stderr
    return p


def _records(stdout):
    import re
    return [dict(re.findall(r'"([A-Za-z]+)":"([^"]*)"', body)) for body in re.findall(r"\{(.*?)\},", stdout, flags=re.S)]


def _full_precision_dir(tmp_path, seed=7):
    """A copy of small_32x32_generated (Hamrle1's structure) holding ONE .bsr, its values and dense.in replaced by random
    full-mantissa doubles, written with repr() (round-trips every double)."""
    d = tmp_path / "f64"
    shutil.copytree(os.path.join(GOLDEN, "small_32x32_generated"), d)
    for extra in ("Hamrle1_b2.bsr", "Hamrle1_b4.bsr", "result.expect"):
        (d / extra).unlink()
    rng = np.random.default_rng(seed)
    csr = formats.read_csr(str(d / "Hamrle1.csr"), dtype=np.float64)
    csr = formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, random_f64(rng, csr.nnz))
    formats.write_csr(d / "Hamrle1.csr", csr)
    formats.write_coo(d / "Hamrle1.coo", formats.csr_to_coo(csr))
    formats.write_bsr(d / "Hamrle1.bsr", formats.csr_to_bsr(csr, 4))
    formats.write_ell_colmajor(d / "Hamrle1_rowind.ell", d / "Hamrle1_values_colmajor.ell", formats.csr_to_ell_colmajor(csr))
    b = random_f64(rng, (csr.num_cols, 12))
    formats.write_dense(d / "dense.in", b)
    return d, csr, b


def _want(fmt, d, b):
    """The contract's bits for the file of `fmt` in d, in that format's own order of addition."""
    if fmt == "CSR":
        a = formats.read_csr(str(d / "Hamrle1.csr"), dtype=np.float64)
        return ref_rows(a.row_ptrs, a.col_idxs, a.data, b)
    if fmt == "COO":
        a = formats.read_coo(str(d / "Hamrle1.coo"), dtype=np.float64)
        return ref_rows(*coo_rows(a.num_rows, a.row_idxs, a.col_idxs, a.data), b)
    if fmt == "ELL":
        a = formats.read_ell_colmajor(str(d / "Hamrle1_rowind.ell"), str(d / "Hamrle1_values_colmajor.ell"), dtype=np.float64)
        return ref_rows(*ell_colmajor_rows(a.num_rows, a.num_cols, a.max_col_nnz, a.row_idxs, a.data), b)
    a = formats.read_bsr(str(d / "Hamrle1.bsr"), dtype=np.float64)
    # the CPU engine multiplies the explicit zeros too; with a finite B they add +-0 to a sum that is never -0: same bits
    return ref_rows(*bsr_rows(a.num_rows, a.block_row_size, a.block_col_size, a.block_row_ptrs, a.block_col_idxs, a.data,
                              skip_zeros=False), b)


FLAGS = (("--csr", "CSR"), ("--coo", "COO"), ("--ell", "ELL"), ("--bsr", "BSR"))


@pytest.mark.parametrize("synthetic", [False, True])
def test_cli_cpu_only_fp64_is_the_contract_bitwise(tmp_path, synthetic):
    d, csr, b = _full_precision_dir(tmp_path)
    extra = []
    if synthetic:
        extra = ["-k", "8"]
        b = synth.dense_b(csr.num_cols, 8).astype(np.float64)
    # the products of full-mantissa doubles round: a result computed in fp32 anywhere would be off in its low bits
    assert not np.array_equal(ref_rows(csr.row_ptrs, csr.col_idxs, csr.data, b),
                              ref_rows(csr.row_ptrs, csr.col_idxs, csr.data.astype(np.float32).astype(np.float64), b))
    for flag, fmt in FLAGS:
        out = tmp_path / f"{fmt}.txt"
        p = run_cli(flag, "--cpu-only", "--dtype", "fp64", "-d", str(d), "--save", str(out), *extra)
        recs = _records(p.stdout)
        assert len(recs) == 1 and recs[0]["format"] == fmt and recs[0]["kernelType"] == "0" and recs[0]["correct"] == "1"
        assert recs[0]["dtype"] == "fp64"
        got = np.loadtxt(out, skiprows=1, ndmin=2, dtype=np.float64)
        assert_same_bits64(got, _want(fmt, d, b), f"{fmt} --cpu-only --dtype fp64")


def test_cli_all_formats_in_one_fp64_run_carry_the_dtype(tmp_path):
    d, _, _ = _full_precision_dir(tmp_path)
    p = run_cli("--csr", "--coo", "--ell", "--bsr", "--cpu-only", "--dtype", "fp64", "-d", str(d))
    recs = _records(p.stdout)
    assert [r["format"] for r in recs] == ["COO", "CSR", "BSR", "ELL"]
    assert all(r["dtype"] == "fp64" for r in recs)
    # an fp32 run of the same files prints no dtype (records unchanged)
    assert all("dtype" not in r for r in _records(run_cli("--csr", "--coo", "--cpu-only", "-d", str(d)).stdout))


def test_cli_fp64_refusals(tmp_path):
    g = os.path.join(GOLDEN, "small_32x32_generated")
    p = run_cli("--csr", "--cpu-only", "--dtype", "fp8", "-d", g, check=False)
    assert p.returncode != 0 and "--dtype" in p.stderr
    for extra in (["--gpus", "2"], ["--batch", "3"]):
        p = run_cli("--csr", "--cpu-only", "--dtype", "fp64", "-d", g, *extra, check=False)
        assert p.returncode != 0 and "fp64" in p.stderr


def _ell_rows_f32(ell):
    """The fp32 helpers' route to the same list: colmajor_to_rowmajor + ell_compact."""
    rm = ops.colmajor_ell_to_rowmajor(ell)
    cols = np.ascontiguousarray(rm.col_idxs, dtype=np.uint32).reshape(-1)
    vals = np.ascontiguousarray(rm.data, dtype=np.float32).reshape(-1)
    nnz = ctypes.c_uint32(0)
    head = (rm.num_rows, rm.width, cols.ctypes.data, vals.ctypes.data, ctypes.byref(nnz))
    l = capi.lib()
    capi.check(l.mispmm_ell_compact_host(*head, None, None, None))
    rp = np.zeros(rm.num_rows + 1, np.uint32)
    ci, va = np.zeros(max(nnz.value, 1), np.uint32), np.zeros(max(nnz.value, 1), np.float32)
    capi.check(l.mispmm_ell_compact_host(*head, rp.ctypes.data, ci.ctypes.data, va.ctypes.data))
    return rp, ci[:nnz.value]


def _host_matrices():
    return [(n, datasets.load_csr(n, dtype=np.float64)) for n in ("GL7d25", "Hamrle1", "n3c5-b6")]


@pytest.mark.parametrize("name,csr", _host_matrices(), ids=lambda x: x if isinstance(x, str) else "")
def test_f64_ell_helper_matches_the_fp32_route_and_keeps_values(name, csr):
    rng = np.random.default_rng(3)
    csr = formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, random_f64(rng, csr.nnz))
    ell = formats.csr_to_ell_colmajor(csr)
    rp, ci, va = ops.ell_rows_f64(ell)
    rp32, ci32 = _ell_rows_f32(ell)
    assert np.array_equal(rp, rp32) and np.array_equal(ci, ci32)
    wrp, wci, wva = ell_colmajor_rows(ell.num_rows, ell.num_cols, ell.max_col_nnz, ell.row_idxs, ell.data)
    assert np.array_equal(rp, wrp) and np.array_equal(ci, wci)
    assert np.array_equal(va.view(np.uint64), wva.view(np.uint64))     # the inputs, bit for bit


@pytest.mark.parametrize("name,csr", _host_matrices(), ids=lambda x: x if isinstance(x, str) else "")
@pytest.mark.parametrize("block", [2, 4])
def test_f64_bsr_helper_matches_the_fp32_helper_and_keeps_values(name, csr, block):
    rng = np.random.default_rng(5)
    m = (csr.num_rows + block - 1) // block * block
    k = (csr.num_cols + block - 1) // block * block
    rp_in = np.concatenate([csr.row_ptrs, np.full(m - csr.num_rows, csr.row_ptrs[-1], np.uint32)])
    csr = formats.CSR(m, k, rp_in, csr.col_idxs, random_f64(rng, csr.nnz))
    bsr = formats.csr_to_bsr(csr, block)
    rp, ci, va = ops.bsr_nonzeros_f64_host(bsr)
    l = capi.lib()
    nnz = ctypes.c_uint32(0)
    ptrs, cols = np.ascontiguousarray(bsr.block_row_ptrs, np.uint32), np.ascontiguousarray(bsr.block_col_idxs, np.uint32)
    data = np.ascontiguousarray(bsr.data, np.float32).reshape(-1)    # the fp32 helper on the same blocks (no value rounds to 0)
    args = (bsr.num_block_rows, block, block, bsr.num_blocks, ptrs.ctypes.data, cols.ctypes.data, data.ctypes.data, ctypes.byref(nnz))
    capi.check(l.mispmm_bsr_nonzeros_host(*args, None, None, None))
    rp32, ci32, va32 = np.empty(m + 1, np.uint32), np.empty(max(nnz.value, 1), np.uint32), np.empty(max(nnz.value, 1), np.float32)
    capi.check(l.mispmm_bsr_nonzeros_host(*args, rp32.ctypes.data, ci32.ctypes.data, va32.ctypes.data))
    assert np.array_equal(rp, rp32) and np.array_equal(ci, ci32[:nnz.value])
    wrp, wci, wva = bsr_rows(bsr.num_rows, block, block, bsr.block_row_ptrs, bsr.block_col_idxs, bsr.data)
    assert np.array_equal(rp, wrp) and np.array_equal(ci, wci)
    assert np.array_equal(va.view(np.uint64), wva.view(np.uint64))


def test_f64_helpers_on_the_golden_ell_and_bsr_fixtures():
    g = os.path.join(GOLDEN, "small_32x32_generated")
    ell = formats.read_ell_colmajor(os.path.join(g, "Hamrle1_rowind.ell"), os.path.join(g, "Hamrle1_values_colmajor.ell"), dtype=np.float64)
    rp, ci, va = ops.ell_rows_f64(ell)
    rp32, ci32 = _ell_rows_f32(ell)
    assert np.array_equal(rp, rp32) and np.array_equal(ci, ci32) and int(rp[-1]) == ell.nnz
    g210 = os.path.join(GOLDEN, "small_210_generated")
    ell = formats.read_ell_colmajor(os.path.join(g210, "n3c5-b6_rowind.ell"), os.path.join(g210, "n3c5-b6_values_colmajor.ell"),
                                    dtype=np.float64)
    rp, ci, va = ops.ell_rows_f64(ell)
    rp32, ci32 = _ell_rows_f32(ell)
    assert np.array_equal(rp, rp32) and np.array_equal(ci, ci32) and int(rp[-1]) == ell.nnz
    for f in (os.path.join(g, "Hamrle1.bsr"), os.path.join(g, "Hamrle1_b2.bsr"), os.path.join(g, "Hamrle1_b4.bsr"),
              os.path.join(g210, "n3c5-b6.bsr"), os.path.join(g210, "n3c5-b6_b2.bsr")):
        bsr = formats.read_bsr(f, dtype=np.float64)
        rp, ci, va = ops.bsr_nonzeros_f64_host(bsr)
        wrp, wci, wva = bsr_rows(bsr.num_rows, bsr.block_row_size, bsr.block_col_size, bsr.block_row_ptrs, bsr.block_col_idxs, bsr.data)
        assert np.array_equal(rp, wrp) and np.array_equal(ci, wci) and np.array_equal(va, wva)


def test_f64_helper_size_queries_and_errors():
    l = capi.lib()
    nnz = ctypes.c_uint32(0)
    assert l.mispmm_ell_colmajor_to_rows_f64_host(2, 2, 1, None, None, None, None, None, None) == capi.ERR_INVALID_ARG
    ri = np.array([1, 5], np.uint32)                      # row 5 of a 2-row matrix
    va = np.array([1.0, 2.0])
    assert l.mispmm_ell_colmajor_to_rows_f64_host(2, 2, 1, ri.ctypes.data, va.ctypes.data, ctypes.byref(nnz), None, None, None) == capi.ERR_INVALID_ARG
    assert l.mispmm_bsr_nonzeros_f64_host(1, 0, 1, 0, None, None, None, ctypes.byref(nnz), None, None, None) == capi.ERR_INVALID_ARG


def test_csr_f64_validates_before_device_work():
    """Every refusal comes back before a device is touched (this machine may have none)."""
    l = capi.lib()
    buf = ctypes.c_void_p(0x1000)                         # never dereferenced: validation fails first
    ok = dict(rp=buf, ci=buf, va=buf, b=buf, c=buf)
    def call(M=4, N=8, ldb=8, ldc=8, acc=0, **kw):
        p = {**ok, **kw}
        return l.mispmm_csr_f64(None, M, 4, 3, p["rp"], p["ci"], p["va"], p["b"], N, ldb, p["c"], ldc, acc)
    assert call(rp=None) == capi.ERR_INVALID_ARG
    assert call(ci=None) == capi.ERR_INVALID_ARG
    assert call(va=None) == capi.ERR_INVALID_ARG
    assert call(b=None) == capi.ERR_INVALID_ARG
    assert call(c=None) == capi.ERR_INVALID_ARG
    assert call(ldb=7) == capi.ERR_INVALID_ARG
    assert call(ldc=7) == capi.ERR_INVALID_ARG
    assert call(acc=2) == capi.ERR_INVALID_ARG
    assert call(acc=-1) == capi.ERR_INVALID_ARG
    assert call(M=0) == capi.OK                           # M == 0: nothing to do
    assert l.mispmm_vendor_spmm_f64(None, 7, 4, 4, 3, 0, buf, buf, buf, buf, 8, 8, buf, 8, None, None, None) == capi.ERR_INVALID_ARG
    assert l.mispmm_vendor_spmm_f64(None, 0, 4, 4, 3, 0, None, buf, buf, buf, 8, 8, buf, 8, None, None, None) == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------ the checker itself, on rows derived by hand
def _one_row(vals, bcol):
    vals = np.asarray(vals, np.float64)
    b = np.asarray(bcol, np.float64).reshape(-1, 1)
    rp, ci = np.array([0, len(vals)]), np.arange(len(vals))
    return ref_rows(rp, ci, vals, b)[0, 0], ref_rows_accumulate(rp, ci, vals, b)[0, 0]


def test_ref64_adds_in_list_order():
    # 2^53 + 1 rounds back to 2^53 (ties to even), then - 2^53 gives +0; 1 + (2^53 - 2^53) would give 1
    for got in _one_row([2.0 ** 53, 1.0, -(2.0 ** 53)], [1.0, 1.0, 1.0]):
        assert got == 0.0 and not np.signbit(got)


def test_ref64_starts_from_plus_zero():
    for got in _one_row([-0.0, -0.0], [1.0, 1.0]):          # -0 + -0 alone would stay -0; +0 + -0 = +0
        assert got == 0.0 and not np.signbit(got)
    for got in _one_row([-1.0], [0.0]):                     # a single -0 product
        assert not np.signbit(got)
    empty = ref_rows(np.array([0, 0]), np.array([], np.int64), np.array([]), np.ones((1, 1)))[0, 0]
    assert empty == 0.0 and not np.signbit(empty)            # an empty row is +0


def test_ref64_keeps_subnormal_products():
    tiny = 2.0 ** -1070
    for got in _one_row([tiny, tiny], [0.5, 0.25]):          # 2^-1071 + 2^-1072: both subnormal, exact
        assert got == 2.0 ** -1071 + 2.0 ** -1072 and 0 < got < np.finfo(np.float64).tiny


def test_ref64_rounds_each_product_once_and_has_no_fma():
    a, b = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30               # a * b = 1 + 2^-29 + 2^-60: the 2^-60 is rounded away
    for got in _one_row([a, -1.0], [b, 1.0 + 2.0 ** -29]):
        assert got == 0.0                                    # an FMA would keep 2^-60


def test_bitwise_comparison_tells_signed_zeros_and_requires_nans():
    with pytest.raises(AssertionError):
        assert_same_bits64(np.array([-0.0]), np.array([0.0]))
    with pytest.raises(AssertionError):
        assert_same_bits64(np.array([1.0]), np.array([np.nan]))
    assert_same_bits64(np.array([np.nan, 1.0]), np.array([-np.nan, 1.0]))
