"""The panel kernel's host side on a machine WITHOUT a GPU: the offsets mispmm_csr_panels_host builds (what the kernel walks
without searching), what it declines, and the `--panels` flag of the CLI.  No compute call is made here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, datasets, formats

import _adversarial as adv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-optimization-for-spmm_amd", "cuspmm")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def random_csr(m, k, density, seed):
    """Bernoulli(density) positions, columns ascending in every row."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, k)) < density
    r, c = np.nonzero(mask)
    ptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.uint32)
    return formats.CSR(m, k, ptr, c.astype(np.uint32), rng.uniform(-2, 2, r.shape[0]).astype(np.float32))


def build(csr, depth, row_ptrs=None, col_idxs=None):
    """(status of the size query, numPanels, numOffsets, status of the fill, panelPtrs as [M, numPanels + 1])"""
    l = capi.lib()
    rp = np.ascontiguousarray(csr.row_ptrs if row_ptrs is None else row_ptrs, dtype=np.uint32)
    ci = np.ascontiguousarray(csr.col_idxs if col_idxs is None else col_idxs, dtype=np.uint32)
    npan, noff = ctypes.c_uint32(0), ctypes.c_uint64(0)
    head = (csr.num_rows, csr.num_cols, rp.ctypes.data, ci.ctypes.data if ci.size else None, depth, ctypes.byref(npan), ctypes.byref(noff))
    st = l.mispmm_csr_panels_host(*head, None, 0)
    if st != capi.OK:
        return st, 0, 0, None, None
    asked = (npan.value, noff.value)
    pp = np.full(max(noff.value, 1) + 3, 0xDEADBEEF, np.uint32)                     # three guard words behind the offsets
    st2 = l.mispmm_csr_panels_host(*head, pp.ctypes.data, noff.value if noff.value else 1)
    assert (npan.value, noff.value) == asked, "the size query and the fill disagree"
    assert np.all(pp[max(noff.value, 1):] == 0xDEADBEEF), "the fill wrote past the offsets it announced"
    return st, npan.value, noff.value, st2, pp[:noff.value].reshape(csr.num_rows, npan.value + 1)


def check_invariants(csr, depth):
    st, npan, noff, st2, pp = build(csr, depth)
    assert st == capi.OK and st2 == capi.OK, capi.lib().mispmm_last_error()
    assert npan == -(-csr.num_cols // depth) and noff == csr.num_rows * (npan + 1)
    rp = csr.row_ptrs.astype(np.int64)
    p64 = pp.astype(np.int64)
    assert np.all(np.diff(p64, axis=1) >= 0), "a row's offsets decrease"
    assert np.array_equal(p64[:, 0], rp[:-1]) and np.array_equal(p64[:, -1], rp[1:]), "offsets do not span the row"
    # every entry between offsets p and p + 1 has its column in [p depth, (p + 1) depth)
    panel_of_entry = np.zeros(csr.nnz, np.int64)
    for r in range(csr.num_rows):
        panel_of_entry[rp[r]:rp[r + 1]] = np.repeat(np.arange(npan), np.diff(p64[r]))
    assert np.array_equal(csr.col_idxs.astype(np.int64) // depth, panel_of_entry), "an entry sits in the wrong panel"
    return pp


@pytest.mark.parametrize("depth", [64, 128])
@pytest.mark.parametrize("which", ["random_0.1", "random_0.5", "n4c6-b13"])
def test_builder_invariants(which, depth):
    csr = datasets.load_csr(which) if which == "n4c6-b13" else random_csr(700, 1000, float(which.split("_")[1]), 5)
    check_invariants(csr, depth)


def test_default_depth_is_the_header_constant():
    text = open(os.path.join(ROOT, "include", "mispmm.h")).read()
    assert int(re.search(r"#define MISPMM_PANEL_ROWS (\d+)u", text).group(1)) == capi.lib().mispmm_csr_panel_rows() == 128


def test_builder_degenerate_shapes():
    depth = capi.lib().mispmm_csr_panel_rows()
    empty = formats.CSR(0, 40, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32))      # M = 0
    st, npan, noff, st2, _ = build(empty, depth)
    assert (st, npan, noff, st2) == (capi.OK, 1, 0, capi.OK)
    hollow = formats.CSR(37, 300, np.zeros(38, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32))  # all rows empty
    assert np.all(check_invariants(hollow, depth) == 0)
    small = random_csr(50, depth - 29, 0.3, 6)                                                              # K < P: one panel
    pp = check_invariants(small, depth)
    assert pp.shape == (50, 2)
    check_invariants(random_csr(33, 257, 0.4, 7), depth)                                                    # K = 2 P + 1: a one-row panel


def test_builder_declines():
    l = capi.lib()
    depth = l.mispmm_csr_panel_rows()
    csr = random_csr(40, 300, 0.2, 8)
    rp = csr.row_ptrs.astype(np.int64)
    r = int(np.argmax(np.diff(rp) >= 2))
    swapped = csr.col_idxs.copy()
    swapped[rp[r]], swapped[rp[r] + 1] = csr.col_idxs[rp[r] + 1], csr.col_idxs[rp[r]]
    assert build(csr, depth, col_idxs=swapped)[0] == capi.ERR_UNSUPPORTED
    assert b"ascend" in l.mispmm_last_error()
    repeated = csr.col_idxs.copy()
    repeated[rp[r] + 1] = repeated[rp[r]]                                                # a repeated column does not ascend either
    assert build(csr, depth, col_idxs=repeated)[0] == capi.ERR_UNSUPPORTED
    for case in adv.corpus():                                                            # the corpus' unsorted rows
        if "unsorted" in case.tags:
            assert build(case.csr, depth)[0] == capi.ERR_UNSUPPORTED
    too_big = csr.col_idxs.copy()
    too_big[-1] = csr.num_cols
    assert build(csr, depth, col_idxs=too_big)[0] == capi.ERR_INVALID_ARG
    falling = csr.row_ptrs.copy()
    falling[5] = falling[6] + 1                                                          # row 5 ends before it starts
    assert build(csr, depth, row_ptrs=falling)[0] == capi.ERR_INVALID_ARG
    assert build(csr, 0)[0] == capi.ERR_INVALID_ARG
    # outputs half-given: the array without its capacity, the capacity without the array, a capacity too small
    rp32, ci32 = np.ascontiguousarray(csr.row_ptrs, np.uint32), np.ascontiguousarray(csr.col_idxs, np.uint32)
    npan, noff = ctypes.c_uint32(0), ctypes.c_uint64(0)
    head = (csr.num_rows, csr.num_cols, rp32.ctypes.data, ci32.ctypes.data, depth, ctypes.byref(npan), ctypes.byref(noff))
    buf = np.zeros(csr.num_rows * 8, np.uint32)
    assert l.mispmm_csr_panels_host(*head, buf.ctypes.data, 0) == capi.ERR_INVALID_ARG
    assert l.mispmm_csr_panels_host(*head, None, buf.shape[0]) == capi.ERR_INVALID_ARG
    assert l.mispmm_csr_panels_host(*head, buf.ctypes.data, 7) == capi.ERR_INVALID_ARG
    assert not buf.any(), "a refused fill wrote offsets"
    assert l.mispmm_csr_panels_host(*head[:5], None, ctypes.byref(noff), None, 0) == capi.ERR_INVALID_ARG


def test_entry_point_validates_before_any_device_work():
    l = capi.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: every call below must end in validation
    assert l.mispmm_csr_panel_f32(None, 4, 4, 1, one, one, one, one, 128, one, 8, 8, one, 8, 7) == capi.ERR_INVALID_ARG
    assert l.mispmm_csr_panel_f32(None, 4, 4, 1, one, one, one, None, 128, one, 8, 8, one, 8, 0) == capi.ERR_INVALID_ARG
    assert l.mispmm_csr_panel_f32(None, 4, 4, 1, one, one, one, one, 128, one, 8, 4, one, 8, 0) == capi.ERR_INVALID_ARG   # ldb < N
    assert l.mispmm_csr_panel_f32(None, 4, 4, 1, one, one, one, one, 100, one, 8, 8, one, 8, 0) == capi.ERR_UNSUPPORTED   # depth
    assert l.mispmm_csr_panel_f32(None, 4, 4, 1, one, one, one, one, 128, one, 6, 8, one, 8, 0) == capi.ERR_UNSUPPORTED   # N % 4
    assert l.mispmm_csr_panel_f32(None, 4, 4, 1, one, one, one, one, 128, ctypes.c_void_p(20), 8, 8, one, 8, 0) == capi.ERR_UNSUPPORTED
    assert l.mispmm_csr_panel_f32(None, 0, 4, 0, None, None, None, None, 128, None, 8, 8, None, 8, 0) == capi.OK          # empty: no-op


# ---------------------------------------------------------------------------------------------------- the CLI flag
def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def test_cli_help_lists_panels():
    p = run_cli("--help")
    assert p.returncode == 0 and "--panels" in p.stdout


def test_cli_rejects_panels_with_fp64_or_gpus():
    d = os.path.join(GOLDEN, "small_32x32")
    for extra in (("--dtype", "fp64"), ("--gpus", "2")):
        p = run_cli("--csr", "--cpu-only", "--panels", *extra, "-d", d)
        assert p.returncode != 0 and "--panels is the fp32 single-GPU panel kernel" in p.stderr and p.stdout == ""


def test_cli_rejects_panels_without_csr():
    p = run_cli("--coo", "--cpu-only", "--panels", "-d", os.path.join(GOLDEN, "small_32x32"))
    assert p.returncode != 0 and "--panels" in p.stderr and "needs --csr" in p.stderr and p.stdout == ""


def test_sweep_tool_parses_and_prints_the_panel_record():
    """tools/sparsity_sweep.py: a record whose kernel tag holds commas, brackets and spaces is parsed whole, the panel record
    is printed (opening with `panels`, ending with its tag) and the other lines keep their form."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sparsity_sweep
    tag = "csr_panel<ref,P128,R64,lds-dma> xcd 1x8, 16 panels"
    out = ('{\n"testcase":"t",\n"sparsity":"0.5",\n"format":"CSR",\n"kernelType":"5",\n"correct":"1",\n"cudaKernelTimeMs":"0.250000",\n'
           '"steadyIters":"200",\n"steadyKernelUs":"298.800000",\n"gflops":"14400.000000",\n"kernel":"row_gather<G16,V4,ref64,csr,B128,U16,roll,S32> xcd 1x8"\n},\n'
           '{\n"testcase":"t",\n"sparsity":"0.5",\n"format":"CSR",\n"kernelType":"7",\n"correct":"1",\n"cudaKernelTimeMs":"0.500000",\n'
           '"steadyIters":"200",\n"steadyKernelUs":"123.400000",\n"gflops":"34800.000000",\n"kernel":"' + tag + '"\n},\n'
           '{\n"testcase":"t",\n"format":"CSR",\n"kernelType":"-1",\n"correct":"0",\n"cudaKernelTimeMs":"3.000000"\n},\n')
    recs = sparsity_sweep.parse_records(out)
    assert [r["kernelType"] for r in recs] == ["5", "7", "-1"]
    assert recs[1]["kernel"] == tag and recs[0]["kernel"].endswith("xcd 1x8") and recs[1]["gflops"] == "34800.000000"
    lines = [sparsity_sweep.format_line("0.5", r) for r in recs]
    assert lines[0].startswith("density 0.5 CSR kernel  5 correct 1 ") and "298.8 us" in lines[0] and "row_gather" not in lines[0]
    assert lines[1].startswith("panels density 0.5 CSR kernel  7 correct 1 ") and "123.4 us" in lines[1] and lines[1].endswith(tag)
    assert lines[2].startswith("density 0.5 CSR kernel -1 correct 0 ")


def test_cli_cpu_only_records_do_not_change_with_panels():
    d = os.path.join(GOLDEN, "small_32x32")
    strip = lambda s: re.sub(r'"(sequentialTimeMs|cuda[A-Za-z]*TimeMs)":"[^"]*"', "", s)    # wall-clock figures
    plain, with_flag = run_cli("--csr", "--cpu-only", "-d", d), run_cli("--csr", "--cpu-only", "--panels", "-d", d)
    assert plain.returncode == 0 and with_flag.returncode == 0, with_flag.stderr
    assert plain.stdout.count('"kernelType"') >= 1
    assert strip(plain.stdout) == strip(with_flag.stdout)
