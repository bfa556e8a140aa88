"""The structure check every upload now runs must not change what valid input computes: the valid-but-unusual corpus of
tests/_ingest_cases.py (unsorted and repeated columns, explicit zeros, NaN and Inf, empty rows and block rows, all-padding
ELL lines, no entries at all, one row, one column) through from_host with the check on and each format's default entry
point in REFERENCE mode, bit for bit against the oracle.  Valid input only: nothing malformed is referenced here."""
import os
import re
import subprocess

import numpy as np
import pytest

import _bits
import _ingest_cases as ic
import _spmm_bf16_ref as bf
from mispmm import ops

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-optimization-for-spmm_amd", "cuspmm")
UNUSUAL = ic.unusual()
WIDTHS = (5, 64)          # one column group with a ragged end; whole 16-byte vectors of B and C


def _upload(case):
    from_host = {"csr": ops.DeviceCSR.from_host, "coo": ops.DeviceCOO.from_host, "ell_cm": ops.DeviceELL.from_host,
                 "ell_rm": ops.DeviceELL.from_host, "bsr": ops.DeviceBSR.from_host}[case.fmt]
    return from_host(case.mem, check=True)


@pytest.mark.parametrize("case", UNUSUAL, ids=repr)
def test_checked_upload_then_the_default_entry_point_gives_the_oracles_bits(case, oracle):
    product = {"csr": ops.spmm_csr, "coo": ops.spmm_coo, "ell_cm": ops.spmm_ell, "ell_rm": ops.spmm_ell, "bsr": ops.spmm_bsr}[case.fmt]
    a = _upload(case)
    for n in WIDTHS:
        b = ic.dense_b(case.mem.num_cols, n)
        got = product(a, torch.from_numpy(b).cuda(), acc="reference")
        _bits.assert_same_bits(got, ic.oracle_product(oracle, case, b), f"{case.name} N={n}")


@pytest.mark.parametrize("case", [c for c in UNUSUAL if c.fmt == "csr"], ids=repr)
def test_checked_upload_then_the_bf16_row_product_gives_the_oracles_bits(case):
    a = ops.DeviceCSR.from_host(case.mem, plan=False, check=True)
    for n in WIDTHS:
        bits = bf.bf16_bits(ic.dense_b(case.mem.num_cols, n))
        got = ops.spmm_csr_bf16(a, torch.from_numpy(bits.view(np.int16)).cuda(), acc="reference", ref_sum="f64")
        want = bf.expected("ref64", case.mem.row_ptrs, case.mem.col_idxs, case.mem.data, bits)
        _bits.assert_same_bits(got, want, f"{case.name} N={n}")


@pytest.mark.parametrize("csr,coo", [("csr-repeated-pairs", "coo-reverse-order"), ("csr-unsorted-columns", "coo-repeated-pairs-and-zeros")])
def test_cli_full_engine_flow_on_unusual_files(tmp_path, csr, coo):
    """`cuspmm --csr --coo` on a directory of such files: every kernel's record and the vendor check say correct."""
    by_name = {c.name: c for c in UNUSUAL}
    by_name[csr].write(tmp_path)
    by_name[coo].write(tmp_path)        # both 6 x 7: one dense.in serves the two
    p = subprocess.run([CLI, "--csr", "--coo", "-d", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    correct = re.findall(r'"format":"(\w+)",\s*"kernelType":"(-?\d+)".*?"correct":"(\d)"', p.stdout, flags=re.S)
    assert {f for f, _, _ in correct} == {"CSR", "COO"} and len(correct) >= 12
    assert all(c == "1" for _, _, c in correct), correct
