"""No malformed sparse structure gets in, by any of the ways in; every valid one keeps getting in (the validity contract of
include/mispmm.h, corpus in tests/_ingest_cases.py).

The four routes: the `cuspmm` command line on the sequential engine, the formats.read_* functions, ops.*.from_host onto the
host ("cpu") device, and the library's mispmm_*_check_host.  Everything here runs on the host: malformed input never goes
near a device -- that the refusal also covers the device path is shown by where the check sits (a reader's constructor ends
with it, every copy2Device() and every from_host begins with it), not by trying.

Where a route does not exist for a case the test says so by construction, never by a skip: the command line reads no
row-major ELL pair; a defect of the text alone (a token that is no number, a malformed dense.in) has no container to hand
to from_host or to the checker."""
import os
import re
import subprocess

import numpy as np
import pytest

import _ingest_cases as ic
from mispmm import capi, formats, ops

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-optimization-for-spmm_amd")
CLI = os.path.join(PKG, "cuspmm")

MALFORMED, UNUSUAL = ic.malformed(), ic.unusual()
IN_MEMORY = [c for c in MALFORMED if c.mem is not None]
ON_THE_COMMAND_LINE = [c for c in MALFORMED if c.cli]


def test_the_corpus_is_what_the_contract_lists():
    names = {c.name for c in MALFORMED}
    assert len(names) == len(MALFORMED) == 26 and len({c.name for c in UNUSUAL}) == len(UNUSUAL) == 25
    # every case goes through the readers; all but the text-only defects through from_host and the checker; all but the
    # row-major ELL pairs through the command line
    assert sorted(c.name for c in MALFORMED if c.mem is None) == ["csr-token-is-no-number", "dense-header-is-not-two-numbers",
                                                                  "dense-short-row", "dense-token-is-no-number"]
    assert sorted(c.name for c in MALFORMED if not c.cli) == ["ell-rowmajor-column-0xFFFFFFFE", "ell-rowmajor-column-equals-K"]
    assert all(c.mem is not None for c in UNUSUAL)


def run_cli(case, directory, *more):
    return subprocess.run([CLI, ic.CLI_FLAG[case.fmt], "--cpu-only", "-d", str(directory), *more], capture_output=True, text=True, timeout=120)


def uploads(case):
    """Every from_host that takes the case's container: (name, call)."""
    m = case.mem
    if case.fmt == "csr":
        return [("DeviceCSR", lambda **kw: ops.DeviceCSR.from_host(m, device="cpu", **kw)),
                ("DeviceCSR f64", lambda **kw: ops.DeviceCSR.from_host(m, device="cpu", dtype=torch.float64, **kw)),
                ("DeviceCSRTiles", lambda **kw: ops.DeviceCSRTiles.from_host(m, device="cpu", **kw)),
                ("DeviceCSRPanels", lambda **kw: ops.DeviceCSRPanels.from_host(m, device="cpu", **kw))]
    if case.fmt == "coo":
        return [("DeviceCOO", lambda **kw: ops.DeviceCOO.from_host(m, device="cpu", **kw))]
    if case.fmt in ("ell_cm", "ell_rm"):
        return [("DeviceELL", lambda **kw: ops.DeviceELL.from_host(m, device="cpu", **kw)),
                ("DeviceELL f64", lambda **kw: ops.DeviceELL.from_host(m, device="cpu", dtype=torch.float64, **kw))]
    return [("DeviceBSR", lambda **kw: ops.DeviceBSR.from_host(m, device="cpu", **kw)),
            ("bsr_nonzeros", lambda **kw: ops.bsr_nonzeros(m, device="cpu", **kw)),
            ("bsr_nonzeros f64", lambda **kw: ops.bsr_nonzeros(m, device="cpu", dtype=torch.float64, **kw)),
            ("DeviceBSRC", lambda **kw: ops.DeviceBSRC.from_host(m, device="cpu", **kw)),
            ("DeviceBSRCSlots", lambda **kw: ops.DeviceBSRCSlots.from_host(m, device="cpu", **kw))]


def c_verdict(case):
    """(status, mispmm_last_error()) of the library's checker on the case's container."""
    try:
        ops.check_host(case.mem)
    except capi.MispmmError as e:
        return e.status, capi.lib().mispmm_last_error().decode()
    return capi.OK, ""


def numpy_verdict(case):
    try:
        ic.NUMPY_CHECK[case.fmt](case.mem)
    except ValueError as e:
        return capi.ERR_INVALID_ARG, str(e)
    return capi.OK, ""


# ------------------------------------------------------------------------------------------------------------ malformed
@pytest.mark.parametrize("case", ON_THE_COMMAND_LINE, ids=repr)
def test_malformed_the_command_line_refuses(case, tmp_path):
    p = run_cli(case, case.write(tmp_path))
    print(p.returncode, p.stderr)
    assert p.returncode > 0, f"killed by signal {-p.returncode}"
    assert p.returncode == 1 and case.want in p.stderr and p.stderr.startswith("Error: ") and "{" not in p.stdout


@pytest.mark.parametrize("case", MALFORMED, ids=repr)
def test_malformed_the_reader_refuses(case, tmp_path):
    with pytest.raises(ValueError, match=re.escape(case.want)):
        ic.read(case, case.write(tmp_path))


@pytest.mark.parametrize("case", IN_MEMORY, ids=repr)
def test_malformed_every_upload_refuses(case):
    for name, upload in uploads(case):
        with pytest.raises(capi.MispmmError, match=re.escape(case.want_mem)) as e:
            upload()
        assert e.value.status == capi.ERR_INVALID_ARG, name


@pytest.mark.parametrize("case", IN_MEMORY, ids=repr)
def test_malformed_the_checker_names_the_defect(case):
    status, detail = c_verdict(case)
    assert status == capi.ERR_INVALID_ARG and case.want_mem in detail, detail


def test_an_index_array_that_is_no_uint32_is_never_wrapped():
    """A container built by hand with signed indices: the upload range-checks before it narrows."""
    bad = formats.CSR(ic.M, ic.K, np.array(ic.PTRS, np.int64), np.array(ic._with(ic.COLS, 4, -1), np.int64), ic.f32(ic.VALS))
    with pytest.raises(ValueError, match=re.escape("colIdxs[4] = -1 is not an index")):
        ops.DeviceCSR.from_host(bad, device="cpu")
    with pytest.raises(ValueError, match=re.escape("colIdxs[4] = -1 is not an index")):
        formats.check_csr(bad)
    good = formats.CSR(ic.M, ic.K, np.array(ic.PTRS, np.int64), np.array(ic.COLS, np.int32), ic.f32(ic.VALS))
    assert ops.DeviceCSR.from_host(good, device="cpu").nnz == ic.NNZ


def test_a_header_beyond_the_file_allocates_nothing(tmp_path):
    """`4294967295 4 3`: 16 GiB of row pointers if believed.  Refused from the file's size, under an address-space limit
    that an allocation of that size could not pass."""
    d = tmp_path / "huge"
    d.mkdir()
    (d / "a.csr").write_text("4294967295 4 3\n0 1 2 3 3\n0 1 2\n1 2 3\n")
    (d / "a.bsr").write_text("8 8 16 2 2 4294967295\n0 1 2 3 4\n0 1 2 3\n1 2 3 4\n")
    (d / "dense.in").write_text("4294967295 4294967295\n1 2\n")
    for flag in ("--csr", "--bsr"):
        p = subprocess.run(f"ulimit -v 12000000; exec '{CLI}' {flag} --cpu-only -d '{d}'", shell=True, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "header promises" in p.stderr, (flag, p.returncode, p.stderr)
    (d / "a.csr").write_text("4 4 3\n0 1 2 3 3\n0 1 2\n1 2 3\n")
    p = subprocess.run(f"ulimit -v 12000000; exec '{CLI}' --csr --cpu-only -d '{d}'", shell=True, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "header promises" in p.stderr and "dense" in p.stderr, p.stderr
    with pytest.raises(ValueError, match="header promises"):
        formats.read_dense(str(d / "dense.in"))


# ------------------------------------------------------------------------------------------------------------ both lists
@pytest.mark.parametrize("case", IN_MEMORY + UNUSUAL, ids=repr)
def test_the_checker_and_the_numpy_check_agree(case):
    """Same verdict, and the same words for it: two statements of one contract."""
    assert c_verdict(case) == numpy_verdict(case)
    assert (c_verdict(case)[0] == capi.OK) == (case in UNUSUAL)


# ------------------------------------------------------------------------------------------------------------ valid but unusual
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", UNUSUAL, ids=repr)
def test_unusual_the_reader_returns_the_arrays(case, tmp_path):
    got, want = ic.read(case, case.write(tmp_path)), case.mem
    assert type(got) is type(want)
    for field in ("num_rows", "num_cols"):
        assert getattr(got, field) == getattr(want, field)
    for field in ("row_ptrs", "col_idxs", "row_idxs", "block_row_ptrs", "block_col_idxs", "data"):
        if hasattr(want, field):
            # NaN payloads do not survive text: compare the values' bits where they are numbers
            g, w = np.asarray(getattr(got, field)), np.asarray(getattr(want, field))
            assert g.shape == w.shape and g.dtype == w.dtype and (field != "data" or np.array_equal(np.isnan(g), np.isnan(w)))
            assert _same(np.nan_to_num(g, nan=0.0) if field == "data" else g, np.nan_to_num(w, nan=0.0) if field == "data" else w), field


@pytest.mark.parametrize("case", UNUSUAL, ids=repr)
def test_unusual_every_upload_and_the_checker_accept(case):
    assert c_verdict(case) == (capi.OK, "")
    for name, upload in uploads(case):
        try:
            checked = upload()
        except (ValueError, capi.MispmmError) as e:
            # what a builder declines for reasons of its own (rows of one width for the LDS tiles, ascending columns for the
            # panels, 16-row blocks for the bf16 tiles) it must decline the same way with the check switched off
            with pytest.raises(type(e), match=re.escape(str(e))):
                upload(check=False)
            assert name in ("DeviceCSRTiles", "DeviceCSRPanels", "DeviceBSRC", "DeviceBSRCSlots"), (name, e)
            continue
        unchecked = upload(check=False)
        for field, value in vars(checked).items():
            if isinstance(value, torch.Tensor):
                assert _same(value.numpy(), getattr(unchecked, field).numpy()), (name, field)


@pytest.mark.parametrize("case", [c for c in UNUSUAL if c.cli], ids=repr)
def test_unusual_the_command_line_computes_the_oracles_product(case, tmp_path, oracle):
    out = tmp_path / "c.txt"
    p = run_cli(case, case.write(tmp_path / "d"), "--save", str(out))
    assert p.returncode == 0, p.stderr
    assert '"correct":"1"' in p.stdout
    want = ic.oracle_product(oracle, case, case.b)
    got = np.loadtxt(out, skiprows=1, ndmin=2).reshape(want.shape)
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6, equal_nan=True)     # as tests/test_cli.py compares; a NaN must be a NaN


# ------------------------------------------------------------------------------------------------------------ sanitizers
@pytest.mark.skipif(torch.cuda.is_available(), reason="sanitizer builds run on machines without a GPU only")
def test_the_way_in_under_address_and_ub_sanitizers(tmp_path):
    """make ingest_san: the C++ host layer and the library's host-only units with -fsanitize=address,undefined in one
    stand-alone executable, over the whole corpus: every malformed case refused, every valid one accepted and taken through
    toDense(), the sequential engine and the `_host` builders, and no sanitizer report."""
    for case in MALFORMED:
        case.write(tmp_path / "malformed" / case.name)
    for case in UNUSUAL:
        case.write(tmp_path / "valid" / case.name)
    b = subprocess.run(["make", "-s", "-j", "8", "-C", PKG, "ingest_san"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([os.path.join(PKG, "ingest_san"), str(tmp_path / "malformed"), str(tmp_path / "valid")], capture_output=True, text=True,
                       timeout=300, env=env)
    print(p.stdout[-6000:], p.stderr[-6000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert f"ingest_san: {len(MALFORMED)} malformed cases, {len(UNUSUAL)} valid cases, 0 wrong verdicts" in p.stdout
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr
    for case in MALFORMED:
        assert case.want in p.stdout, case.name
