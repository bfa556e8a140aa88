"""fp64 SpMM on the GPU (mispmm_csr_f64 behind ops and the CLI): REFERENCE bit-exact against the contract's numpy restatement
(tests/_ref64.py) for every format, odd and strided shapes, adversarial values and a B beyond 2 GiB; FAST within its bound;
graph replay; the CLI's fp64 records and the rocSPARSE fp64 cross-check.  Operands carry full 53-bit mantissas."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _ref64 import (abs_scale, assert_same_bits64, bsr_rows, coo_rows, ell_colmajor_rows, random_f64, ref_rows)
from mispmm import capi, datasets, formats, ops

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-optimization-for-spmm_amd", "cuspmm")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SENTINEL = 0x7FF8DEADBEEF0001        # a quiet NaN no arithmetic produces: fills the gaps of strided operands


def _randomised(csr, seed):
    rng = np.random.default_rng(seed)
    return formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, random_f64(rng, csr.nnz))


def _b(k, n, seed, ldb=None):
    """B [k, n] float64 on the device, rows ldb apart (the gap columns hold the NaN sentinel); returns (view, host copy)."""
    host = random_f64(np.random.default_rng(seed), (k, n))
    ldb = ldb or n
    buf = torch.empty((k, ldb), dtype=torch.float64, device="cuda")
    buf.view(torch.int64).fill_(SENTINEL)
    buf[:, :n] = torch.from_numpy(host).cuda()
    return buf[:, :n], host


def _out(m, n, ldc):
    buf = torch.empty((m, ldc), dtype=torch.float64, device="cuda")
    buf.view(torch.int64).fill_(SENTINEL)
    return buf


def _gap_untouched(buf, n):
    gap = buf[:, n:].cpu().numpy().view(np.uint64)
    assert (gap == SENTINEL).all(), "a store landed in the gap between rows"


def _mat(name):
    return _randomised(datasets.load_csr(name, dtype=np.float64), seed=len(name))


def _empty_rows():
    """Ragged rows with many empty ones (first, last and runs in between)."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 12, 700)
    lens[rng.random(700) < 0.4] = 0
    lens[[0, 1, 699]] = 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cols = np.concatenate([np.sort(rng.choice(900, size=int(n), replace=False)) for n in lens]).astype(np.uint32)
    return formats.CSR(700, 900, rp, cols, random_f64(rng, int(rp[-1])))


NS = [1, 2, 3, 8, 63, 64, 128, 200, 512]


def _check_csr(csr, n, seed, ldb_pad=0, ldc_pad=0, acc="reference"):
    b, bh = _b(csr.num_cols, n, seed, n + ldb_pad)
    a = ops.DeviceCSR.from_host(csr, dtype=torch.float64)
    out = _out(csr.num_rows, n, n + ldc_pad)
    got = ops.spmm_csr(a, b, out=out[:, :n], acc=acc)
    torch.cuda.synchronize()
    assert "csr_f64" in capi.last_kernel() or csr.num_rows == 0
    want = ref_rows(csr.row_ptrs, csr.col_idxs, csr.data, bh)
    _gap_untouched(out, n)
    return got.cpu().numpy(), want, bh


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["delaunay_n12", "qh1484", "empty_rows"])
def test_csr_reference_bitwise_over_widths(name, n):
    csr = _empty_rows() if name == "empty_rows" else _mat(name)
    pad = (0, 0) if n % 2 else (3, 1)                     # odd strides: the 8-byte body
    got, want, _ = _check_csr(csr, n, seed=n, ldb_pad=pad[0], ldc_pad=pad[1])
    assert_same_bits64(got, want, f"{name} N={n}")


@pytest.mark.parametrize("name,n", [("n4c6-b13", 64), ("n4c6-b13", 128), ("n4c6-b13", 63), ("GL7d25", 64), ("GL7d25", 200),
                                    ("GL7d25", 512)])
def test_csr_reference_bitwise_uniform_and_long_rows(name, n):
    got, want, _ = _check_csr(_mat(name), n, seed=3)
    assert_same_bits64(got, want, f"{name} N={n}")


def test_empty_matrices():
    for m, k in ((0, 5), (6, 5)):
        csr = formats.CSR(m, k, np.zeros(m + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0))
        a = ops.DeviceCSR.from_host(csr, dtype=torch.float64)
        b = torch.zeros((k, 8), dtype=torch.float64, device="cuda")
        got = ops.spmm_csr(a, b).cpu().numpy()
        assert got.shape == (m, 8)
        assert_same_bits64(got, np.zeros((m, 8)), f"empty {m}x{k}")


@pytest.mark.parametrize("n", [8, 64, 63, 128])
def test_coo_handed_over_unsorted(n):
    csr = _mat("delaunay_n12")
    coo = formats.csr_to_coo(csr)
    perm = np.random.default_rng(1).permutation(coo.nnz)
    coo = formats.COO(coo.num_rows, coo.num_cols, coo.row_idxs[perm], coo.col_idxs[perm], coo.data[perm])
    b, bh = _b(csr.num_cols, n, 5)
    got = ops.spmm_coo(ops.DeviceCOO.from_host(coo, dtype=torch.float64), b).cpu().numpy()
    assert_same_bits64(got, ref_rows(*coo_rows(coo.num_rows, coo.row_idxs, coo.col_idxs, coo.data), bh), f"COO N={n}")


@pytest.mark.parametrize("name", ["qh1484", "GL7d25"])
@pytest.mark.parametrize("n", [3, 64])
def test_ell_from_the_column_major_form(name, n):
    ell = formats.csr_to_ell_colmajor(_mat(name))
    b, bh = _b(ell.num_cols, n, 6)
    got = ops.spmm_ell(ops.DeviceELL.from_host(ell, dtype=torch.float64), b).cpu().numpy()
    want = ref_rows(*ell_colmajor_rows(ell.num_rows, ell.num_cols, ell.max_col_nnz, ell.row_idxs, ell.data), bh)
    assert_same_bits64(got, want, f"ELL {name} N={n}")


@pytest.mark.parametrize("block", [16, 4])
def test_bsr_nonzero_list(block):
    csr = _mat("ACTIVSg10K")
    m = (csr.num_rows + block - 1) // block * block
    k = (csr.num_cols + block - 1) // block * block
    csr = formats.CSR(m, k, np.concatenate([csr.row_ptrs, np.full(m - csr.num_rows, csr.row_ptrs[-1], np.uint32)]), csr.col_idxs, csr.data)
    bsr = formats.csr_to_bsr(csr, block)
    b, bh = _b(k, 64, 7)
    got = ops.spmm_bsr_nonzeros(ops.bsr_nonzeros(bsr, dtype=torch.float64), b).cpu().numpy()
    rp, ci, va = ops.bsr_nonzeros_f64_host(bsr)
    assert_same_bits64(got, ref_rows(rp, ci, va, bh), f"BSR{block} list")


def _adversarial(seed=0):
    """Rows of 1..200 entries whose 2^53 cancellations sit across 8-slot blocks, 64-entry chunks and the wave; signed zeros,
    subnormals, Inf and NaN in A; the arrays continue past nnz with NaN values and a wild column index."""
    rng = np.random.default_rng(seed)
    k = 600
    lens = np.array([3, 9, 10, 17, 64, 65, 66, 130, 200, 1, 0, 8, 16, 33, 127, 129] * 6)
    m = lens.shape[0]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cols = np.concatenate([rng.choice(k - 50, size=int(n), replace=False) for n in lens]).astype(np.uint32)
    vals = random_f64(rng, int(rp[-1]))
    for r in range(m):
        s, e = int(rp[r]), int(rp[r + 1])
        for at in (6, 7, 8, 62, 63, 64, 127, 128):              # the triple (2^53, 1, -2^53) around block/chunk/wave edges
            if s + at + 2 < e:
                vals[s + at:s + at + 3] = [2.0 ** 53, 1.0, -(2.0 ** 53)]
        if e - s > 4 and r % 3 == 0:
            vals[s + 1] = -0.0
        if e - s > 5 and r % 5 == 1:
            vals[s + 2] = 2.0 ** -1070                          # subnormal products
        if e - s > 6 and r % 7 == 2:
            vals[s + 3] = np.inf if r % 2 else -np.inf
        if e - s > 6 and r % 11 == 3:
            vals[s + 4] = np.nan
    return formats.CSR(m, k, rp, cols, vals)


def _adversarial_b(k, n, seed):
    rng = np.random.default_rng(seed)
    b = random_f64(rng, (k, n))
    b[rng.random((k, n)) < 0.02] = -0.0
    b[rng.random((k, n)) < 0.01] = 2.0 ** -1060
    b[5, :] = np.inf
    b[9, n // 2] = -np.inf
    b[13, 0] = np.nan
    b[k - 50:, :] = np.nan                                    # rows no entry references
    return b


@pytest.mark.parametrize("n", [2, 3, 64, 128, 200])
def test_adversarial_values_reference_bitwise_and_fast_bound(n):
    csr = _adversarial()
    nnz = csr.nnz
    bh = _adversarial_b(csr.num_cols, n, n)
    b = torch.from_numpy(bh).cuda()
    # arrays past nnz: NaN values and a wild column index that must never be read
    ci = torch.from_numpy(np.concatenate([csr.col_idxs, [0xFFFFFFF0, 7]]).astype(np.uint32).view(np.int32)).cuda()
    va = torch.from_numpy(np.concatenate([csr.data, [np.nan, np.nan]])).cuda()
    rp = torch.from_numpy(csr.row_ptrs.view(np.int32)).cuda()
    a = ops.DeviceCSR(csr.num_rows, csr.num_cols, nnz, rp, ci, va)
    want = ref_rows(csr.row_ptrs, csr.col_idxs, csr.data, bh)
    ref = ops.spmm_csr(a, b).cpu().numpy()
    assert_same_bits64(ref, want, f"adversarial REFERENCE N={n}")
    fast = ops.spmm_csr(a, b, acc="fast").cpu().numpy()
    assert "fast" in capi.last_kernel()
    assert np.array_equal(np.isnan(fast), np.isnan(want)), "FAST NaN positions differ from REFERENCE"
    assert np.array_equal(np.isinf(fast) & (fast > 0), np.isinf(want) & (want > 0))
    assert np.array_equal(np.isinf(fast) & (fast < 0), np.isinf(want) & (want < 0))
    assert not np.any((fast == 0) & np.signbit(fast)), "FAST returned -0.0"
    fin = np.isfinite(want)
    scale = abs_scale(csr.row_ptrs, csr.col_idxs, csr.data, bh)
    assert np.all(np.abs(fast[fin] - want[fin]) <= 1e-12 * scale[fin])


@pytest.mark.parametrize("n", [64, 63])
def test_b_beyond_2gib_takes_the_64_bit_body(n):
    k = (1 << 31) // (8 * n) + 2                               # K x N doubles: just over 2 GiB
    assert k * n * 8 > 0x7FFFFFFF
    rows = np.array([0, 1, k // 2, k - 1, k - 2, 3])
    rng = np.random.default_rng(2)
    b = torch.empty((k, n), dtype=torch.float64, device="cuda")
    b.view(torch.int64).fill_(SENTINEL)                        # rows no entry references: NaN
    bh_rows = random_f64(rng, (rows.shape[0], n))
    b[torch.from_numpy(rows).cuda()] = torch.from_numpy(bh_rows).cuda()
    lens = [3, 0, 6, 1, 2]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    sel = np.array([0, 2, 3, 1, 5, 4, 0, 3, 2, 4, 1, 5])[: int(rp[-1])]
    csr = formats.CSR(len(lens), k, rp, rows[sel].astype(np.uint32), random_f64(rng, int(rp[-1])))
    got = ops.spmm_csr(ops.DeviceCSR.from_host(csr, dtype=torch.float64), b).cpu().numpy()
    assert ",wide" in capi.last_kernel(), capi.last_kernel()
    del b
    torch.cuda.empty_cache()
    # the reference over the referenced rows only (a compacted B with remapped columns: same values, same order)
    want = ref_rows(csr.row_ptrs, sel[: int(rp[-1])], csr.data, bh_rows)
    assert_same_bits64(got, want, f"B over 2 GiB N={n}")


def test_graph_replay_equals_eager_bitwise():
    csr = _mat("delaunay_n12")
    a = ops.DeviceCSR.from_host(csr, dtype=torch.float64)
    b, _ = _b(csr.num_cols, 64, 9)
    eager = ops.spmm_csr(a, b).clone()
    out = torch.empty_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.spmm_csr(a, b, out=out)                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.spmm_csr(a, b, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert_same_bits64(out.cpu().numpy(), eager.cpu().numpy(), "graph replay")


def test_mixed_precision_operands_are_refused():
    csr = _mat("qh1484")
    a64 = ops.DeviceCSR.from_host(csr, dtype=torch.float64)
    a32 = ops.DeviceCSR.from_host(formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, csr.data.astype(np.float32)))
    b64 = torch.zeros((csr.num_cols, 8), dtype=torch.float64, device="cuda")
    b32 = torch.zeros((csr.num_cols, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        ops.spmm_csr(a64, b32)
    with pytest.raises(ValueError):
        ops.spmm_csr(a32, b64)
    with pytest.raises(ValueError):
        ops.spmm_csr(a64, b64, out=torch.empty((csr.num_rows, 8), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        ops.spmm_csr(a64, b64, kernel=5)
    coo = ops.DeviceCOO.from_host(formats.csr_to_coo(csr), dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.spmm_coo(coo, b32)


@pytest.mark.parametrize("fmt", ["CSR", "COO"])
def test_vendor_fp64_agrees_within_the_fast_bound(fmt):
    csr = _mat("delaunay_n12")
    b, bh = _b(csr.num_cols, 64, 4)
    c = torch.zeros((csr.num_rows, 64), dtype=torch.float64, device="cuda")
    if fmt == "CSR":
        a = ops.DeviceCSR.from_host(csr, dtype=torch.float64)
        args = (0, csr.num_rows, csr.num_cols, csr.nnz, 0, ops._p(a.row_ptrs), ops._p(a.col_idxs), ops._p(a.data))
    else:
        a = ops.DeviceCOO.from_host(formats.csr_to_coo(csr), dtype=torch.float64)
        args = (1, csr.num_rows, csr.num_cols, csr.nnz, 0, ops._p(a.row_idxs), ops._p(a.col_idxs), ops._p(a.data))
    p, k, e = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    capi.check(capi.lib().mispmm_vendor_spmm_f64(None, *args, ops._p(b), 64, 64, ops._p(c), 64, ctypes.byref(p), ctypes.byref(k),
                                                 ctypes.byref(e)))
    torch.cuda.synchronize()
    want = ref_rows(csr.row_ptrs, csr.col_idxs, csr.data, bh)
    scale = abs_scale(csr.row_ptrs, csr.col_idxs, csr.data, bh)
    assert np.all(np.abs(c.cpu().numpy() - want) <= 1e-12 * scale)


@pytest.mark.parametrize("n", [2, 64, 128, 200])
def test_strided_and_8_byte_aligned_operands(n):
    """Even strides keep the 16-byte body (and its gap columns untouched); views that start one double into their buffers
    are 8-byte but not 16-byte aligned and take the 8-byte body."""
    csr = _mat("qh1484")
    a = ops.DeviceCSR.from_host(csr, dtype=torch.float64)
    want_for = {}
    for ldb, ldc, offset, body in ((n + 2, n + 4, 0, "V2"), (n + 2, n + 2, 1, "V1")):
        host = random_f64(np.random.default_rng(n), (csr.num_cols, n))
        bbuf = torch.empty((csr.num_cols, ldb), dtype=torch.float64, device="cuda")
        bbuf.view(torch.int64).fill_(SENTINEL)
        b = bbuf[:, offset:offset + n]
        b.copy_(torch.from_numpy(host).cuda())
        cbuf = _out(csr.num_rows, n, ldc)
        out = cbuf[:, offset:offset + n]
        ops.spmm_csr(a, b, out=out)
        torch.cuda.synchronize()
        assert f"V{body[1]}" in capi.last_kernel(), capi.last_kernel()
        got = cbuf.cpu().numpy()
        want = want_for.setdefault(offset, ref_rows(csr.row_ptrs, csr.col_idxs, csr.data, host))
        assert_same_bits64(got[:, offset:offset + n], want, f"N={n} ldb={ldb} ldc={ldc} offset={offset}")
        gap = np.delete(got.view(np.uint64), np.s_[offset:offset + n], axis=1)
        assert (gap == SENTINEL).all(), "a store landed outside the view"


def test_batched_entry_point_refuses_a_float64_a():
    csr = _mat("qh1484")
    a = ops.DeviceCSR.from_host(csr, dtype=torch.float64)
    b = torch.zeros((csr.num_cols, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        ops.spmm_csr_batch(a, [b, b])


def _records(stdout):
    return [dict(re.findall(r'"([A-Za-z]+)":"([^"]*)"', body)) for body in re.findall(r"\{(.*?)\},", stdout, flags=re.S)]


def test_cli_fp64_records_and_saved_results(tmp_path):
    d = tmp_path / "f64"
    shutil.copytree(os.path.join(GOLDEN, "small_210_generated"), d)
    for extra in ("n3c5-b6_b2.bsr", "result.expect"):
        (d / extra).unlink()
    rng = np.random.default_rng(21)
    csr = formats.read_csr(str(d / "n3c5-b6.csr"), dtype=np.float64)
    csr = formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, random_f64(rng, csr.nnz))
    formats.write_csr(d / "n3c5-b6.csr", csr)
    formats.write_coo(d / "n3c5-b6.coo", formats.csr_to_coo(csr))
    formats.write_bsr(d / "n3c5-b6.bsr", formats.csr_to_bsr(csr, 2))
    ell = formats.csr_to_ell_colmajor(csr)
    formats.write_ell_colmajor(d / "n3c5-b6_rowind.ell", d / "n3c5-b6_values_colmajor.ell", ell)
    bh = random_f64(rng, (csr.num_cols, 24))
    formats.write_dense(d / "dense.in", bh)
    bsr = formats.read_bsr(str(d / "n3c5-b6.bsr"), dtype=np.float64)
    coo = formats.read_coo(str(d / "n3c5-b6.coo"), dtype=np.float64)
    wants = {"CSR": ref_rows(csr.row_ptrs, csr.col_idxs, csr.data, bh),
             "COO": ref_rows(*coo_rows(coo.num_rows, coo.row_idxs, coo.col_idxs, coo.data), bh),
             "ELL": ref_rows(*ell_colmajor_rows(ell.num_rows, ell.num_cols, ell.max_col_nnz, ell.row_idxs, ell.data), bh),
             "BSR": ref_rows(*bsr_rows(bsr.num_rows, 2, 2, bsr.block_row_ptrs, bsr.block_col_idxs, bsr.data), bh)}
    for flag, fmt, kernels in (("--csr", "CSR", ["0", "1", "-1"]), ("--coo", "COO", ["0", "1", "-1"]), ("--ell", "ELL", ["0", "1"]),
                               ("--bsr", "BSR", ["0", "3"])):
        out = tmp_path / f"{fmt}.txt"
        p = subprocess.run([CLI, flag, "--dtype", "fp64", "--iters", "50", "-d", str(d), "--save", str(out)], capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr
        recs = _records(p.stdout)
        assert [r["kernelType"] for r in recs] == kernels, p.stdout
        assert all(r["correct"] == "1" and r["dtype"] == "fp64" for r in recs)
        assert all("csr_f64" in r["kernel"] for r in recs if r["kernelType"] not in ("0", "-1"))
        assert_same_bits64(np.loadtxt(out, skiprows=1, ndmin=2, dtype=np.float64), wants[fmt], f"CLI {fmt}")


F64_RATIO_BOUND = 1.27  # measured 1.157 and 1.171 (4.16 us against 3.55 us) + ~10 % (profiles/fp64/README.md)


@pytest.mark.perf
def test_fp64_n64_against_fp32_n128_on_the_headline():
    """Same B bytes per entry (512) and the same C bytes: fp64 REFERENCE at N = 64 against fp32 REFERENCE at N = 128 on
    n4c6-b13, graph replays of 200 launches after warm-up (profiles/fp64/README.md has the measurement)."""
    csr = datasets.load_csr("n4c6-b13", dtype=np.float64)
    a64 = ops.DeviceCSR.from_host(_randomised(csr, 1), dtype=torch.float64)
    a32 = ops.DeviceCSR.from_host(formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, csr.data.astype(np.float32)))
    b64 = torch.rand((csr.num_cols, 64), dtype=torch.float64, device="cuda")
    b32 = torch.rand((csr.num_cols, 128), dtype=torch.float32, device="cuda")
    c64 = torch.empty((csr.num_rows, 64), dtype=torch.float64, device="cuda")
    c32 = torch.empty((csr.num_rows, 128), dtype=torch.float32, device="cuda")

    def per_launch(fn, launches=200, reps=5):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(launches):
                fn()
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3 / launches)
        return best

    t64 = per_launch(lambda: ops.spmm_csr(a64, b64, out=c64))
    t32 = per_launch(lambda: ops.spmm_csr(a32, b32, out=c32))
    print(f"fp64 N=64 {t64:.3f} us, fp32 N=128 {t32:.3f} us, ratio {t64 / t32:.3f}")
    assert t64 <= F64_RATIO_BOUND * t32, f"fp64 N=64 {t64:.2f} us against fp32 N=128 {t32:.2f} us"
