"""The panel-tiled CSR kernel (mispmm_csr_panel_f32: B staged in LDS panel by panel, for dense-regime matrices) against the
CPU oracle -- never against itself or another HIP kernel.  REFERENCE mode must give the oracle's bits (tests/_bits.py), FAST
mode the usual bound on sum |a||b|; strided operands keep their gap columns; what the entry point does not take is declined
with the library's error and nothing is launched."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mispmm import capi, datasets, formats, ops, synth  # noqa: E402

import _adversarial as adv  # noqa: E402
from _bits import assert_gap_untouched, assert_same_bits, sentinel_buffer  # noqa: E402
from _ref64 import abs_scale  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-optimization-for-spmm_amd", "cuspmm")
FAST_RTOL = 1e-5                       # the FAST bar of tests/test_gpu_spmm.py: |c - ref| <= 1e-5 * sum |a||b|
GAP = 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs a GPU"
    assert os.path.exists(capi.LIB_PATH), "libmispmm.so must be built (no fallback path exists)"
    capi.lib()


def random_csr(m, k, density, seed, lo=-2.0, hi=2.0):
    """Bernoulli(density) positions, columns ascending in every row."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, k)) < density
    r, c = np.nonzero(mask)
    ptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.uint32)
    return formats.CSR(m, k, ptr, c.astype(np.uint32), rng.uniform(lo, hi, r.shape[0]).astype(np.float32))


def assert_fast_close(c, ref, scale, what=""):
    err = np.abs(c.astype(np.float64) - ref.astype(np.float64))
    bound = FAST_RTOL * scale + 1e-37
    assert np.all(err <= bound), f"{what}: max err/bound {np.max(err / bound):.3g}"


def check_both_modes(oracle, csr, b, what, fast=True):
    """REFERENCE bit for bit, FAST within its bound; both into strided C buffers whose gap columns must survive."""
    ref = oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b)
    a = ops.DeviceCSRPanels.from_host(csr)
    bd = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    n = b.shape[1]
    buf = sentinel_buffer(csr.num_rows, n, n + GAP, torch)
    got = ops.spmm_csr_panels(a, bd, out=buf[:, :n])
    assert "csr_panel<ref" in capi.last_kernel(), capi.last_kernel()
    assert_same_bits(got, ref, what)
    assert_gap_untouched(buf, n, what)
    if fast:
        got = ops.spmm_csr_panels(a, bd, acc="fast").cpu().numpy()
        assert "csr_panel<fast" in capi.last_kernel(), capi.last_kernel()
        assert_fast_close(got, ref, abs_scale(csr.row_ptrs, csr.col_idxs, csr.data, b), what + " fast")


@pytest.mark.parametrize("n", [64, 128, 200, 1024])
@pytest.mark.parametrize("density", [0.02, 0.1, 0.5, 0.9])
def test_random_matrices_match_oracle(oracle, density, n):
    """700 x 1000: no multiple of the 64-row block, the 64-column part or the panel depth."""
    csr = random_csr(700, 1000, density, 100 + int(density * 100))
    check_both_modes(oracle, csr, synth.dense_b(1000, n), f"density {density} N {n}")


def ascends(csr):
    """Every row's columns ascend strictly (what the panel builder takes)."""
    step = np.diff(csr.col_idxs.astype(np.int64))
    inside = np.ones(max(csr.nnz - 1, 0), bool)
    inside[csr.row_ptrs[1:-1][(csr.row_ptrs[1:-1] > 0) & (csr.row_ptrs[1:-1] < csr.nnz)].astype(np.int64) - 1] = False   # row boundaries
    return bool(np.all(step[inside] > 0))


ASCENDING = [c for c in adv.corpus() if ascends(c.csr)]
DECLINED = [c for c in adv.corpus() if not ascends(c.csr)]     # rows in another order: test_declines


def test_the_corpus_has_both_kinds():
    assert len(ASCENDING) >= 8 and {"order", "signed_zero", "width", "poisoned_nan", "poisoned_inf"} <= {c.name for c in ASCENDING}
    assert DECLINED and "storage_order" in {c.name for c in DECLINED}


@pytest.mark.parametrize("case", ASCENDING, ids=[c.name for c in ASCENDING])
def test_adversarial_cases_match_oracle_bits(oracle, case):
    """Values chosen so that a changed order of addition, a narrower sum, a sum started from -0 or a padding slot that read
    real B data changes bits; B sits in a buffer with NaN gap columns, the A arrays of the poisoned cases have NaN tails."""
    ref = oracle.spmm_csr(case.csr.row_ptrs, case.csr.col_idxs, case.csr.data, case.b)
    a = ops.DeviceCSRPanels.from_host(case.csr)
    if case.poison is not None:
        for name, fill in (("col_idxs", int(case.poison_cols[0])), ("data", float("nan"))):
            t = getattr(a, name)
            longer = torch.empty(t.numel() + 37, dtype=t.dtype, device=t.device)
            longer[t.numel():] = fill
            longer[:t.numel()].copy_(t)
            setattr(a, name, longer[:t.numel()])
    k, n = case.b.shape
    bbuf = torch.full((k, n + GAP), float("nan"), dtype=torch.float32, device="cuda")
    bbuf[:, :n] = torch.from_numpy(np.ascontiguousarray(case.b)).cuda()
    cbuf = sentinel_buffer(case.csr.num_rows, n, n + GAP, torch)
    got = ops.spmm_csr_panels(a, bbuf[:, :n], out=cbuf[:, :n])
    assert_same_bits(got, ref, case.name)
    assert_gap_untouched(cbuf, n, case.name)


def sorted_rows(csr):
    """The same entries with every row's columns ascending (a different matrix as far as the order of addition goes)."""
    rp = csr.row_ptrs.astype(np.int64)
    row_of = np.repeat(np.arange(csr.num_rows), np.diff(rp))
    perm = np.lexsort((csr.col_idxs, row_of))
    return formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs[perm], csr.data[perm])


@pytest.mark.parametrize("make", [adv.subnormal, adv.nonfinite], ids=["subnormal", "nonfinite"])
def test_sorted_variants_of_the_declined_cases(oracle, make):
    """The corpus' subnormal and non-finite cases keep some rows in another order (declined: test_declines); with their rows
    sorted they go through -- subnormal products and sums, Inf - Inf, NaN, a stored zero meeting an Inf row of B."""
    case = make()
    csr = sorted_rows(case.csr)
    assert ascends(csr)
    ref = oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, case.b)
    assert np.isnan(ref).any() or make is adv.subnormal
    got = ops.spmm_csr_panels(ops.DeviceCSRPanels.from_host(csr), torch.from_numpy(case.b).cuda())
    assert_same_bits(got, ref, case.name + " (rows sorted)")


def test_empty_rows_one_row_and_short_k(oracle):
    depth = capi.lib().mispmm_csr_panel_rows()
    rng = np.random.default_rng(3)
    holes = random_csr(150, 400, 0.3, 31)
    lens = np.diff(holes.row_ptrs.astype(np.int64))
    lens[rng.choice(150, 60, replace=False)] = 0                      # 60 empty rows, among them (forced) the first and last
    lens[[0, 149]] = 0
    keep = np.concatenate([np.arange(s, s + l) for s, l in zip(holes.row_ptrs[:-1].astype(np.int64), lens)] + [np.zeros(0, np.int64)])
    holes = formats.CSR(150, 400, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), holes.col_idxs[keep], holes.data[keep])
    check_both_modes(oracle, holes, synth.dense_b(400, 64), "empty rows")
    nothing = formats.CSR(70, 300, np.zeros(71, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    check_both_modes(oracle, nothing, synth.dense_b(300, 64), "no entries at all")
    check_both_modes(oracle, random_csr(1, 900, 0.6, 32), synth.dense_b(900, 128), "one row")
    check_both_modes(oracle, random_csr(130, depth - 29, 0.5, 33), synth.dense_b(depth - 29, 64), "K < P")
    check_both_modes(oracle, random_csr(65, 2 * depth + 1, 0.5, 34), synth.dense_b(2 * depth + 1, 72), "a one-row last panel")


def test_sparse_matrix_outside_the_sweet_spot(oracle):
    csr = datasets.load_csr("n4c6-b13")
    check_both_modes(oracle, csr, synth.dense_b(csr.num_cols, 128), "n4c6-b13 x 128")


def test_full_sweep_shape_reference_bits(oracle):
    """2048 x 2048 at density 0.5 times 2048 x 1024, values in (-100, 100) as the sweep's generator draws them."""
    csr = random_csr(2048, 2048, 0.5, 35, -100.0, 100.0)
    b = np.random.default_rng(36).uniform(-100, 100, (2048, 1024)).astype(np.float32)
    check_both_modes(oracle, csr, b, "sweep shape", fast=False)


def test_other_panel_depth(oracle):
    """Offsets built for 64-row panels go through the 64-row kernel."""
    csr = random_csr(300, 500, 0.4, 37)
    b = synth.dense_b(500, 128)
    a = ops.DeviceCSRPanels.from_host(csr, panel_rows=64)
    got = ops.spmm_csr_panels(a, torch.from_numpy(b).cuda())
    assert "P64" in capi.last_kernel()
    assert_same_bits(got, oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b), "P = 64")


@pytest.mark.parametrize("n", [64, 200])
def test_strided_operands(oracle, n):
    """b and out as column slices (at a 16-byte-aligned column) of wider buffers."""
    csr = random_csr(333, 777, 0.3, 38)
    b = synth.dense_b(777, n)
    ref = oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b)
    a = ops.DeviceCSRPanels.from_host(csr)
    bw = torch.full((777, n + 12), float("nan"), dtype=torch.float32, device="cuda")
    bw[:, 8:8 + n] = torch.from_numpy(b).cuda()
    cw = sentinel_buffer(333, 0, n + 24, torch)
    for acc in ("reference", "fast"):
        cw.view(torch.int32).fill_(0x7FC0DEAD)
        got = ops.spmm_csr_panels(a, bw[:, 8:8 + n], out=cw[:, 4:4 + n], acc=acc)
        assert got.data_ptr() == cw[:, 4:4 + n].data_ptr()
        if acc == "reference":
            assert_same_bits(got, ref, f"strided N {n}")
        else:
            assert_fast_close(got.cpu().numpy(), ref, abs_scale(csr.row_ptrs, csr.col_idxs, csr.data, b), f"strided fast N {n}")
        assert_gap_untouched(cw[:, :4], 0, "columns before the view")
        assert_gap_untouched(cw[:, 4 + n:], 0, "columns behind the view")


def test_declines(oracle):
    csr = random_csr(90, 300, 0.2, 39)
    rp = csr.row_ptrs.astype(np.int64)
    r = int(np.argmax(np.diff(rp) >= 2))
    cols = csr.col_idxs.copy()
    cols[rp[r]], cols[rp[r] + 1] = cols[rp[r] + 1], cols[rp[r]]
    with pytest.raises(capi.MispmmError) as e:                                 # a row that does not ascend: at from_host
        ops.DeviceCSRPanels.from_host(formats.CSR(90, 300, csr.row_ptrs, cols, csr.data))
    assert e.value.status == capi.ERR_UNSUPPORTED
    for case in DECLINED:
        with pytest.raises(capi.MispmmError) as e:
            ops.DeviceCSRPanels.from_host(case.csr)
        assert e.value.status == capi.ERR_UNSUPPORTED, case.name
    a = ops.DeviceCSRPanels.from_host(csr)
    good = ops.spmm_csr_panels(a, torch.from_numpy(synth.dense_b(300, 64)).cuda())
    assert "csr_panel" in capi.last_kernel()
    tag = capi.last_kernel()

    def declined(b, out, status=capi.ERR_UNSUPPORTED):
        before = out.clone()
        ops.spmm_csr(ops.DeviceCSR.from_host(csr), torch.zeros((300, 8), device="cuda"))   # another kernel's tag in between
        other = capi.last_kernel()
        with pytest.raises(capi.MispmmError) as err:
            ops.spmm_csr_panels(a, b, out=out)
        assert err.value.status == status
        torch.cuda.synchronize()
        assert capi.last_kernel() == other and "csr_panel" not in other, "a declined call launched"
        assert torch.equal(out.view(torch.int32), before.view(torch.int32)), "a declined call wrote C"

    wide = torch.zeros((300, 72), device="cuda")
    cw = sentinel_buffer(90, 0, 72, torch)
    declined(wide[:, :62], cw[:, :62])                                   # N not a multiple of 4
    declined(wide[:, 1:65], cw[:, :64])                                  # B 4 bytes off a 16-byte boundary
    declined(wide[:, :64], cw[:, 2:66])                                  # C 8 bytes off
    odd = torch.zeros((300, 70), device="cuda")
    declined(odd[:, :64], cw[:, :64])                                    # ldb not a multiple of 4
    with pytest.raises(ValueError):
        ops.spmm_csr_panels(a, torch.zeros((300, 64)))                   # a CPU tensor: there is no CPU path
    assert tag.startswith("csr_panel<ref,") and good.shape == (90, 64)


# ---------------------------------------------------------------------------------------------------- the CLI flag
def records(stdout):
    return [dict(re.findall(r'"([A-Za-z]+)":"([^"]*)"', body)) for body in re.findall(r"\{\n(.*?)\n\},", stdout, flags=re.S)]


def test_cli_panels_adds_exactly_one_record(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_sparse
    path = gen_sparse.generate(str(tmp_path), rows=256, cols=256, k=128, densities=(0.5,))[0]
    base = ["--csr", "--iters", "20", "-d", path]
    plain = subprocess.run([CLI, *base], capture_output=True, text=True, timeout=600)
    flagged = subprocess.run([CLI, *base, "--panels"], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and flagged.returncode == 0, flagged.stderr
    rp, rf = records(plain.stdout), records(flagged.stdout)
    # without the flag: the parent commit's record set (sequential engine, kernels 1..6, the vendor cross-check)
    assert [r["kernelType"] for r in rp] == ["0", "1", "2", "3", "4", "5", "6", "-1"]
    seven = [r for r in rf if r["kernelType"] == "7"]
    assert len(seven) == 1 and [r["kernelType"] for r in rf if r["kernelType"] != "7"] == [r["kernelType"] for r in rp]
    rec = seven[0]
    assert rec["correct"] == "1" and rec["format"] == "CSR" and rec["kernel"].startswith("csr_panel<ref,"), rec
    assert int(rec["steadyIters"]) == 20 and float(rec["steadyKernelUs"]) > 0 and float(rec["gflops"]) > 0
    for a, b in zip(rp, [r for r in rf if r["kernelType"] != "7"]):        # the numbered kernels launch what they launched
        assert a.get("kernel") == b.get("kernel") and a["correct"] == b["correct"]


def test_cli_declined_matrix_adds_no_record(tmp_path):
    case = adv.storage_order()
    d = tmp_path / "unsorted"
    d.mkdir()
    formats.write_csr(str(d / "matrix.csr"), case.csr)
    p = subprocess.run([CLI, "--csr", "--no-vendor", "-k", "64", "--panels", "-d", str(d)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert "--panels" in p.stderr and "declined" in p.stderr and p.stderr.count("\n") == 1
    assert [r["kernelType"] for r in records(p.stdout)] == ["0", "1", "2", "3", "4", "5", "6"]


def test_sweep_tool_runs_the_panel_kernel(tmp_path):
    """tools/sparsity_sweep.py passes --panels for CSR: one `panels density ...` line per density, correct, with the tag."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sparsity_sweep.py"), "--densities", "0.05,0.5", "--rows", "256", "--cols", "256",
                        "--k", "64", "--iters", "5", "--formats", "csr", "--out", str(tmp_path / "sweep")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    panel = [l for l in p.stdout.splitlines() if l.startswith("panels density")]
    assert len(panel) == 2 and all(" kernel  7 correct 1 " in l and " us " in l and "csr_panel<ref," in l for l in panel), p.stdout
    assert len([l for l in p.stdout.splitlines() if l.startswith("density")]) == 2 * 8
