"""The straight-line row-gather body (row_line_kernel in csrc/row_gather.hpp: uniform CSR and ELL rows of 9..14 entries)
against the CPU oracle, through the C ABI.  REFERENCE mode: the oracle's bits.  FAST mode: the bits of the fma chain
(tests/_fma_chain.py).  Operands come from tests/_uniform_line_cases.py; tests/test_uniform_line_cpu.py checks on the CPU
what they promise.  Every launch must name the body in its tag: row_gather<...,line,S..>."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mispmm import capi, formats, ops  # noqa: E402

import _fma_chain as fc  # noqa: E402
import _uniform_line_cases as cases  # noqa: E402
from _bits import assert_gap_untouched, assert_same_bits, sentinel_buffer  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs a GPU"
    assert os.path.exists(capi.LIB_PATH), "libmispmm.so must be built (no fallback path exists)"
    capi.lib()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def slots_of(width):
    return width + width % 2


def assert_line_tag(width, rows="uniform", *more):
    tag = capi.last_kernel()
    assert tag.startswith("row_gather<") and f",{rows},B128,U8,line,S{slots_of(width)}>" in tag, tag
    for word in more:
        assert word in tag, (word, tag)
    return tag


def filled_out(m, n):
    return torch.full((m, n), 7.0, dtype=torch.float32, device="cuda")


@pytest.fixture(scope="module")
def big_b():
    """One [BIG_K, 256] operand for all widths, on the host and on the device."""
    b = cases.dense_b(cases.BIG_K, 256)
    return b, dev(b)


@pytest.mark.parametrize("width", cases.WIDTHS)
def test_uniform_csr_reference_is_bit_exact(oracle, width):
    """M in {1, 7, 8, 9, 33} x N in {64, 128, 192, 256, 512}: a partial workgroup, one row, empty row parts of the XCD grid,
    a short last part; the 8 x 1, 4 x 2, 2 x 4, 8-lane-group (N = 192) and 1 x 8 tilings."""
    k = 40
    for m in cases.ROW_COUNTS:
        csr = cases.uniform_csr(m, k, width, 100 * width + m)
        a = ops.DeviceCSR.from_host(csr, spans=False, plan=False)
        assert a.uniform_row_nnz == width
        for n in cases.COL_COUNTS:
            b = cases.dense_b(k, n)
            out = ops.spmm_csr(a, dev(b), out=filled_out(m, n))
            tag = assert_line_tag(width)
            assert_same_bits(out, oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b), f"W={width} M={m} N={n} [{tag}]")


@pytest.mark.parametrize("width", cases.WIDTHS)
def test_uniform_csr_strided_operands_keep_their_gaps(oracle, width):
    """ldb > N and ldc > N at N = 128: B's gap columns hold NaN, C's gap columns a sentinel that must survive."""
    m, k, n, ldb, ldc = 33, 40, 128, 136, 132
    csr = cases.uniform_csr(m, k, width, 200 + width)
    b = cases.dense_b(k, n)
    bw = torch.full((k, ldb), float("nan"), dtype=torch.float32, device="cuda")
    bw[:, :n] = dev(b)
    cw = sentinel_buffer(m, n, ldc, torch)
    ops.spmm_csr(ops.DeviceCSR.from_host(csr, spans=False, plan=False), bw[:, :n], out=cw[:, :n])
    tag = assert_line_tag(width)
    assert_same_bits(cw[:, :n], oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b), f"W={width} strided [{tag}]")
    assert_gap_untouched(cw, n, f"W={width} strided")


@pytest.mark.parametrize("width", cases.WIDTHS)
def test_uniform_csr_smallest_and_large_k(oracle, width, big_b):
    """K as small as the row (every row reads every B row), and K x 256 B > 4 MiB at N = 256 (eight 32-column parts of 8-lane
    groups) with columns over the whole range, the first and the last B row included."""
    for n in (128, 256):
        csr = cases.uniform_csr(9, width, width, 300 + width)
        b = cases.dense_b(width, n)
        out = ops.spmm_csr(ops.DeviceCSR.from_host(csr, spans=False, plan=False), dev(b), out=filled_out(9, n))
        tag = assert_line_tag(width)
        assert_same_bits(out, oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b), f"W={width} K={width} N={n} [{tag}]")
    b, bd = big_b
    csr = cases.uniform_csr(33, cases.BIG_K, width, 400 + width)
    assert csr.col_idxs.min() == 0 and csr.col_idxs.max() == cases.BIG_K - 1 and cases.BIG_K * 256 > (4 << 20)
    out = ops.spmm_csr(ops.DeviceCSR.from_host(csr, spans=False, plan=False), bd, out=filled_out(33, 256))
    tag = assert_line_tag(width, "uniform", "xcd 1x8")
    assert tag.startswith("row_gather<G8,"), tag
    assert_same_bits(out, oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b), f"W={width} K={cases.BIG_K} [{tag}]")


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("width", [10, 14])
def test_ell_with_padded_rows_is_bit_exact(oracle, width, n):
    """Real lengths 0 .. width, all-padding rows included: padding is a dropped load with a zero coefficient."""
    csr = cases.padded_ell_csr(width, 500 + width)
    ellc = formats.csr_to_ell_colmajor(csr)
    a = ops.DeviceELL.from_host(ellc, compact=False)
    assert a.width == width and a.compact is None
    b = cases.dense_b(csr.num_cols, n)
    ref = oracle.spmm_ell_colmajor(ellc.num_rows, ellc.row_idxs, ellc.data, b)
    out = ops.spmm_ell(a, dev(b), out=filled_out(csr.num_rows, n))
    tag = assert_line_tag(width, "ell")
    assert_same_bits(out, ref, f"ELL W={width} N={n} [{tag}]")
    out = ops.spmm_ell(a, dev(b), out=filled_out(csr.num_rows, n), acc="fast")
    tag = assert_line_tag(width, "ell", "fast")
    assert_same_bits(out, oracle.rows_fma(*fc.ell_colmajor_rows(ellc), b), f"ELL FAST W={width} N={n} [{tag}]")


@pytest.mark.parametrize("width", cases.WIDTHS)
def test_uniform_csr_fast_returns_the_fma_chain(oracle, width):
    csr = cases.uniform_csr(9, 40, width, 600 + width)
    b = cases.dense_b(40, 128)
    rows = fc.csr_rows(csr)
    assert fc.corpus_is_sharp(rows, b)
    out = ops.spmm_csr(ops.DeviceCSR.from_host(csr, spans=False, plan=False), dev(b), out=filled_out(9, 128), acc="fast")
    tag = assert_line_tag(width, "uniform", "fast")
    assert_same_bits(out, oracle.rows_fma(*rows, b), f"FAST W={width} [{tag}]")


def test_adversarial_rows_of_width_14(oracle):
    """(3e38, 3e38, -3e38), (1, 2^-30, -1), big / small orders across the slot 7 / 8 boundary, Inf and NaN rows of B, sums of
    -0 products: the oracle's bits in REFERENCE mode, the chain's in FAST mode."""
    csr, b, expect = cases.adversarial(128)
    ref = oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b)
    for r, want in expect.items():
        assert_same_bits(ref[r], want, f"the oracle on adversarial row {r}")
    a = ops.DeviceCSR.from_host(csr, spans=False, plan=False)
    out = ops.spmm_csr(a, dev(b), out=filled_out(csr.num_rows, 128))
    tag = assert_line_tag(14)
    assert_same_bits(out, ref, f"adversarial [{tag}]")
    out = ops.spmm_csr(a, dev(b), out=filled_out(csr.num_rows, 128), acc="fast")
    tag = assert_line_tag(14, "uniform", "fast")
    assert_same_bits(out, oracle.rows_fma(*fc.csr_rows(csr), b), f"adversarial FAST [{tag}]")


@pytest.mark.parametrize("acc", ["reference", "fast"])
def test_plan_order_and_batches_equal_the_plain_product(oracle, acc):
    """A row map (plan order) through ops.spmm_csr, batches of 1, 2 and 16 operands with and without the row map: all equal
    to the unbatched, unmapped product, which equals the oracle."""
    width, m, k, n = 14, 33, 40, 128
    csr = cases.uniform_csr(m, k, width, 700)
    bs = [cases.dense_b(k, n)] + [fc.sharp_values(np.random.default_rng(710 + i), (k, n), np.float32) for i in range(2)]
    plain = ops.DeviceCSR.from_host(csr, spans=False, plan=False)
    singles = []
    for b in bs:
        singles.append(ops.spmm_csr(plain, dev(b), out=filled_out(m, n), acc=acc).cpu().numpy())
        tag = assert_line_tag(width)
        assert "plan-order" not in tag and "batched" not in tag
    want = oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, bs[0]) if acc == "reference" else oracle.rows_fma(*fc.csr_rows(csr), bs[0])
    assert_same_bits(singles[0], want, f"single launch, {acc}")
    planned = ops.DeviceCSR.from_host(csr, spans=False, plan=True)
    order = planned.plan.row_map.cpu().numpy().view(np.uint32)
    assert sorted(order.tolist()) == list(range(m))
    planned.tuned[(n, acc)] = (True, (0.0, 0.0))             # take the plan: nothing to measure in a test
    out = ops.spmm_csr(planned, dev(bs[0]), out=filled_out(m, n), acc=acc)
    assert_line_tag(width, "uniform", "plan-order")
    assert_same_bits(out, singles[0], f"plan order, {acc}")
    for count in (1, 2, 16):
        for a, words in ((plain, ("batched",)), (planned, ("plan-order",) + (("batched",) if count > 1 else ()))):
            outs = ops.spmm_csr_batch(a, [dev(bs[i % 3]) for i in range(count)], outs=[filled_out(m, n) for _ in range(count)], acc=acc)
            tag = assert_line_tag(width, "uniform", *words)
            for i, o in enumerate(outs):
                assert_same_bits(o, singles[i % 3], f"batch of {count}, operand {i} [{tag}]")
