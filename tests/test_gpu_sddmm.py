"""SDDMM on a CSR pattern (mispmm_sddmm_csr_f32 / _f64), the transposed product and the autograd function built on the two,
on the GPU, against the numpy restatements and bounds of tests/_sddmm_ref.py."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, formats, ops  # noqa: E402

from _bits import assert_same_bits  # noqa: E402
from _ref64 import assert_same_bits64, ref_rows  # noqa: E402
from _sddmm_ref import (assert_within, dense_of, entry_rows, full_mantissa, matrix, sddmm_exact, sddmm_f64,  # noqa: E402
                        small_ints)

pytestmark = pytest.mark.gpu

MATRICES = ["qh1484", "ragged", "long", "unsorted"]
WIDTHS = [1, 3, 4, 63, 64, 65, 200, 512]
DTYPES = {"f32": (np.float32, torch.float32), "f64": (np.float64, torch.float64)}
MODES = ("reference", "fast")


@functools.lru_cache(maxsize=None)
def device_csr(name):
    return ops.DeviceCSR.from_host(matrix(name), plan=False)


@functools.lru_cache(maxsize=None)
def operands(name, n, dt, kind="full"):
    """(x, y) on the host for (matrix, N, dtype), shared by the tests that use them; read-only."""
    csr = matrix(name)
    rng = np.random.default_rng(1000 + n)
    make = full_mantissa if kind == "full" else small_ints
    return make(rng, (csr.num_rows, n), DTYPES[dt][0]), make(rng, (csr.num_cols, n), DTYPES[dt][0])


@functools.lru_cache(maxsize=None)
def reference(name, n, dt, kind="full"):
    csr = matrix(name)
    return sddmm_exact(csr.row_ptrs, csr.col_idxs, *operands(name, n, dt, kind))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("name", MATRICES)
def test_sddmm_within_the_stated_bounds(name, n, dt):
    a = device_csr(name)
    x, y = operands(name, n, dt)
    exact, scale = reference(name, n, dt)
    xd, yd = dev(x), dev(y)
    for acc in MODES:
        out = ops.sddmm_csr(a, xd, yd, acc=acc)
        assert capi.last_kernel().startswith("sddmm_csr<"), capi.last_kernel()
        assert out.shape == (a.nnz,) and out.dtype == DTYPES[dt][1]
        assert_within(out.cpu().numpy(), DTYPES[dt][0], acc, n, exact, scale, f"{name} N={n} {dt} {acc} {capi.last_kernel()}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("name", MATRICES)
def test_sddmm_is_exact_on_small_integers(name, n, dt):
    a = device_csr(name)
    x, y = operands(name, n, dt, "ints")
    exact, _ = reference(name, n, dt, "ints")
    xd, yd = dev(x), dev(y)
    for acc in MODES:
        got = ops.sddmm_csr(a, xd, yd, acc=acc).cpu().numpy()
        assert np.array_equal(got.astype(np.float64), exact), f"{name} N={n} {dt} {acc}: {int((got != exact).sum())} entries differ"


# the chunked bodies the widths above leave out: 4 register chunks of 16-byte lanes (f32 N = 1024), the chunk loop with
# 16-byte lanes (N = 1028 / 516) and with narrow ones (N = 257), 4 narrow chunks (N = 255).  Not every instance the dispatcher
# can pick: tests/test_gpu_census.py runs each of the 56 by its tag (table sddmm_csr of tests/_census.py).
@pytest.mark.parametrize("dt,n,tag", [("f32", 1024, "V4,C4"), ("f32", 1028, "V4,C0"), ("f32", 257, "V1,C0"), ("f32", 255, "V1,C4"),
                                      ("f64", 516, "V2,C0"), ("f64", 257, "V1,C0"), ("f64", 129, "V1,C4")])
def test_sddmm_wide_rows_take_the_chunked_bodies(dt, n, tag):
    name = "long"
    a = device_csr(name)
    for kind in ("full", "ints"):
        xd, yd = (dev(v) for v in operands(name, n, dt, kind))
        exact, scale = reference(name, n, dt, kind)
        for acc in MODES:
            got = ops.sddmm_csr(a, xd, yd, acc=acc).cpu().numpy()
            assert tag in capi.last_kernel(), capi.last_kernel()
            if kind == "ints":
                assert np.array_equal(got.astype(np.float64), exact)
            else:
                assert_within(got, DTYPES[dt][0], acc, n, exact, scale, f"long N={n} {dt} {acc} {capi.last_kernel()}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name,n,pad", [("long", 64, 4), ("long", 64, 3), ("ragged", 200, 8), ("unsorted", 5, 2), ("long", 512, 4)])
def test_sddmm_strided_operands_and_out_sentinels(name, n, pad, dt):
    """ldx, ldy > N with NaN in the gap columns (a kernel that reads a gap poisons its sum), and `out` as the head of a longer
    buffer whose tail must stay untouched."""
    a = device_csr(name)
    x, y = operands(name, n, dt)
    exact, scale = reference(name, n, dt)
    tdt = DTYPES[dt][1]
    xb = torch.full((a.num_rows, n + pad), float("nan"), dtype=tdt, device="cuda")
    yb = torch.full((a.num_cols, n + 2 * pad), float("nan"), dtype=tdt, device="cuda")
    xb[:, :n], yb[:, :n] = dev(x), dev(y)
    for acc in MODES:
        buf = torch.full((a.nnz + 37,), -7.0, dtype=tdt, device="cuda")
        got = ops.sddmm_csr(a, xb[:, :n], yb[:, :n], out=buf[:a.nnz], acc=acc)
        assert got.data_ptr() == buf.data_ptr()
        assert ("V1" in capi.last_kernel()) == (pad % (4 if dt == "f32" else 2) != 0 or n % (4 if dt == "f32" else 2) != 0), capi.last_kernel()
        assert bool((buf[a.nnz:] == -7.0).all()), "elements behind out[nnz - 1] were written"
        assert_within(got.cpu().numpy(), DTYPES[dt][0], acc, n, exact, scale, f"strided {name} N={n} pad={pad} {dt} {acc}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("which", ["x", "y"])
@pytest.mark.parametrize("name,n", [("long", 64), ("long", 200), ("long", 512)])
def test_sddmm_misaligned_operand_takes_the_narrow_body(name, n, which, dt):
    """An operand that starts one element into its buffer is not 16-byte aligned: one element per lane, same results."""
    a = device_csr(name)
    x, y = operands(name, n, dt)
    exact, scale = reference(name, n, dt)

    def shifted(v):
        flat = torch.full((v.size + 1,), float("nan"), dtype=DTYPES[dt][1], device="cuda")
        flat[1:] = dev(v).reshape(-1)
        return flat[1:].view(v.shape)
    xd, yd = (shifted(x), dev(y)) if which == "x" else (dev(x), shifted(y))
    assert (xd.data_ptr() % 16 != 0) or (yd.data_ptr() % 16 != 0)
    for acc in MODES:
        got = ops.sddmm_csr(a, xd, yd, acc=acc).cpu().numpy()
        assert "V1" in capi.last_kernel(), capi.last_kernel()
        assert_within(got, DTYPES[dt][0], acc, n, exact, scale, f"misaligned {which} N={n} {dt} {acc}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name,n", [("long", 64), ("unsorted", 5), ("ragged", 200)])
def test_sddmm_nan_and_inf_stay_where_they_belong(name, n, dt):
    csr, a = matrix(name), device_csr(name)
    x, y = (v.copy() for v in operands(name, n, dt))
    rows, cols = entry_rows(csr.row_ptrs), csr.col_idxs.astype(np.int64)
    mid = csr.nnz // 2
    x[rows[mid], n // 2] = np.nan
    y[cols[0], 0] = np.inf
    y[cols[-1], n - 1] = -np.inf
    x[rows[csr.nnz // 3], n // 3] = np.inf
    want = sddmm_f64(csr.row_ptrs, csr.col_idxs, x, y)
    finite = np.isfinite(want)
    assert (~finite).any() and np.isnan(want).any() and np.isinf(want).any() and finite.sum() > csr.nnz // 2
    xf, yf = np.where(np.isfinite(x), x, 0), np.where(np.isfinite(y), y, 0)      # for the finite entries: same sums
    exact, scale = sddmm_exact(csr.row_ptrs, csr.col_idxs, xf, yf)
    for acc in MODES:
        got = ops.sddmm_csr(a, dev(x), dev(y), acc=acc).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{acc}: NaN positions differ"
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.signbit(got[np.isinf(got)]), np.signbit(want[np.isinf(want)]))
        assert_within(got[finite], DTYPES[dt][0], acc, n, exact[finite], scale[finite], f"finite entries {name} N={n} {dt} {acc}")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_sddmm_zero_width_writes_plus_zero(dt):
    a = device_csr("long")
    tdt = DTYPES[dt][1]
    for acc in MODES:
        out = torch.full((a.nnz,), -0.0, dtype=tdt, device="cuda")
        ops.sddmm_csr(a, torch.empty((a.num_rows, 0), dtype=tdt, device="cuda"), torch.empty((a.num_cols, 0), dtype=tdt, device="cuda"),
                      out=out, acc=acc)
        assert capi.last_kernel().startswith("sddmm_csr<")
        got = out.cpu().numpy()
        assert not got.any() and not np.signbit(got).any()


def test_sddmm_empty_patterns_are_no_ops():
    x, y = torch.ones((5, 8), device="cuda"), torch.ones((7, 8), device="cuda")
    empty = ops.DeviceCSR.from_host(formats.CSR(5, 7, np.zeros(6, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32)), plan=False)
    assert ops.sddmm_csr(empty, x, y).shape == (0,)
    none = ops.DeviceCSR.from_host(formats.CSR(0, 7, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32)), plan=False)
    assert ops.sddmm_csr(none, torch.ones((0, 8), device="cuda"), y).shape == (0,)
    with pytest.raises(ValueError):
        ops.sddmm_csr(empty, x, y.double())
    with pytest.raises(ValueError):
        ops.sddmm_csr(empty, x, y[:, :4])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_sddmm_is_deterministic_and_replays_from_a_graph(dt):
    name, n = "long", 200
    a = device_csr(name)
    xd, yd = (dev(v) for v in operands(name, n, dt))
    same = assert_same_bits if dt == "f32" else assert_same_bits64
    for acc in MODES:
        eager = ops.sddmm_csr(a, xd, yd, acc=acc).clone()
        same(ops.sddmm_csr(a, xd, yd, acc=acc), eager, f"second run {acc}")
        out = torch.empty_like(eager)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.sddmm_csr(a, xd, yd, out=out, acc=acc)             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.sddmm_csr(a, xd, yd, out=out, acc=acc)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        same(out, eager, f"graph replay {acc}")


# ---- the transposed product
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name,n", [("ragged", 3), ("ragged", 64), ("long", 3), ("long", 64), ("n4c6-b13", 64)])
def test_transposed_product_reference_mode_is_the_oracle_on_the_transposed_arrays(name, n, dt, oracle):
    csr = matrix(name)
    rng = np.random.default_rng(31)
    t, perm = ops.csr_transpose(csr)
    if dt == "f32":
        g = full_mantissa(rng, (csr.num_rows, n), np.float32)
        got = ops.spmm_csr(ops.DeviceCSR.from_host(t, plan=False), dev(g))
        assert_same_bits(got, oracle.spmm_csr(t.row_ptrs, t.col_idxs, t.data, g), f"A^T G {name} N={n}")
    else:
        # the oracle is the reference's fp32 CSR engine and has no fp64 form; as in tests/test_gpu_f64.py the fp64 contract
        # (product and add rounded once each, in list order) is its numpy restatement, _ref64.ref_rows
        vals = full_mantissa(rng, csr.nnz, np.float64)
        t = formats.CSR(t.num_rows, t.num_cols, t.row_ptrs, t.col_idxs, vals[perm.astype(np.int64)])
        g = full_mantissa(rng, (csr.num_rows, n), np.float64)
        got = ops.spmm_csr(ops.DeviceCSR.from_host(t, plan=False, dtype=torch.float64), dev(g))
        assert_same_bits64(got, ref_rows(t.row_ptrs, t.col_idxs, t.data, g), f"A^T G {name} N={n} f64")


# ---- autograd
def _tiny():
    """7 x 9, 20 entries, row 2 empty, column 4 twice in row 5."""
    lens = [3, 4, 0, 2, 5, 4, 2]
    cols = [0, 3, 8, 1, 2, 5, 7, 4, 6, 0, 1, 3, 5, 8, 4, 2, 4, 7, 6, 8]
    rng = np.random.default_rng(41)
    return formats.CSR(7, 9, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), np.array(cols, np.uint32),
                       rng.uniform(-1, 1, 20).astype(np.float64))


@pytest.mark.parametrize("acc", MODES)
def test_autograd_gradcheck_in_float64(acc):
    csr = _tiny()
    a = autograd.TrainableCSR.from_host(csr, dtype=torch.float64)
    rng = np.random.default_rng(42)
    b0 = dev(rng.uniform(-1, 1, (9, 5)))
    for wv, wb in ((True, True), (True, False), (False, True)):
        values = a.values.clone().requires_grad_(wv)
        b = b0.clone().requires_grad_(wb)
        assert torch.autograd.gradcheck(lambda v, m: autograd.spmm(a, v, m, acc=acc), (values, b))
    want = dense_of(csr) @ b0.cpu().numpy()
    assert np.allclose(autograd.spmm(a, a.values, b0).cpu().numpy(), want, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("n", [3, 64])
@pytest.mark.parametrize("name", ["ragged", "long"])
def test_autograd_float32_gradients(name, n, oracle):
    csr = matrix(name)
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(43)
    b_h, g_h = full_mantissa(rng, (csr.num_cols, n), np.float32), full_mantissa(rng, (csr.num_rows, n), np.float32)
    t, _ = ops.csr_transpose(csr)
    exact, scale = sddmm_exact(csr.row_ptrs, csr.col_idxs, g_h, b_h)
    for acc in MODES:
        values = a.values.clone().requires_grad_(True)
        b = dev(b_h).requires_grad_(True)
        c = autograd.spmm(a, values, b, acc=acc)
        assert_same_bits(c, ops.spmm_csr(a.fwd, dev(b_h), acc=acc), f"forward {acc}")          # forward parity
        c.backward(dev(g_h))
        if acc == "reference":
            assert_same_bits(b.grad, oracle.spmm_csr(t.row_ptrs, t.col_idxs, t.data, g_h), "grad_b")
            assert_same_bits(c, oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b_h), "forward against the oracle")
        else:
            want = dense_of(csr).T @ g_h.astype(np.float64)
            lim = 1e-5 * (np.abs(dense_of(csr)).T @ np.abs(g_h).astype(np.float64))
            assert np.all(np.abs(b.grad.cpu().numpy() - want) <= lim + 1e-30)
        assert_within(values.grad.cpu().numpy(), np.float32, acc, n, exact, scale, f"grad_values {name} N={n} {acc}")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_autograd_sum_backward_takes_a_stride_zero_gradient(dt):
    csr = matrix("long")
    a = autograd.TrainableCSR.from_host(csr, dtype=DTYPES[dt][1])
    rng = np.random.default_rng(44)
    b_h = small_ints(rng, (csr.num_cols, 6), DTYPES[dt][0])
    values = a.values.clone().requires_grad_(True)
    b = dev(b_h).requires_grad_(True)
    autograd.spmm(a, values, b).sum().backward()
    # d sum(C) / d values[e] = sum_j B[col(e)][j];  d sum(C) / d B[k][j] = sum of column k of A: integers / short exact sums
    assert np.array_equal(values.grad.cpu().numpy().astype(np.float64), b_h.astype(np.float64).sum(axis=1)[csr.col_idxs.astype(np.int64)])
    col_sums = dense_of(csr).sum(axis=0)
    assert np.allclose(b.grad.cpu().numpy(), np.repeat(col_sums[:, None], 6, axis=1), rtol=1e-5, atol=1e-6)


def test_autograd_frozen_inputs_skip_their_kernel():
    csr = matrix("long")
    a = autograd.TrainableCSR.from_host(csr)
    b_h = full_mantissa(np.random.default_rng(45), (csr.num_cols, 8), np.float32)
    # the tag of the last kernel is kept per thread: run the backward pass on this one
    with torch.autograd.set_multithreading_enabled(False):
        values, b = a.values.clone().requires_grad_(True), dev(b_h)
        c = autograd.spmm(a, values, b)
        assert not capi.last_kernel().startswith("sddmm_csr<")
        c.sum().backward()
        assert capi.last_kernel().startswith("sddmm_csr<"), capi.last_kernel()      # the last and only kernel of this backward
        assert b.grad is None and values.grad is not None
        values, b = a.values.clone(), dev(b_h).requires_grad_(True)
        c = autograd.spmm(a, values, b)
        ops.sddmm_csr(a.fwd, c.detach(), b.detach())                                # leave an SDDMM tag behind ...
        assert capi.last_kernel().startswith("sddmm_csr<")
        c.sum().backward()
        assert not capi.last_kernel().startswith("sddmm_csr<"), capi.last_kernel()  # ... which the product with A^T replaces
        assert values.grad is None and b.grad is not None
        # and with both trainable the SDDMM does run, then the transposed product
        values, b = a.values.clone().requires_grad_(True), dev(b_h).requires_grad_(True)
        autograd.spmm(a, values, b).sum().backward()
        assert values.grad is not None and b.grad is not None
    out = autograd.spmm(a, a.values, dev(b_h))
    assert out.grad_fn is None and not out.requires_grad
    with pytest.raises(ValueError):
        autograd.spmm(a, a.values.double(), dev(b_h))
