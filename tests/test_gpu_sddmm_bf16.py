"""SDDMM on a CSR pattern with X and Y in bf16 on the GPU (mispmm_sddmm_csr_bf16 behind sddmm_bf16.sddmm_csr_bf16 and
autograd.spmm_bf16(..., sddmm="bf16")).  Every parity check is BIT FOR BIT: FAST against the numpy restatement of ALGORITHM
(tests/_sddmm_bf16_ref.py), REFERENCE against the restatement AND against the correctly rounded exact sum (the operands'
exact sums fit a double), and on element lanes against the fp32 kernel on the widened operands.  The one tolerance is the
header's bound (c) for FAST, checked beside the bits with the worst ratio printed."""
import numpy as np
import pytest

import _sddmm_bf16_ref as ref
from _sddmm_ref import assert_within
from mispmm import capi_sddmm_bf16, ops, sddmm_bf16

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC1                      # int16 pairs of it make a quiet NaN in fp32 too: fills the gaps of strided operands
ACCS = ("fast", "reference")
f = sddmm_bf16.sddmm_csr_bf16


def _dev_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


@pytest.fixture(scope="module")
def patterns():
    """name -> DeviceCSR of the shared cases, uploaded once."""
    return {name: ops.DeviceCSR.from_host(ref.case(name).csr, plan=False) for name in ("census", "ragged", "long", "unsorted", "tall", "flat")}


def _check(c, a, n, acc):
    """One (pattern, width, arithmetic) against the restatement, in REFERENCE against the rounded exact sum too; both out
    types.  Returns the fp32 result."""
    x, y = _dev_bits(c.x_bits[:, :n]), _dev_bits(c.y_bits[:, :n])
    got = _host(f(a, x, y, acc=acc))
    tag = capi_sddmm_bf16.last_kernel()
    assert tag == ref.tag_of(acc, n), tag
    want = c.expected(acc, n)
    assert ref.same_bits(got, want), f"{c.name} N={n} {acc}: {int(np.sum(got.view(np.uint32) != want.view(np.uint32)))} of {want.size} entries differ from ALGORITHM"
    rounded, exact, scale = c.exact(n)
    if acc == "reference":
        assert ref.same_bits(got, rounded), f"{c.name} N={n}: REFERENCE is not the correctly rounded exact sum"
    got16 = _host(f(a, x, y, out_bf16=True, acc=acc))
    assert capi_sddmm_bf16.last_kernel() == ref.tag_of(acc, n, out_bf16=True)
    assert ref.same_bits(got16, ref.bf16_bits(want)), f"{c.name} N={n} {acc}: the bf16 out is not the rounded fp32 out"
    return got


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("n", sorted(ref.V8_WIDTHS) + sorted(ref.V1_WIDTHS))
def test_every_instance_on_short_rows(patterns, n, acc):
    """70 x 90, rows of 0-12 entries: one width per tag, the smallest that reaches it -- with the two arithmetics every
    instance of the CPU census."""
    assert ref.TAGS[ref.head(ref.tag_of(acc, n))] == n
    _check(ref.case("census"), patterns["census"], n, acc)


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("name", ["ragged", "long", "unsorted", "tall", "flat"])
def test_ragged_long_unsorted_tall_and_flat_patterns(patterns, name, acc):
    """Empty rows (first and last among them), a row of 300 entries, unsorted and repeated columns, M >> K and K >> M, on
    16-byte lanes (N = 40) and on element lanes (N = 33)."""
    c = ref.case(name)
    for n in (40, 33):
        got = _check(c, patterns[name], n, acc)
        if acc == "fast":
            _, exact, scale = c.exact(n)
            assert_within(got, np.float32, "fast", n, exact, scale, f"{name} N={n} FAST")


@pytest.mark.parametrize("acc", ACCS)
def test_reference_order_shows_where_the_sums_do_not_fit_a_double(patterns, acc):
    """Operands of exponents -40 .. 40 whose large products cancel: the result is what the order of the chain leaves, and it
    is ALGORITHM's on both lane widths (the CPU test shows that the two differ there, and from the exact sum)."""
    for name, n in (("census", 264), ("ragged", 40)):
        c = ref.case(name)
        xb, yb = c.far(n)
        for ld, v in ((n, 8), (n + 3, 1)):
            x, y = _strided(xb, ld), _strided(yb, ld)
            got = _host(f(patterns[name], x, y, acc=acc))
            assert f",V{v}," in capi_sddmm_bf16.last_kernel()
            assert ref.same_bits(got, c.expected(acc, n, v, far=True)), (name, n, v)


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("n", [33, 257])
def test_element_lanes_equal_the_fp32_kernel_on_the_widened_operands(patterns, n, acc):
    c, a = ref.case("census"), patterns["census"]
    xb, yb = c.x_bits[:, :n], c.y_bits[:, :n]
    got = _host(f(a, _dev_bits(xb), _dev_bits(yb), acc=acc))
    assert ",V1," in capi_sddmm_bf16.last_kernel()
    want = ops.sddmm_csr(a, torch.from_numpy(ref.widen(xb)).cuda(), torch.from_numpy(ref.widen(yb)).cuda(), acc=acc)
    from mispmm import capi
    assert ",V1," in capi.last_kernel(), capi.last_kernel()
    assert ref.same_bits(got, _host(want))


def _strided(host_bits, ld, offset=0):
    """bf16 bits [rows, n] on the device, rows ld apart, the first element `offset` elements into a 16-byte aligned buffer;
    the gaps hold the sentinel, a NaN."""
    rows, n = host_bits.shape
    buf = torch.full((offset + rows * ld,), SENTINEL, dtype=torch.int16, device="cuda")
    view = buf[offset:].view(rows, ld)[:, :n]
    view.copy_(_dev_bits(host_bits))
    return view


@pytest.mark.parametrize("acc", ACCS)
def test_strided_operands_whose_gap_columns_hold_nan(patterns, acc):
    c, a = ref.case("ragged"), patterns["ragged"]
    # (N, ldx, ldy, offset of X, offset of Y, lane width)
    rows = [(40, 48, 48, 0, 0, 8), (40, 48, 40, 8, 0, 8), (40, 48, 48, 1, 0, 1), (40, 43, 48, 0, 0, 1),
            (33, 41, 41, 0, 0, 1), (33, 36, 36, 1, 1, 1), (33, 36, 33, 1, 0, 1)]
    for n, ldx, ldy, xo, yo, v in rows:
        x, y = _strided(c.x_bits[:, :n], ldx, xo), _strided(c.y_bits[:, :n], ldy, yo)
        got = _host(f(a, x, y, acc=acc))
        tag = capi_sddmm_bf16.last_kernel()
        assert tag == ref.tag_of(acc, n, ldx, ldy, xo, yo) and f",V{v}," in tag, (tag, n, ldx, ldy, xo, yo)
        assert not np.isnan(got).any(), f"a gap column was read ({tag})"
        assert ref.same_bits(got, c.expected(acc, n, v)), (tag, n, ldx, ldy, xo, yo)


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("n", [40, 33])
def test_nan_and_inf_stay_in_the_entries_that_touch_them(patterns, n, acc):
    """A NaN row and a +Inf row of X, an Inf - Inf row and a NaN row of Y: exactly the entries of those rows and columns are
    NaN / Inf, all others keep their bits."""
    c, a = ref.case("ragged"), patterns["ragged"]
    rp, ci = c.row_ptrs.astype(np.int64), c.col_idxs.astype(np.int64)
    lens = np.diff(rp)
    r_nan, r_inf = [int(r) for r in np.flatnonzero(lens >= 3)[:2]]
    used = np.setdiff1d(np.unique(ci), ci[rp[r_nan]:rp[r_nan + 1]].tolist() + ci[rp[r_inf]:rp[r_inf + 1]].tolist())
    c_mix, c_nan = int(used[0]), int(used[1])
    xb, yb = c.x_bits[:, :n].copy(), c.y_bits[:, :n].copy()
    xb[r_nan, 5] = 0x7FC0
    xb[r_inf, 2] = 0x7F80                                 # +Inf times a finite, non-zero y
    yb[c_mix, 1], yb[c_mix, n - 1] = 0x7F80, 0x7F80       # +-Inf products of both signs below: Inf - Inf
    xb[:, 1] = (xb[:, 1] & 0x7FFF)
    xb[:, n - 1] = (xb[:, n - 1] | 0x8000)
    yb[c_nan, 0] = 0xFFC1
    want = ref.restate(acc, c.row_ptrs, c.col_idxs, xb, yb)
    rows = np.repeat(np.arange(lens.shape[0]), lens)
    nan_at = (rows == r_nan) | (ci == c_mix) | (ci == c_nan)
    inf_at = (rows == r_inf) & ~nan_at
    assert np.array_equal(np.isnan(want), nan_at) and np.array_equal(np.isinf(want), inf_at) and inf_at.sum() >= 3 and nan_at.sum() >= 5
    got = _host(f(a, _dev_bits(xb), _dev_bits(yb), acc=acc))
    assert np.array_equal(np.isnan(got), nan_at) and np.array_equal(np.isinf(got), inf_at)
    assert ref.same_bits(got, want)
    # the entries that touch none of them: the bits of the run without special values, but for the two sign columns
    clean = ref.restate(acc, c.row_ptrs, c.col_idxs, np.where(np.isin(np.arange(n), [1, n - 1])[None, :], xb, c.x_bits[:, :n]), c.y_bits[:, :n])
    keep = ~(nan_at | inf_at)
    assert np.array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))
    got16 = _host(f(a, _dev_bits(xb), _dev_bits(yb), out_bf16=True, acc=acc))
    assert ref.same_bits(got16, ref.bf16_bits(want))


def test_edge_shapes_no_columns_no_entries_no_rows(patterns):
    from mispmm import formats
    c, a = ref.case("census"), patterns["census"]
    assert c.row_ptrs[1] == 0 and c.row_ptrs[-1] == c.row_ptrs[-2]          # empty first and last rows (every census case ran them)
    m, k, nnz = c.csr.num_rows, c.csr.num_cols, a.nnz
    for out_bf16, dtype in ((False, torch.float32), (True, torch.int16)):
        out = torch.full((nnz,), 0x7FC1, dtype=torch.int16, device="cuda") if out_bf16 else torch.full((nnz,), float("nan"), device="cuda")
        got = f(a, torch.zeros((m, 0), dtype=torch.int16, device="cuda"), torch.zeros((k, 0), dtype=torch.int16, device="cuda"),
                out_bf16=out_bf16, out=out)
        assert capi_sddmm_bf16.last_kernel() == "sddmm_csr_bf16<zero>"
        assert got.dtype == dtype and _host(got).view(np.uint16).max() == 0           # +0 everywhere
    empty = ops.DeviceCSR.from_host(formats.CSR(5, 7, np.zeros(6, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32)), plan=False)
    got = f(empty, _dev_bits(c.x_bits[:5, :8]), _dev_bits(c.y_bits[:7, :8]))
    assert got.shape == (0,) and got.dtype == torch.float32
    none = ops.DeviceCSR.from_host(formats.CSR(0, 7, np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32)), plan=False)
    got = f(none, torch.zeros((0, 8), dtype=torch.int16, device="cuda"), _dev_bits(c.y_bits[:7, :8]), out_bf16=True)
    assert got.shape == (0,) and got.dtype == torch.int16
    torch.cuda.synchronize()


@pytest.mark.parametrize("out_bf16", [False, True])
def test_out_is_taken_and_nothing_is_written_past_its_end(patterns, out_bf16):
    c, a = ref.case("census"), patterns["census"]
    n, nnz = 40, a.nnz
    buf = torch.full((nnz + 16,), SENTINEL, dtype=torch.int16, device="cuda") if out_bf16 else \
        torch.full((2 * (nnz + 16),), SENTINEL, dtype=torch.int16, device="cuda").view(torch.float32)
    out = buf[:nnz]
    got = f(a, _dev_bits(c.x_bits[:, :n]), _dev_bits(c.y_bits[:, :n]), out_bf16=out_bf16, out=out, acc="fast")
    assert got.data_ptr() == buf.data_ptr()
    want = c.expected("fast", n)
    assert ref.same_bits(_host(got), ref.bf16_bits(want) if out_bf16 else want)
    assert (buf[nnz:].contiguous().view(torch.int16).cpu().numpy().view(np.uint16) == SENTINEL).all(), "a store landed past the end of out"


def test_two_runs_have_the_same_bits_and_a_captured_graph_replays(patterns):
    c, a = ref.case("long"), patterns["long"]
    n = 40
    x, y = _dev_bits(c.x_bits[:, :n]), _dev_bits(c.y_bits[:, :n])
    first, second = _host(f(a, x, y, acc="fast")), _host(f(a, x, y, acc="fast"))
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    out32 = torch.zeros(a.nnz, dtype=torch.float32, device="cuda")
    out16 = torch.zeros(a.nnz, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        f(a, x, y, out=out32, acc="fast")                  # warm-up outside the capture
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            f(a, x, y, out=out32, acc="fast")
            f(a, x, y, out_bf16=True, out=out16, acc="reference")
    for _ in range(2):
        out32.zero_()
        out16.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert ref.same_bits(_host(out32), c.expected("fast", n))
        assert ref.same_bits(_host(out16), ref.bf16_bits(c.expected("reference", n)))


@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("out_dtype", ["bfloat16", "float32"])
def test_autograd_grad_values_through_the_bf16_kernel(out_dtype, acc):
    from mispmm import autograd
    c = ref.case("ragged")
    csr, n = c.csr, 40
    t = autograd.TrainableCSR.from_host(csr)
    bbits = c.y_bits[:, :n]
    gbits = c.x_bits[:, :n]                               # grad_C in bf16: what a float32 grad_C of these values rounds to, unchanged
    g = torch.from_numpy(ref.widen(gbits)).cuda()
    g = g.to(torch.bfloat16) if out_dtype == "bfloat16" else g
    grads = {}
    for path in ("bf16", "f32"):
        values = t.values.clone().requires_grad_(True)
        b = _dev_bits(bbits).view(torch.bfloat16).requires_grad_(True)
        autograd.spmm_bf16(t, values, b, out_dtype=getattr(torch, out_dtype), acc=acc, sddmm=path).backward(g)
        grads[path] = (values.grad, b.grad)
    got = grads["bf16"][0]
    assert got.dtype == torch.float32 and ref.same_bits(_host(got), c.expected(acc, n))
    if acc == "reference":
        assert ref.same_bits(_host(got), _host(grads["f32"][0]))
    assert grads["bf16"][1].dtype == torch.bfloat16
    assert ref.same_bits(_host(grads["bf16"][1].view(torch.int16)), _host(grads["f32"][1].view(torch.int16)))
    # only the gradient that is asked for: one launch of the side library, and none of the widenings
    # (the tag is the calling thread's: the backward is kept on this one)
    values = t.values.clone().requires_grad_(True)
    with torch.autograd.set_multithreading_enabled(False):
        out = autograd.spmm_bf16(t, values, _dev_bits(bbits).view(torch.bfloat16), out_dtype=getattr(torch, out_dtype), acc=acc, sddmm="bf16")
        out.backward(g)
        assert capi_sddmm_bf16.last_kernel() == ref.tag_of(acc, n), capi_sddmm_bf16.last_kernel()
    assert ref.same_bits(_host(values.grad), c.expected(acc, n))
