"""The row-list product with B in bf16 on the GPU (mispmm_rows_bf16 behind ops.spmm_csr_bf16 / spmm_coo_bf16 / spmm_ell_bf16 and
autograd.spmm_bf16).  Every parity check is BIT FOR BIT against the project's own oracles applied to the widened B
(tests/_spmm_bf16_ref.py): no tolerance anywhere.  A bf16 C hides the arithmetic (the CPU test measures how much), so the
arithmetic is judged on the fp32 C, and the bf16 C is held to the one rounding of the oracle's fp32 result."""
import dataclasses

import numpy as np
import pytest

import _fma_chain as fc
import _spmm_bf16_ref as ref
from mispmm import capi_bf16, datasets, formats, ops

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC1                      # int16 pairs of it make a quiet NaN in fp32 too: fills the slack of strided operands


def _dev_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


@pytest.fixture(scope="module")
def device_lists():
    """name -> DeviceCSR of the shared cases, uploaded once."""
    return {name: ops.DeviceCSR.from_host(ref.case(name).csr(), plan=False) for name in ("ragged", "n3c5-b6", "edges", "empty")}


def _check(c, a, n, mode, f=ops.spmm_csr_bf16, want_tag=None, **kw):
    """Both out types of one (list, width, arithmetic) against the oracle; returns the fp32 C."""
    acc, ref_sum = ref.OPS_ARGS[mode]
    if f is ops.spmm_csr_bf16:
        kw["ref_sum"] = ref_sum
    b = _dev_bits(c.b_bits[:, :n])
    want = c.expected(mode)[:, :n]
    got = _host(f(a, b, acc=acc, **kw))
    tag = capi_bf16.last_kernel()
    assert ref.head(tag) == (want_tag or ref.tag_of(mode, n)) and " f32 xcd " in tag, tag
    assert ref.same_bits(got, want), f"{c.name} N={n} {mode}: {int(np.sum(got.view(np.uint32) != want.view(np.uint32)))} of {want.size} elements differ"
    got16 = _host(f(a, b, out_bf16=True, acc=acc, **kw))
    tag = capi_bf16.last_kernel()
    assert ref.head(tag) == (want_tag or ref.tag_of(mode, n, out_bf16=True)) and " bf16 xcd " in tag, tag
    assert ref.same_bits(got16, ref.bf16_bits(want)), f"{c.name} N={n} {mode}: the bf16 C is not the rounded fp32 C"
    return got


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("n", ref.WIDTHS)
def test_every_instance_on_the_ragged_list(device_lists, n, mode):
    """Rows of 0-9 entries and of 300, 129, 77 and 40: chunk ends at every G, ring ends at 8, empty rows.  The widths reach
    every (G, V): with the three arithmetics every tag of the CPU table, each at its smallest shape."""
    c = ref.case("ragged")
    assert c.is_sharp(n)
    _check(c, device_lists["ragged"], n, mode)
    if n in ref.SMALLEST_N.values():
        assert ref.TAGS[ref.tag_of(mode, n)] == n


def test_the_widths_reach_every_tag_of_the_table():
    reached = {ref.tag_of(mode, n, out_bf16=o) for mode in ref.MODES for n in ref.WIDTHS for o in (False, True)}
    assert reached == set(ref.TAGS)


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("name", ["n3c5-b6", "edges", "empty"])
def test_uniform_rows_empty_rows_and_no_entries(device_lists, name, mode):
    c = ref.case(name)
    for n in (8, 36, 9, 72):
        assert c.is_sharp(n) or name == "empty"
        _check(c, device_lists[name], n, mode)


@pytest.mark.parametrize("mode", ref.MODES)
def test_the_uniform_list_with_and_without_row_pointers(device_lists, mode, monkeypatch):
    c, a = ref.case("n3c5-b6"), device_lists["n3c5-b6"]
    assert a.uniform_row_nnz == 7 and c.is_sharp(17)
    acc, ref_sum = ref.OPS_ARGS[mode]
    outs = []
    for hint in (True, False):
        if not hint:
            monkeypatch.setenv("MISPMM_NO_HINT", "1")
        # what reaches the library: a null rowPtrs with the hint, the array without
        seen = {}
        monkeypatch.setattr(ops, "_p", lambda t, _p=ops._p: seen.setdefault("ptrs", []).append(t is None) or _p(t))
        for n in (136, 68, 17):
            outs.append((n, _check(c, a, n, mode)))
        monkeypatch.undo()
        assert any(seen["ptrs"]) == hint
    for (n, x), (_, y) in zip(outs[:3], outs[3:]):
        assert ref.same_bits(x, y), n


def _strided(host_bits, ld, offset=0):
    """bf16 bits [rows, n] on the device, rows ld apart, the first element `offset` elements into a 16-byte aligned buffer;
    the slack holds the sentinel."""
    rows, n = host_bits.shape
    buf = torch.full((offset + rows * ld,), SENTINEL, dtype=torch.int16, device="cuda")
    view = buf[offset:].view(rows, ld)[:, :n]
    view.copy_(_dev_bits(host_bits))
    return buf, view


@pytest.mark.parametrize("mode", ref.MODES)
def test_leading_dimensions_offsets_and_the_slack_of_c(device_lists, mode):
    c, a = ref.case("ragged"), device_lists["ragged"]
    acc, ref_sum = ref.OPS_ARGS[mode]
    m, k = c.num_rows, c.num_cols
    # (N, ldb, ldc fp32, ldc bf16, B offset, expected V fp32 C, expected V bf16 C)
    rows = [(72, 88, 76, 80, 0, 8, 8),          # ldc % 4 is enough for an fp32 C at V8; a bf16 C wants % 8
            (72, 88, 76, 76, 0, 8, 4),          # ... and falls to 8-byte lanes without
            (72, 72, 72, 72, 8, 8, 8),          # B 16 bytes into its buffer: still V8
            (72, 72, 72, 72, 4, 4, 4),          # 8 bytes: V4
            (72, 72, 72, 72, 1, 1, 1),          # 2 bytes: V1, same bits
            (36, 44, 38, 40, 0, 4, 4),
            (33, 35, 37, 39, 3, 1, 1),
            (72, 73, 72, 72, 0, 1, 1)]          # an odd ldb alone
    assert c.is_sharp(72) and c.is_sharp(36) and c.is_sharp(33)
    for n, ldb, ldc32, ldc16, off, v32, v16 in rows:
        _, b = _strided(c.b_bits[:, :n], ldb, off)
        want = c.expected(mode)[:, :n]
        for out_bf16, ldc, v in ((False, ldc32, v32), (True, ldc16, v16)):
            dtype = torch.int16 if out_bf16 else torch.float32
            buf = torch.full((m, ldc), SENTINEL, dtype=torch.int16, device="cuda") if out_bf16 else \
                torch.full((m, ldc * 2), SENTINEL, dtype=torch.int16, device="cuda").view(torch.float32)
            assert buf.dtype == dtype and buf.shape == (m, ldc)
            out = ops.spmm_csr_bf16(a, b, out_bf16=out_bf16, out=buf[:, :n], acc=acc, ref_sum=ref_sum)
            assert out.data_ptr() == buf.data_ptr()
            tag = capi_bf16.last_kernel()
            assert f",V{v}," in tag, (tag, n, ldb, ldc, off)
            assert ref.same_bits(_host(out), ref.bf16_bits(want) if out_bf16 else want), (tag, n, ldb, ldc, off)
            slack = buf[:, n:].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
            assert (slack == SENTINEL).all(), f"a store landed in the slack of C ({tag})"


SPECIAL_BITS = [0x7FC0, 0xFFC1, 0x7F80, 0xFF80, 0x8000, 0x0000, 0x0001, 0x807F, 0x0080, 0x7F7F, 0xFF7F, 0x3F80]
#               NaN     -NaN    +Inf    -Inf    -0      +0      subnormals      min normal, largest finite +-, 1


@pytest.mark.parametrize("mode", ref.MODES)
def test_special_values_of_b_and_of_the_values(mode):
    """NaN, +-Inf, -0, bf16 subnormals and the largest finite value in B; Inf and -0 among A's values.  Bit for bit with the
    oracle, NaNs compared as NaNs: nothing is flushed, -0 * x and Inf * 0 follow IEEE."""
    c = ref.case("edges")
    rng = np.random.default_rng(21)
    vals = c.vals.copy()
    vals[rng.choice(vals.shape[0], 12, replace=False)] = np.array([np.inf, -np.inf, -0.0, 0.0] * 3, np.float32)
    bits = c.b_bits[:, :40].copy()
    at = rng.random(bits.shape) < 0.08
    bits[at] = rng.choice(np.array(SPECIAL_BITS, np.uint16), int(at.sum()))
    acc, ref_sum = ref.OPS_ARGS[mode]
    a = ops.DeviceCSR.from_host(dataclasses.replace(c.csr(), data=vals), plan=False)
    want = ref.expected(mode, c.row_ptrs, c.col_idxs, vals, bits)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    for n in (40, 36, 33):
        b = _dev_bits(bits[:, :n])
        assert ref.same_bits(_host(ops.spmm_csr_bf16(a, b, acc=acc, ref_sum=ref_sum)), want[:, :n]), n
        assert ref.same_bits(_host(ops.spmm_csr_bf16(a, b, out_bf16=True, acc=acc, ref_sum=ref_sum)), ref.bf16_bits(want[:, :n])), n
    # subnormal products and sums survive: a B of subnormals alone, values around 1
    tiny = rng.integers(1, 0x80, size=(c.num_cols, 8)).astype(np.uint16) | (rng.integers(0, 2, size=(c.num_cols, 8)).astype(np.uint16) << 15)
    want = ref.expected(mode, c.row_ptrs, c.col_idxs, c.vals, tiny)
    assert (want != 0).mean() > 0.8 and np.all(np.abs(want) < 2.0 ** -110)
    a = ops.DeviceCSR.from_host(c.csr(), plan=False)
    assert ref.same_bits(_host(ops.spmm_csr_bf16(a, _dev_bits(tiny), acc=acc, ref_sum=ref_sum)), want)


@pytest.mark.parametrize("mode", ["fast", "ref32"])
def test_a_padded_ell_whose_padding_values_are_nan(mode):
    """The padded arrays as a uniform list: a padding slot is known by its column index, and a NaN or an Inf in its value
    contributes +0 (the dropped load's 0 times an Inf would be a NaN)."""
    c = ref.case("edges")
    ell = formats.csr_to_ell_rowmajor(c.csr())
    pad = np.asarray(ell.col_idxs) == formats.ELL_PAD
    data = np.asarray(ell.data, np.float32).copy()
    data[pad] = np.where(np.arange(int(pad.sum())) % 2 == 0, np.nan, np.inf).astype(np.float32)
    assert pad.mean() > 0.25
    a = ops.DeviceELL.from_host(dataclasses.replace(ell, data=data), compact=False)
    assert a.compact is None and a.width == ell.width
    acc = ref.OPS_ARGS[mode][0]
    for n in (72, 36, 9):
        assert c.is_sharp(n)
        got = _host(ops.spmm_ell_bf16(a, _dev_bits(c.b_bits[:, :n]), acc=acc))
        assert not np.isnan(got).any() and not np.isinf(got).any()
        assert ref.same_bits(got, c.expected(mode)[:, :n]), n
        assert ref.same_bits(got, ref.expected(mode, None, ell.col_idxs, data, c.b_bits[:, :n], row_nnz=ell.width))
    # the same ELL uploaded with its list of occupied slots
    listed = ops.DeviceELL.from_host(ell, compact=True)
    assert listed.compact is not None
    _check(c, listed, 72, mode, f=ops.spmm_ell_bf16)


@pytest.mark.parametrize("mode", ["fast", "ref32"])
def test_coo_unsorted_with_duplicates_ell_colmajor_and_the_bsr_list(mode):
    acc = ref.OPS_ARGS[mode][0]
    c = ref.case("ragged")
    rng = np.random.default_rng(31)
    csr = c.csr()
    # COO: the entries shuffled, 60 of them repeated with other values
    coo = formats.csr_to_coo(csr)
    extra = rng.choice(coo.row_idxs.shape[0], 60, replace=False)
    rows = np.concatenate([coo.row_idxs, coo.row_idxs[extra]])
    cols = np.concatenate([coo.col_idxs, coo.col_idxs[extra]])
    data = np.concatenate([coo.data, fc.sharp_values(rng, 60, np.float32)])
    order = rng.permutation(rows.shape[0])
    coo = formats.COO(csr.num_rows, csr.num_cols, rows[order], cols[order], data[order])
    a = ops.DeviceCOO.from_host(coo)
    assert a.row_bounds is None
    for n in (72, 36, 17):
        b = c.b_bits[:, :n]
        rp, ci, va = fc.coo_rows(coo)
        assert fc.corpus_is_sharp((rp, ci, va), ref.widen(b))
        got = _host(ops.spmm_coo_bf16(a, _dev_bits(b), acc=acc))
        assert ref.same_bits(got, ref.expected(mode, rp, ci, va, b)), ("coo", n)
        assert ref.same_bits(_host(ops.spmm_coo_bf16(a, _dev_bits(b), out_bf16=True, acc=acc)), ref.bf16_bits(ref.expected(mode, rp, ci, va, b)))
    assert a.row_bounds is not None and np.array_equal(a.row_bounds.cpu().numpy().view(np.uint32), fc.coo_rows(coo)[0])
    # ELL, column-major as formats makes it: the order of addition is ascending column, then slot
    u = ref.case("n3c5-b6")
    ell = formats.csr_to_ell_colmajor(u.csr())
    rp, ci, va = fc.ell_colmajor_rows(ell)
    a = ops.DeviceELL.from_host(ell)
    for n in (72, 9):
        b = u.b_bits[:, :n]
        assert fc.corpus_is_sharp((rp, ci, va), ref.widen(b))
        assert ref.same_bits(_host(ops.spmm_ell_bf16(a, _dev_bits(b), acc=acc)), ref.expected(mode, rp, ci, va, b)), ("ell", n)
    # the non-zero list of a BSR of 2 x 2 blocks: fp32 sums (ref_sum="f32"), the explicit zeros of the blocks dropped
    bsr = formats.csr_to_bsr(u.csr(), 2)
    rp, ci, va = fc.bsr_rows(bsr, skip_zeros=True)
    nz = ops.bsr_nonzeros(bsr)
    for n in (72, 9):
        b = u.b_bits[:, :n]
        assert fc.corpus_is_sharp((rp, ci, va), ref.widen(b))
        assert ref.same_bits(_host(ops.spmm_csr_bf16(nz, _dev_bits(b), acc=acc, ref_sum="f32")), ref.expected(mode, rp, ci, va, b)), ("bsr", n)


def test_graph_capture_and_two_replays(device_lists):
    c, a = ref.case("ragged"), device_lists["ragged"]
    n = 136
    assert c.is_sharp(n)
    b = _dev_bits(c.b_bits[:, :n])
    out32 = torch.zeros((c.num_rows, n), dtype=torch.float32, device="cuda")
    out16 = torch.zeros((c.num_rows, n), dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        ops.spmm_csr_bf16(a, b, out=out32, acc="fast")                  # warm-up outside the capture
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            ops.spmm_csr_bf16(a, b, out=out32, acc="fast")
            ops.spmm_csr_bf16(a, b, out_bf16=True, out=out16, acc="reference", ref_sum="f32")
    for _ in range(2):
        out32.zero_()
        out16.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert ref.same_bits(_host(out32), c.expected("fast")[:, :n])
        assert ref.same_bits(_host(out16), ref.bf16_bits(c.expected("ref32")[:, :n]))


@pytest.mark.parametrize("acc", ["fast", "reference"])
@pytest.mark.parametrize("out_dtype", ["bfloat16", "float32"])
def test_autograd_both_gradients_are_the_composition_through_the_oracle(out_dtype, acc):
    from mispmm import autograd
    c = ref.case("ragged")
    csr = c.csr()
    n = 40
    mode = "fast" if acc == "fast" else "ref64"
    t = autograd.TrainableCSR.from_host(csr)
    values = t.values.clone().requires_grad_(True)
    bbits = c.b_bits[:, :n]
    b = _dev_bits(bbits).view(torch.bfloat16).requires_grad_(True)
    out = autograd.spmm_bf16(t, values, b, out_dtype=getattr(torch, out_dtype), acc=acc)
    fwd = c.expected(mode)[:, :n]
    if out_dtype == "bfloat16":
        assert ref.same_bits(_host(out.detach().view(torch.int16)), ref.bf16_bits(fwd))
    else:
        assert ref.same_bits(_host(out.detach()), fwd)
    rng = np.random.default_rng(41)
    grad = fc.sharp_values(rng, (c.num_rows, n), np.float32)            # full mantissas: the rounding to bf16 is visible
    gbits = ref.bf16_bits(grad)
    assert (ref.widen(gbits) != grad).mean() > 0.9
    g = torch.from_numpy(grad).cuda()
    out.backward(g.to(torch.bfloat16) if out_dtype == "bfloat16" else g)
    # grad_b: the same kernel on A^T's pattern with values[perm], on grad_C rounded once to bf16; back in bf16
    t_csr, perm = ops.csr_transpose(csr)
    t_rows = (t_csr.row_ptrs, t_csr.col_idxs, np.asarray(csr.data, np.float32)[perm])
    assert fc.corpus_is_sharp(t_rows, ref.widen(gbits))
    want_b = ref.bf16_bits(ref.expected(mode, *t_rows, gbits))
    assert b.grad.dtype == torch.bfloat16 and ref.same_bits(_host(b.grad.view(torch.int16)), want_b)
    # grad_values: ops.sddmm_csr (an existing kernel, held by its own tests) on the two operands widened by the reference
    want_v = ops.sddmm_csr(t.fwd, torch.from_numpy(ref.widen(gbits)).cuda(), torch.from_numpy(ref.widen(bbits)).cuda(), acc=acc)
    assert values.grad.dtype == torch.float32 and ref.same_bits(_host(values.grad), _host(want_v))
    from _sddmm_ref import assert_within, sddmm_exact
    exact, scale = sddmm_exact(csr.row_ptrs, csr.col_idxs, ref.widen(gbits), ref.widen(bbits))
    assert_within(_host(values.grad), np.float32, acc, n, exact, scale, f"grad_values {acc}")
    # only the gradients that are asked for
    b2 = b.detach().clone().requires_grad_(True)
    autograd.spmm_bf16(t, values.detach(), b2, out_dtype=getattr(torch, out_dtype), acc=acc).backward(g.to(getattr(torch, out_dtype)))
    assert ref.same_bits(_host(b2.grad.view(torch.int16)), want_b)


@pytest.mark.parametrize("mode", ["fast", "ref64"])
def test_full_size_n4c6_b13_at_128_columns(mode):
    """6300 x 25605, 14 entries in every row, N = 128 (G16, V8; 8 XCD parts): FAST and REFERENCE against the oracle, with and
    without the row pointers."""
    csr = datasets.load_csr("n4c6-b13")
    c = ref.Case("n4c6-b13", csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, max_n=128)
    n = 128
    b = c.b_bits[:, :n]
    want = ref.expected(mode, *c.rows, b)
    acc, ref_sum = ref.OPS_ARGS[mode]
    a = ops.DeviceCSR.from_host(c.csr(), plan=False, spans=False)
    assert a.uniform_row_nnz == 14
    got = _host(ops.spmm_csr_bf16(a, _dev_bits(b), acc=acc, ref_sum=ref_sum))
    assert capi_bf16.last_kernel() == f"rows_bf16<G16,V8,{mode}> f32 xcd 8x1"
    assert ref.same_bits(got, want)
    listed = dataclasses.replace(a, uniform_row_nnz=0)
    assert ref.same_bits(_host(ops.spmm_csr_bf16(listed, _dev_bits(b), acc=acc, ref_sum=ref_sum)), want)
    got16 = _host(ops.spmm_csr_bf16(a, _dev_bits(b), out_bf16=True, acc=acc, ref_sum=ref_sum))
    assert capi_bf16.last_kernel() == f"rows_bf16<G16,V8,{mode}> bf16 xcd 8x1"
    assert ref.same_bits(got16, ref.bf16_bits(want))
