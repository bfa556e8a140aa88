"""The adversarial corpus (tests/_adversarial.py) through every REFERENCE-mode entry point, compared BIT FOR BIT with the
oracle (tests/_bits.py: -0 is not +0, a NaN is required wherever the oracle has one).  Every B sits in a wider buffer whose
gap columns are NaN, every C in one whose gap columns hold a sentinel NaN that must survive; in the poisoned cases the A
arrays are views of longer device buffers whose tails hold NaN values and the index of a poisoned B row.

The FAST and bf16 / MFMA paths are held to what their contracts allow on such data: the NaN / Inf positions of the
reference (nothing leaks from a poisoned operand) and no -0 where the reference has +0.

A test walks every case and every variant of its path, collects the differences and fails once with all of them."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mispmm import capi, formats, ops, synth  # noqa: E402

import _adversarial as adv  # noqa: E402
from _bits import assert_gap_untouched, assert_no_leak, assert_same_bits, sentinel_buffer  # noqa: E402

pytestmark = pytest.mark.gpu
GAP = 4                    # extra columns of every B and C buffer (keeps 16-byte rows for N a multiple of 4)
CASES = adv.corpus()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs a GPU"
    assert os.path.exists(capi.LIB_PATH), "libmispmm.so must be built (no fallback path exists)"
    capi.lib()


def b_dev(b):
    """B inside a [K, N + GAP] buffer whose gap columns are NaN."""
    k, n = b.shape
    buf = torch.full((k, n + GAP), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    return buf[:, :n]


def tail(t, fill, extra=37):
    """t as the first t.numel() elements of a longer device buffer whose tail holds `fill`."""
    buf = torch.empty(t.numel() + extra, dtype=t.dtype, device=t.device)
    buf[t.numel():] = fill
    buf[:t.numel()].copy_(t)
    return buf[:t.numel()]


def poison_tails(case, obj, cols="col_idxs", vals="data"):
    """In a poisoned case: the index array's tail names a poisoned (in-range) B row, the value array's tail is NaN."""
    if case.poison is not None:
        setattr(obj, cols, tail(getattr(obj, cols), int(case.poison_cols[0])))
        setattr(obj, vals, tail(getattr(obj, vals), float("nan")))
    return obj


class Check:
    """Runs products into sentinel-filled strided C buffers and collects every difference from the expected bits."""

    def __init__(self):
        self.errors = []

    def out(self, m, n):
        self.buf = sentinel_buffer(m, n, n + GAP, torch)
        return self.buf[:, :n]

    def bits(self, got, want, what):
        try:
            assert_same_bits(got, want, what)
            if got.data_ptr() == self.buf.data_ptr():
                assert_gap_untouched(self.buf, want.shape[1], what)
        except AssertionError as e:
            self.errors.append(str(e))

    def leak(self, got, want, what):
        try:
            assert_no_leak(got, want, what)
        except AssertionError as e:
            self.errors.append(str(e))

    def done(self):
        assert not self.errors, f"{len(self.errors)} differences:\n" + "\n".join(self.errors[:40])


def ref64(oracle, case, b=None):
    c = case.csr
    return oracle.spmm_csr(c.row_ptrs, c.col_idxs, c.data, case.b if b is None else b)


def ref32(oracle, case, b=None):
    coo = formats.csr_to_coo(case.csr)
    return oracle.spmm_coo(coo.num_rows, coo.row_idxs, coo.col_idxs, coo.data, case.b if b is None else b)


# ----------------------------------------------------------------------------------------------------------------- CSR
def test_csr_kernels_in_row_order(oracle):
    """mispmm_csr_f32 kernels 0..6 on the rows in row order, the uniform entry point where the rows have one width, and the
    general entry point (use_hint=False)."""
    chk = Check()
    for case in CASES:
        m, n = case.csr.num_rows, case.b.shape[1]
        want = ref64(oracle, case)
        a = poison_tails(case, ops.DeviceCSR.from_host(case.csr, spans=False, plan=False))
        assert bool(a.uniform_row_nnz) == ("uniform" in case.tags)
        bd = b_dev(case.b)
        for k in range(7):
            chk.bits(ops.spmm_csr(a, bd, out=chk.out(m, n), kernel=k), want, f"{case.name} kernel {k} ({capi.last_kernel()})")
        chk.bits(ops.spmm_csr(a, bd, out=chk.out(m, n), use_hint=False), want, f"{case.name} general entry ({capi.last_kernel()})")
    chk.done()


@pytest.mark.parametrize("share_len", [0, 8, 30])
def test_csr_split_and_two_body_launch(oracle, share_len):
    """The split kernel walking a span list (rows longest first, rows above share_len dealt to the 4 waves of a workgroup)
    and the two-body launch (rows of more than 32 entries by the split body, the others by the row-gather body)."""
    chk = Check()
    hybrids = 0
    for case in CASES:
        m, n = case.csr.num_rows, case.b.shape[1]
        want = ref64(oracle, case)
        a = poison_tails(case, ops.DeviceCSR.from_host(case.csr, spans=True, share_len=share_len, plan=False))
        bd = b_dev(case.b)
        chk.bits(ops.spmm_csr(a, bd, out=chk.out(m, n), kernel=6), want, f"{case.name} split, share_len {share_len} ({capi.last_kernel()})")
        chk.bits(ops.spmm_csr(a, bd, out=chk.out(m, n), kernel=0), want, f"{case.name} kernel 0 with spans ({capi.last_kernel()})")
        hybrids += "csr_hybrid" in capi.last_kernel()
    chk.done()
    assert hybrids >= 4, f"only {hybrids} cases took the two-body launch"


def test_csr_plan_order_single_and_batched(oracle):
    """Rows in a clustered plan order (mispmm_csr_plan_f32).  The row-mapped kernel declines long rows on average (24 entries
    or more): those cases are multiplied from the unpermuted arrays by the other tests."""
    chk = Check()
    taken = 0
    for case in CASES:
        m, n = case.csr.num_rows, case.b.shape[1]
        want = ref64(oracle, case)
        a = ops.DeviceCSR.from_host(case.csr, plan=True, spans=False)
        poison_tails(case, a.plan)
        bd = b_dev(case.b)
        c = chk.out(m, n)
        if not ops._csr_plan(a, [bd], [c], "reference", None):
            assert case.csr.nnz // m >= 24 and not a.uniform_row_nnz, f"{case.name}: plan order declined"
            continue
        taken += 1
        chk.bits(c, want, f"{case.name} plan order ({capi.last_kernel()})")
        outs = [sentinel_buffer(m, n, n + GAP, torch)[:, :n] for _ in range(2)]
        b2 = (case.b * np.float32(2)).astype(np.float32)
        assert ops._csr_plan(a, [bd, b_dev(b2)], outs, "reference", None), case.name
        chk.bits(outs[0], want, f"{case.name} batched plan order [0]")
        chk.bits(outs[1], ref64(oracle, case, b2), f"{case.name} batched plan order [1]")
    chk.done()
    assert taken >= 7, taken


def test_csr_batch(oracle):
    chk = Check()
    for case in CASES:
        m, n = case.csr.num_rows, case.b.shape[1]
        b2 = (-case.b).astype(np.float32)
        a = poison_tails(case, ops.DeviceCSR.from_host(case.csr, spans=False, plan=False))
        outs = [chk.out(m, n), sentinel_buffer(m, n, n + GAP, torch)[:, :n]]
        ops.spmm_csr_batch(a, [b_dev(case.b), b_dev(b2)], outs=outs)
        chk.bits(outs[0], ref64(oracle, case), f"{case.name} batch [0] ({capi.last_kernel()})")
        chk.bits(outs[1], ref64(oracle, case, b2), f"{case.name} batch [1]")
    chk.done()


def test_csr_lds_tiles(oracle):
    chk = Check()
    ran = 0
    for case in CASES:
        w = case.uniform_width
        if not w or w > 16:
            continue
        m, n = case.csr.num_rows, case.b.shape[1]
        a = ops.DeviceCSRTiles.from_host(case.csr)
        if case.poison is not None:
            a.data = tail(a.data, float("nan"))
        chk.bits(ops.spmm_csr_tiles(a, b_dev(case.b), out=chk.out(m, n)), ref64(oracle, case), f"{case.name} LDS tiles ({capi.last_kernel()})")
        ran += 1
    chk.done()
    assert ran >= 3


def test_csr_lds_tiles_decline_tiles_wider_than_the_lds_image(oracle):
    """Tiles of more than MISPMM_LDS_TILE_COLS (128) columns are declined with MISPMM_ERR_UNSUPPORTED (the kernel stages 128
    list positions only); tiles built within the limit keep the oracle's bits.  The kernel is never run on a wider tile."""
    from mispmm import datasets
    csr = datasets.load_csr("n4c6-b13")
    b = synth.dense_b(csr.num_cols, 128)
    wide = ops.DeviceCSRTiles.from_host(csr, max_cols=256)
    assert wide.max_tile_cols > 128
    with pytest.raises(capi.MispmmError):
        ops.spmm_csr_tiles(wide, b_dev(b))
    ok = ops.DeviceCSRTiles.from_host(csr, max_cols=128)
    assert 0 < ok.max_tile_cols <= 128
    c = sentinel_buffer(csr.num_rows, 128, 128 + GAP, torch)
    ops.spmm_csr_tiles(ok, b_dev(b), out=c[:, :128])
    assert_same_bits(c[:, :128], oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, b), "LDS tiles, 128 columns")
    assert_gap_untouched(c, 128, "LDS tiles, 128 columns")


# ------------------------------------------------------------------------------------------------- COO, ELL, row lists
def test_coo_storage_order_and_workspace(oracle):
    """spmm_coo with and without the row-bounds workspace, on the COO in CSR order and on a shuffled COO (rows interleaved,
    a row's entries in a new order): fp32 sums in storage order."""
    chk = Check()
    for case in CASES:
        m, n = case.csr.num_rows, case.b.shape[1]
        bd = b_dev(case.b)
        for tag, coo in (("csr order", formats.csr_to_coo(case.csr)), ("shuffled", adv.coo_shuffled(case.csr, seed=len(case.name)))):
            want = oracle.spmm_coo(coo.num_rows, coo.row_idxs, coo.col_idxs, coo.data, case.b)
            a = poison_tails(case, ops.DeviceCOO.from_host(coo))
            if case.poison is not None:
                a.row_idxs = tail(a.row_idxs, m - 1)
            for ws in (True, False):
                chk.bits(ops.spmm_coo(a, bd, out=chk.out(m, n), workspace=ws), want, f"{case.name} COO {tag} workspace={ws} ({capi.last_kernel()})")
    chk.done()


def test_rows_split_and_two_body_on_row_lists(oracle):
    """mispmm_rows_split_f32 and mispmm_rows_hybrid_f32 (the long-row shapes of COO / ELL / BSR lists, fp32 sums) on every
    case, whatever its row lengths."""
    chk = Check()
    for case in CASES:
        m, n = case.csr.num_rows, case.b.shape[1]
        want = ref32(oracle, case)
        a = poison_tails(case, ops.DeviceCOO.from_host(formats.csr_to_coo(case.csr)))
        host = ops.csr_spans_by_length(case.csr.row_ptrs, 0xFFFFFFFF)
        spans = ops._dev_u32(host.reshape(-1), "cuda")
        bd = b_dev(case.b)
        for tag, rs in (("split", ops.RowSpans(spans, 0, False)), ("two-body", ops.RowSpans(spans, ops.spans_long_count(host), False))):
            c = chk.out(m, n)
            assert ops._rows_split(rs, m, case.csr.num_cols, a.nnz, a.col_idxs, a.data, bd, c, "reference", None), (case.name, tag)
            chk.bits(c, want, f"{case.name} rows {tag} ({capi.last_kernel()})")
    chk.done()


def test_ell_row_major_compact_and_column_major(oracle):
    chk = Check()
    for case in CASES:
        m, n = case.csr.num_rows, case.b.shape[1]
        bd = b_dev(case.b)
        ell = formats.csr_to_ell_rowmajor(case.csr)
        for compact in (False, True):
            a = ops.DeviceELL.from_host(ell, compact=compact)
            chk.bits(ops.spmm_ell(a, bd, out=chk.out(m, n)), ref32(oracle, case), f"{case.name} ELL row-major compact={compact} ({capi.last_kernel()})")
        ellc = formats.csr_to_ell_colmajor(case.csr)
        want = oracle.spmm_ell_colmajor(m, ellc.row_idxs, ellc.data, case.b)
        chk.bits(ops.spmm_ell(ops.DeviceELL.from_host(ellc), bd, out=chk.out(m, n)), want, f"{case.name} ELL column-major ({capi.last_kernel()})")
    chk.done()


# ----------------------------------------------------------------------------------------------------------------- BSR
BSR_CASES = [c for c in CASES if not c.has_duplicates]      # a BSR holds one value per position


@pytest.mark.parametrize("br,bc", adv.BLOCK_SHAPES)
def test_bsr_kernel1(oracle, br, bc):
    chk = Check()
    for case in BSR_CASES:
        bsr, b = adv.bsr_of(case, br, bc)
        m, n = bsr.num_rows, b.shape[1]
        want = oracle.spmm_bsr(m, br, bc, bsr.block_row_ptrs, bsr.block_col_idxs, bsr.data, b)
        chk.bits(ops.spmm_bsr(ops.DeviceBSR.from_host(bsr), b_dev(b), out=chk.out(m, n), kernel=1), want,
                 f"{case.name} BSR {br}x{bc} kernel 1 ({capi.last_kernel()})")
    chk.done()


@pytest.mark.parametrize("br,bc", [(1, 1), (4, 4), (16, 16), (32, 32), (2, 4), (16, 8)])
def test_bsr_nonzeros_under_its_rule(oracle, br, bc):
    """The zero-skipping path: the reference's fp32 sums over the NON-ZERO block entries in the reference's order (DESIGN.md:
    a skipped 0 * b would add +-0, except that 0 * Inf = NaN is not formed)."""
    chk = Check()
    for case in BSR_CASES:
        bsr, b = adv.bsr_of(case, br, bc)
        m, n = bsr.num_rows, b.shape[1]
        rows, cols, vals = adv.bsr_entries(bsr, nonzero_only=True)
        want = oracle.spmm_coo(m, rows, cols, vals, b)
        nz = poison_tails(case, ops.bsr_nonzeros(bsr))
        chk.bits(ops.spmm_bsr_nonzeros(nz, b_dev(b), out=chk.out(m, n)), want, f"{case.name} BSR {br}x{bc} non-zeros ({capi.last_kernel()})")
    chk.done()


# -------------------------------------------------------------------------------------------------- one-card drivers
def test_one_card_slot_drivers(oracle):
    from mispmm.multi import MultiCsrSpmm, MultiEllSpmm
    case = next(c for c in CASES if c.name == "poisoned_nan")
    n = case.b.shape[1]
    job = MultiCsrSpmm(case.csr, n, [0], gather="first")
    job.set_b(case.b)
    job.step()
    job.sync()
    assert_same_bits(job.full_c(0), ref64(oracle, case), "MultiCsrSpmm")
    job.close()
    case = next(c for c in CASES if c.name == "order")
    ellc = formats.csr_to_ell_colmajor(case.csr)
    job = MultiEllSpmm(ellc, n, [0], gather="first")
    job.set_b(case.b)
    job.step()
    job.sync()
    assert_same_bits(job.full_c(0), oracle.spmm_ell_colmajor(case.csr.num_rows, ellc.row_idxs, ellc.data, case.b), "MultiEllSpmm")
    job.close()


# ------------------------------------------------------------------------------------------ FAST and bf16 / MFMA paths
LEAK_CASES = [c for c in CASES if c.poison is not None or "zero" in c.tags]


def test_fast_paths_leak_nothing(oracle):
    chk = Check()
    for case in LEAK_CASES:
        m, n = case.csr.num_rows, case.b.shape[1]
        bd = b_dev(case.b)
        w64, w32 = ref64(oracle, case), ref32(oracle, case)
        a = poison_tails(case, ops.DeviceCSR.from_host(case.csr, spans=False, plan=False))
        for k in (0, 1, 5):
            chk.leak(ops.spmm_csr(a, bd, out=chk.out(m, n), kernel=k, acc="fast"), w64, f"{case.name} CSR kernel {k} fast")
        s = poison_tails(case, ops.DeviceCSR.from_host(case.csr, spans=True, plan=False))
        chk.leak(ops.spmm_csr(s, bd, out=chk.out(m, n), kernel=6, acc="fast"), w64, f"{case.name} CSR split fast")
        chk.leak(ops.spmm_csr(s, bd, out=chk.out(m, n), acc="fast"), w64, f"{case.name} CSR kernel 0 spans fast ({capi.last_kernel()})")
        coo = poison_tails(case, ops.DeviceCOO.from_host(formats.csr_to_coo(case.csr)))
        chk.leak(ops.spmm_coo(coo, bd, out=chk.out(m, n), acc="fast"), w32, f"{case.name} COO fast")
        chk.leak(ops.spmm_ell(ops.DeviceELL.from_host(formats.csr_to_ell_rowmajor(case.csr)), bd, out=chk.out(m, n), acc="fast"), w32,
                 f"{case.name} ELL fast")
    chk.done()


def bf16_dev(b):
    """bf16 bits of B in a [K, N + 8] buffer whose gap columns are NaN."""
    k, n = b.shape
    buf = torch.full((k, n + 8), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    return ops.f32_to_bf16(buf)[:, :n]


def test_mfma_and_bf16_paths_leak_nothing(oracle):
    """fp32 MFMA BSR (kernel 2), bf16 BSR, and the column-compacted bf16 block rows (wave and workgroup per block row):
    NaN / Inf where the oracle on bf16-rounded operands has them, nowhere else, and no -0 for +0."""
    chk = Check()
    for case in LEAK_CASES:
        for br, bc in ((16, 16), (32, 32), (16, 8)):
            bsr, b = adv.bsr_of(case, br, bc)
            m, n = bsr.num_rows, b.shape[1]
            a = ops.DeviceBSR.from_host(bsr)
            if br == bc == 16:
                want = oracle.spmm_bsr(m, br, bc, bsr.block_row_ptrs, bsr.block_col_idxs, bsr.data, b)
                chk.leak(ops.spmm_bsr(a, b_dev(b), out=chk.out(m, n), kernel=2, acc="fast"), want, f"{case.name} BSR {br}x{bc} MFMA fp32")
            a16 = synth.bf16_round(bsr.data.reshape(-1)).reshape(bsr.data.shape)
            b16 = synth.bf16_round(b.reshape(-1)).reshape(b.shape)
            want = oracle.spmm_bsr(m, br, bc, bsr.block_row_ptrs, bsr.block_col_idxs, a16, b16)
            bb = bf16_dev(b)
            if br == bc:
                chk.leak(ops.spmm_bsr_bf16(a, ops.f32_to_bf16(a.data), bb), want, f"{case.name} BSR {br}x{bc} bf16")
            if br == 16:
                chk.leak(ops.spmm_bsrc_bf16(ops.DeviceBSRC.from_host(bsr), bb), want, f"{case.name} bsrc {br}x{bc}")
                chk.leak(ops.spmm_bsrc_slots_bf16(ops.DeviceBSRCSlots.from_host(bsr), bb), want, f"{case.name} bsrc_slots {br}x{bc}")
    chk.done()
