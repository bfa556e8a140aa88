"""FAST mode held to its written contract (include/mispmm.h enum mispmm_acc_mode), bit for bit: every
single-chain path must return oracle.rows_fma -- acc = +0, one fma per entry in the format's list order -- on data where an
unfused kernel, a reordered row, a sum started elsewhere or a partial sum through another width each change the bits
(tests/_fma_chain.py: sharp_values, corpus_is_sharp; the CPU half of that precondition is tests/test_fma_chain_cpu.py).
The paths that promise a fixed order but not the storage-order chain (kernel 6 and the launches built on it: tags csr_split,
csr_hybrid) are held to the derived any-order bound gamma_L * sum|a||b| and to run-to-run identity; the rows a two-body
launch hands to its row-gather body are single chains again and are compared bitwise.  Every case asserts the kernel family
in capi.last_kernel(), so a re-dispatch cannot satisfy a test through another kernel.

The 1e-5 * sum|a||b| assertions of the other GPU files stay where they are; nothing here replaces them."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mispmm import capi, formats, ops  # noqa: E402

import _fast_corpus as corpus  # noqa: E402
import _fma_chain as fc  # noqa: E402
from _bits import assert_same_bits  # noqa: E402
from _ref64 import assert_same_bits64  # noqa: E402

pytestmark = pytest.mark.gpu
SCALE = int(os.environ.get("MISPMM_FUZZ_SCALE", "1"))

SINGLE = ("csr_k1<", "csr_k2<", "csr_k3<", "csr_wave_deep<", "row_gather<", "row_stream<", "coo_k1<", "csr_lds_tile<", "csr_panel<",
          "bsr_valu<", "bsr_rowblock<", "csr_f64<")
SPLIT = ("csr_split<", "csr_hybrid<")
SEEN = {}                                   # path -> kernel tags observed (printed by the last test)
TALLY = {"bitwise": 0, "bounded": 0, "fuzz_bitwise": 0, "fuzz_bounded": 0, "fuzz_cases": 0}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs a GPU"
    assert os.path.exists(capi.LIB_PATH), "libmispmm.so must be built (no fallback path exists)"
    capi.lib()


@pytest.fixture(scope="module")
def mats():
    """The corpus, built once."""
    m = {f"uniform{w}": corpus.uniform(w) for w in corpus.UNIFORM_WIDTHS}
    m.update(ragged=corpus.ragged(), long_tail=corpus.long_tail(), long_mean=corpus.long_mean(), long_only=corpus.long_only(),
             dense=corpus.dense_regime(), sum9=corpus.uniform_sum_only(9), sum14=corpus.uniform_sum_only(14))
    return m


_REF = {}


def chain_ref(oracle, key, rows, b):
    """oracle.rows_fma of a (named list, B), computed once and shared; handed out read-only."""
    key = (key, b.shape[1], b.dtype.str)
    if key not in _REF:
        assert np.diff(np.asarray(rows[0], np.int64)).max(initial=0) <= 1 or fc.corpus_is_sharp(rows, b), f"{key}: the corpus is not sharp"
        ref = oracle.rows_fma(*rows, b)
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def padded_device(x, rng):
    """x on the device inside a wider buffer (random leading dimension, sometimes a misaligned start)."""
    r, c = x.shape
    ld = c + int(rng.integers(0, 9))
    shift = int(rng.integers(0, 3))
    buf = torch.zeros(r * ld + 4, dtype=torch.float32, device="cuda")
    view = buf[shift:shift + r * ld].view(r, ld)[:, :c]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    return view


def padded_out(r, c, rng):
    ld = c + int(rng.integers(0, 9))
    shift = int(rng.integers(0, 3))
    buf = torch.full((r * ld + 4,), 7.0, dtype=torch.float32, device="cuda")
    return buf[shift:shift + r * ld].view(r, ld)[:, :c]


def operands(b, m, seed):
    """(B on the device, out): contiguous where N is a multiple of 4, the padded operands of the fuzz suite otherwise."""
    n = b.shape[1]
    if n % 4 == 0:
        return dev(b), torch.full((m, n), 7.0, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(seed)
    return padded_device(b, rng), padded_out(m, n, rng)


def family(tag, families):
    return any(f in tag for f in families)


def check_single(path, out, ref, families, fuzz=False):
    """The launch just made must have been one of `families`, in FAST mode, and return the chain's bits."""
    tag = capi.last_kernel()
    SEEN.setdefault(path, set()).add(tag.split(" ")[0])
    assert family(tag, families) and "fast" in tag, f"{path}: expected {families} in FAST mode, the library ran {tag!r}"
    (assert_same_bits64 if ref.dtype == np.float64 else assert_same_bits)(out, ref, f"{path} [{tag}]")
    TALLY["fuzz_bitwise" if fuzz else "bitwise"] += ref.size


def gather_body_rows(row_ptrs, share_len):
    """The rows a two-body launch over this list hands to its row-gather body: the span positions behind the long ones."""
    spans = ops.csr_spans_by_length(row_ptrs, share_len)
    rows = spans[ops.spans_long_count(spans):, 0].astype(np.int64)
    lens = np.diff(np.asarray(row_ptrs, np.int64))
    assert np.all(lens[rows] <= ops.HYBRID_ROW_LEN)
    return rows


def check_split(path, run, rows, b, oracle, share_len, fuzz=False):
    """A path that promises a fixed order: within the derived any-order bound of the exact sum, identical run to run, and --
    under the two-body launch -- the chain's bits on every row of the row-gather body."""
    got = run().cpu().numpy()
    tag = capi.last_kernel()
    SEEN.setdefault(path, set()).add(tag.split(" ")[0])
    assert family(tag, SPLIT) and "fast" in tag, f"{path}: expected a split launch in FAST mode, the library ran {tag!r}"
    again = run().cpu().numpy()
    assert capi.last_kernel() == tag
    assert_same_bits(again, got, f"{path}: two runs [{tag}]")
    exact, bound = fc.exact_and_bound(rows, b)
    err = np.abs(got.astype(np.float64) - exact)
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))
    print(f"{path} [{tag.split(' ')[0]}]: worst err / any-order bound = {worst:.3f}")
    assert np.all(err <= bound), f"{path} [{tag}]: err / bound up to {worst:.3g}"
    chained = 0
    if "csr_hybrid<" in tag:
        short = gather_body_rows(rows[0], share_len)
        ref = oracle.rows_fma(*rows, b)
        for r in short:
            assert_same_bits(got[r], ref[r], f"{path}: row {r} of the row-gather body [{tag}]")
        chained = short.shape[0] * b.shape[1]
    TALLY["fuzz_bitwise" if fuzz else "bitwise"] += chained
    TALLY["fuzz_bounded" if fuzz else "bounded"] += got.size - chained
    return got


def check_by_tag(path, run, rows, b, oracle, share_len, fuzz=False):
    """The fuzz's switch: whatever the dispatch took decides which check applies; an unknown tag is a failure."""
    out = run()
    tag = capi.last_kernel()
    if family(tag, SPLIT):
        check_split(path, run, rows, b, oracle, share_len, fuzz)
    else:
        check_single(path, out, oracle.rows_fma(*rows, b), SINGLE, fuzz)


# ------------------------------------------------------------------------------------------------ single-chain paths
@pytest.mark.parametrize("n", [1, 3, 4, 60, 64, 130, 256])
@pytest.mark.parametrize("name", ["ragged", "long_tail"])
def test_csr_kernels_1_to_4_return_the_chain(oracle, mats, name, n):
    csr = mats[name]
    b = corpus.dense_b(csr.num_cols, n)
    ref = chain_ref(oracle, name, fc.csr_rows(csr), b)
    a = ops.DeviceCSR.from_host(csr, spans=False, plan=False)
    for kernel, tag in ((1, "csr_k1<"), (2, "csr_k2<"), (3, "csr_k3<"), (4, "csr_k3<")):
        bd, out = operands(b, csr.num_rows, 100 * n + kernel)
        ops.spmm_csr(a, bd, out=out, kernel=kernel, acc="fast")
        check_single(f"spmm_csr kernel {kernel}", out, ref, (tag,))


@pytest.mark.parametrize("n", [4, 64, 128, 200, 512])
@pytest.mark.parametrize("name", ["ragged", "long_tail"] + [f"uniform{w}" for w in corpus.UNIFORM_WIDTHS])
def test_csr_kernel_5_and_0_return_the_chain(oracle, mats, name, n):
    """The row-gather kernel: rolling-refill and batch-at-a-time bodies, every slot count of the uniform-row entry point, the
    general entry point on the same uniform rows (use_hint=False: its bet on nnz / M is right)."""
    csr = mats[name]
    b = corpus.dense_b(csr.num_cols, n)
    ref = chain_ref(oracle, name, fc.csr_rows(csr), b)
    a = ops.DeviceCSR.from_host(csr, spans=False, plan=False)       # no span list: the long tail stays on the row-gather kernel
    for kernel in (5, 0):
        for hint in (True, False):
            bd, out = operands(b, csr.num_rows, 7 * n + kernel)
            ops.spmm_csr(a, bd, out=out, kernel=kernel, acc="fast", use_hint=hint)
            check_single(f"spmm_csr kernel {kernel}{'' if hint else ' general entry'} ({name.rstrip('0123456789')})", out, ref, ("row_gather<",))
    if name.startswith("uniform") and n == 200:                   # strided operands through the uniform-row entry point
        rng = np.random.default_rng(n)
        bd, out = padded_device(b, rng), padded_out(csr.num_rows, n, rng)
        ops.spmm_csr(a, bd, out=out, acc="fast")
        check_single("spmm_csr uniform-row entry, strided", out, ref, ("row_gather<",))


@pytest.mark.parametrize("name", ["sum9", "sum14"])
def test_general_entry_bet_on_non_uniform_rows_returns_the_chain(oracle, mats, name):
    """nnz divides by M, the rows are not uniform: the general entry point bets, every wave must notice and fetch again."""
    csr = mats[name]
    assert csr.nnz % csr.num_rows == 0 and ops.uniform_row_nnz(csr.row_ptrs) == 0
    a = ops.DeviceCSR.from_host(csr, spans=False, plan=False)
    for n in (64, 128, 200):
        b = corpus.dense_b(csr.num_cols, n)
        ref = chain_ref(oracle, name, fc.csr_rows(csr), b)
        bd, out = operands(b, csr.num_rows, n)
        ops.spmm_csr(a, bd, out=out, acc="fast", use_hint=False)
        check_single("spmm_csr general entry, bet lost", out, ref, ("row_gather<",))


@pytest.mark.parametrize("n", [64, 130, 200])
def test_deep_wave_per_row_kernel_returns_the_chain(oracle, mats, n):
    """Long rows on average, a B with an odd leading dimension (no 16-byte rows), N < 384: csr_wave_deep."""
    csr = mats["long_mean"]
    b = corpus.dense_b(csr.num_cols, n)
    ref = chain_ref(oracle, "long_mean", fc.csr_rows(csr), b)
    wide = torch.zeros((csr.num_cols, n + 1 + n % 2), dtype=torch.float32, device="cuda")
    assert wide.stride(0) % 2 == 1
    wide[:, :n] = dev(b)
    for a in (ops.DeviceCSR.from_host(csr), ops.DeviceCSR.from_host(csr, spans=False)):
        for kernel in (0, 5, 6):                                    # kernel 6 is handed on to kernel 5 where the split kernel declines
            out = ops.spmm_csr(a, wide[:, :n], kernel=kernel, acc="fast")
            check_single("spmm_csr long rows, odd ldb", out, ref, ("csr_wave_deep<",))


@pytest.mark.parametrize("name,n", [("uniform14", 128), ("uniform9", 128), ("ragged", 64)])
def test_plan_order_returns_the_chain(oracle, mats, name, n):
    """Rows permuted into the clustered order, C rows scattered through the row map; single and a batch of 2.  A shape the
    plan launch declines is recorded and nothing is compared for it."""
    csr = mats[name]
    b = corpus.dense_b(csr.num_cols, n)
    ref = chain_ref(oracle, name, fc.csr_rows(csr), b)
    a = ops.DeviceCSR.from_host(csr, plan=True, spans=False)
    bd = dev(b)
    out = torch.full((csr.num_rows, n), 7.0, device="cuda")
    if not ops._csr_plan(a, [bd], [out], "fast", None):
        SEEN.setdefault("plan order", set()).add(f"declined {name} N={n}")
        return
    assert "plan-order" in capi.last_kernel()
    check_single("plan order", out, ref, ("row_gather<",))
    outs = [torch.full((csr.num_rows, n), 7.0, device="cuda") for _ in range(2)]
    assert ops._csr_plan(a, [bd, bd], outs, "fast", None)
    assert "plan-order" in capi.last_kernel() and "batched" in capi.last_kernel()
    check_single("plan order, batch of 2", outs[0], ref, ("row_gather<",))
    check_single("plan order, batch of 2", outs[1], ref, ("row_gather<",))


@pytest.mark.parametrize("count", [3, 17])
def test_batched_launch_returns_the_chain_for_every_operand(oracle, mats, count):
    csr = mats["uniform14"]
    rng = np.random.default_rng(count)
    base = corpus.dense_b(csr.num_cols, 128)
    bs = [base] + [fc.sharp_values(rng, base.shape, np.float32) for _ in range(2)]     # three different operands, cycled
    refs = [chain_ref(oracle, "uniform14", fc.csr_rows(csr), base)] + [oracle.rows_fma(*fc.csr_rows(csr), x) for x in bs[1:]]
    a = ops.DeviceCSR.from_host(csr, spans=False, plan=False)
    outs = ops.spmm_csr_batch(a, [dev(bs[i % 3]) for i in range(count)], acc="fast")
    assert "batched" in capi.last_kernel()
    for i, out in enumerate(outs):
        check_single("spmm_csr_batch", out, refs[i % 3], ("row_gather<",))
    single = ops.spmm_csr(a, dev(base), acc="fast")
    assert_same_bits(outs[0], single.cpu().numpy(), "batched equals the single launch")


def test_lds_tiles_return_the_chain(oracle, mats):
    csr = mats["uniform14"]
    b = corpus.dense_b(csr.num_cols, 128)
    out = ops.spmm_csr_tiles(ops.DeviceCSRTiles.from_host(csr), dev(b), acc="fast")
    check_single("spmm_csr_tiles", out, chain_ref(oracle, "uniform14", fc.csr_rows(csr), b), ("csr_lds_tile<fast",))


@pytest.mark.parametrize("n", [64, 200])
def test_panel_kernel_returns_the_chain(oracle, mats, n):
    csr = mats["dense"]
    a = ops.DeviceCSRPanels.from_host(csr, panel_rows=128)
    assert a.num_panels == 3                                         # 128 + 128 + 44 B rows
    b = corpus.dense_b(csr.num_cols, n)
    out = ops.spmm_csr_panels(a, dev(b), acc="fast")
    check_single("spmm_csr_panels", out, chain_ref(oracle, "dense", fc.csr_rows(csr), b), ("csr_panel<fast",))


@pytest.mark.parametrize("workspace", [True, False])
@pytest.mark.parametrize("name", ["ragged", "long_tail"])
def test_coo_returns_the_chain(oracle, mats, name, workspace):
    """Entries in a shuffled file order: the list is the stable sort by row, a row's entries NOT by column."""
    csr = mats[name]
    coo = formats.csr_to_coo(csr)
    shuffle = np.random.default_rng(5).permutation(coo.nnz)
    coo = formats.COO(coo.num_rows, coo.num_cols, coo.row_idxs[shuffle], coo.col_idxs[shuffle], coo.data[shuffle])
    rows = fc.coo_rows(coo)
    a = ops.DeviceCOO.from_host(coo)
    for n in (3, 64, 130):
        b = corpus.dense_b(csr.num_cols, n)
        ref = chain_ref(oracle, name + " coo", rows, b)
        bd, out = operands(b, csr.num_rows, n)
        plain = ops.DeviceCOO(a.num_rows, a.num_cols, a.nnz, a.row_idxs, a.col_idxs, a.data)      # no span list: the COO kernels themselves
        ops.spmm_coo(plain, bd, out=out, workspace=workspace, acc="fast")
        check_single(f"spmm_coo workspace={workspace}", out, ref, ("row_gather<",) if workspace else ("coo_k1<",))
        if a.spans is not None and workspace:                       # the long tail as uploaded: the two-body launch where the shape has one
            check_by_tag("spmm_coo with its span list", lambda: ops.spmm_coo(a, bd, acc="fast"), rows, b, oracle, 0xFFFFFFFF)


@pytest.mark.parametrize("name", ["ragged", "uniform9"])
def test_ell_returns_the_chain(oracle, mats, name):
    csr = mats[name]
    ellc = formats.csr_to_ell_colmajor(csr)
    rows = fc.ell_colmajor_rows(ellc)
    for n in (3, 64, 200):
        b = corpus.dense_b(csr.num_cols, n)
        ref = chain_ref(oracle, name + " ell", rows, b)
        for compact in (False, True):
            a = ops.DeviceELL.from_host(ellc, compact=compact)
            assert (a.compact is not None) == compact and (not compact or a.compact[4] is None)
            bd, out = operands(b, csr.num_rows, n)
            ops.spmm_ell(a, bd, out=out, acc="fast")
            check_single(f"spmm_ell {'compact' if compact else 'padded'}", out, ref, ("row_gather<",))


@pytest.mark.parametrize("shape", list(corpus.BSR_SHAPES))
def test_bsr_kernel_1_and_zero_skipping_list_return_their_chains(oracle, shape):
    """Kernel 1 keeps the explicit zeros in its chain, the zero-skipping list drops them (the same bits on finite data, two
    lists all the same: each path against its own)."""
    bsr = corpus.bsr(*shape)
    kept, skipped = fc.bsr_rows(bsr, skip_zeros=False), fc.bsr_rows(bsr, skip_zeros=True)
    a = ops.DeviceBSR.from_host(bsr)
    nz = ops.bsr_nonzeros(bsr)
    assert nz.spans is None and nz.nnz // nz.num_rows < 24          # a short list: the row kernel, not the split shape
    for n in (3, 64, 200):
        b = corpus.dense_b(bsr.num_cols, n)
        bd, out = operands(b, bsr.num_rows, n)
        ops.spmm_bsr(a, bd, out=out, kernel=1, acc="fast")
        check_single(f"spmm_bsr kernel 1 {shape[0]}x{shape[1]}", out, chain_ref(oracle, f"bsr{shape} kept", kept, b), ("bsr_valu<", "bsr_rowblock<"))
        bd, out = operands(b, bsr.num_rows, n + 1000)
        ops.spmm_bsr_nonzeros(nz, bd, out=out, acc="fast")
        check_single(f"spmm_bsr_nonzeros {shape[0]}x{shape[1]}", out, chain_ref(oracle, f"bsr{shape} skipped", skipped, b), ("row_gather<",))


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 200])
@pytest.mark.parametrize("name", ["ragged", "long_tail", "long_mean"])
def test_fp64_returns_the_fp64_chain(oracle, mats, name, n):
    csr = mats[name]
    f64 = formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs,
                      fc.sharp_values(np.random.default_rng(csr.nnz), csr.nnz, np.float64))
    b = corpus.dense_b(csr.num_cols, n, np.float64)
    rows = fc.csr_rows(f64, np.float64)
    ref = chain_ref(oracle, name + " f64", rows, b)
    bd = dev(b)
    body = "V2" if n % 2 == 0 else "V1"                             # the 16-byte body and the 8-byte body
    out = ops.spmm_csr(ops.DeviceCSR.from_host(f64, dtype=torch.float64), bd, acc="fast")
    assert body in capi.last_kernel(), capi.last_kernel()
    check_single(f"fp64 spmm_csr {body}", out, ref, ("csr_f64<",))
    coo = formats.csr_to_coo(f64)
    out = ops.spmm_coo(ops.DeviceCOO.from_host(coo, dtype=torch.float64), bd, acc="fast")
    check_single(f"fp64 spmm_coo {body}", out, ref, ("csr_f64<",))
    if name != "long_mean" or n in (3, 64):                         # the long rows' column-major ELL is wide: two widths are enough
        ellc = formats.csr_to_ell_colmajor(f64)
        assert all(np.array_equal(x, y) for x, y in zip(fc.ell_colmajor_rows(ellc, np.float64), rows))
        out = ops.spmm_ell(ops.DeviceELL.from_host(ellc, dtype=torch.float64), bd, acc="fast")
        check_single(f"fp64 spmm_ell {body}", out, ref, ("csr_f64<",))


@pytest.mark.parametrize("n", [3, 64])
def test_fp64_zero_skipping_bsr_list_returns_the_fp64_chain(oracle, n):
    for shape in ((4, 4), (3, 5), (16, 16)):
        bsr = corpus.bsr(*shape)
        rng = np.random.default_rng(shape[0])
        bsr64 = formats.BSR(bsr.num_rows, bsr.num_cols, bsr.nnz, shape[0], shape[1], bsr.block_row_ptrs, bsr.block_col_idxs,
                            np.where(bsr.data != 0, fc.sharp_values(rng, bsr.data.shape, np.float64), 0.0))
        rows = fc.bsr_rows(bsr64, True, np.float64)
        b = corpus.dense_b(bsr.num_cols, n, np.float64)
        out = ops.spmm_bsr_nonzeros(ops.bsr_nonzeros(bsr64, dtype=torch.float64), dev(b), acc="fast")
        check_single("fp64 spmm_bsr_nonzeros", out, chain_ref(oracle, f"bsr{shape} f64", rows, b), ("csr_f64<",))


# ------------------------------------------------------------------------------------------------ split paths
@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("name", ["ragged", "long_tail", "long_mean"])
def test_kernel_6_keeps_its_fixed_order_within_the_any_order_bound(oracle, mats, name, n):
    csr = mats[name]
    rows, b = fc.csr_rows(csr), corpus.dense_b(csr.num_cols, n)
    chain_ref(oracle, name, rows, b)                                # the precondition: sharp data
    bd = dev(b)
    for spans in (False, True):                                     # rows in order / the span list, longest first
        a = ops.DeviceCSR.from_host(csr, spans=spans, plan=False)
        check_split(f"spmm_csr kernel 6{' span list' if spans else ''}", lambda: ops.spmm_csr(a, bd, kernel=6, acc="fast"), rows, b, oracle, 0)
        assert ("csr_split<" in capi.last_kernel()) and (("longest-first" in capi.last_kernel()) == spans)


@pytest.mark.parametrize("n", [64, 128, 512])
def test_long_row_dispatch_of_kernel_5(oracle, mats, n):
    """Mean row of 24 entries or more, 16-byte rows: the library's kernel 5 takes the split kernel (FAST at every width),
    and with a span list the two-body launch, whose row-gather rows are chains."""
    csr = mats["long_mean"]
    rows, b = fc.csr_rows(csr), corpus.dense_b(csr.num_cols, n)
    chain_ref(oracle, "long_mean", rows, b)
    bd = dev(b)
    a = ops.DeviceCSR.from_host(csr, spans=False, plan=False)
    for kernel in (0, 5):
        check_split("spmm_csr kernel 5, long mean", lambda: ops.spmm_csr(a, bd, kernel=kernel, acc="fast"), rows, b, oracle, 0)
        assert "csr_split<" in capi.last_kernel()
    a = ops.DeviceCSR.from_host(csr, spans=True, plan=False)
    assert 0 < a.long_spans < a.spans.numel() // 4
    check_split("spmm_csr span list, long mean", lambda: ops.spmm_csr(a, bd, acc="fast"), rows, b, oracle, 0)


@pytest.mark.parametrize("n", [64, 128])
def test_two_body_launch_on_the_long_tail(oracle, mats, n):
    csr = mats["long_tail"]
    rows, b = fc.csr_rows(csr), corpus.dense_b(csr.num_cols, n)
    chain_ref(oracle, "long_tail", rows, b)
    a = ops.DeviceCSR.from_host(csr, spans=True, plan=False)
    bd = dev(b)
    check_split("spmm_csr two-body launch", lambda: ops.spmm_csr(a, bd, acc="fast"), rows, b, oracle, 0)
    assert "csr_hybrid<" in capi.last_kernel(), capi.last_kernel()


@pytest.mark.parametrize("n", [64, 128])
def test_coo_ell_and_bsr_lists_on_long_rows(oracle, mats, n):
    """rows_hybrid (long mean: some rows at or below the threshold) and rows_split (long only: none)."""
    for name, want in (("long_mean", "csr_hybrid<"), ("long_only", "csr_split<")):
        csr = mats[name]
        rows, b = fc.csr_rows(csr), corpus.dense_b(csr.num_cols, n)
        chain_ref(oracle, name, rows, b)
        bd = dev(b)
        coo = ops.DeviceCOO.from_host(formats.csr_to_coo(csr))
        check_split(f"spmm_coo {name}", lambda: ops.spmm_coo(coo, bd, acc="fast"), rows, b, oracle, 0xFFFFFFFF)
        assert want in capi.last_kernel(), capi.last_kernel()
        ell = ops.DeviceELL.from_host(formats.csr_to_ell_colmajor(csr), compact=True)
        check_split(f"spmm_ell compact {name}", lambda: ops.spmm_ell(ell, bd, acc="fast"), rows, b, oracle, 0xFFFFFFFF)
        assert want in capi.last_kernel(), capi.last_kernel()
    bsr = corpus.bsr_long()
    rows, b = fc.bsr_rows(bsr, skip_zeros=True), corpus.dense_b(bsr.num_cols, n)
    chain_ref(oracle, "bsr long", rows, b)
    nz = ops.bsr_nonzeros(bsr)
    assert nz.spans is not None
    bd = dev(b)
    check_split("spmm_bsr_nonzeros long rows", lambda: ops.spmm_bsr_nonzeros(nz, bd, acc="fast"), rows, b, oracle, 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the seeded FAST fuzz
def fuzz_csr_case(oracle, seed):
    csr, b = corpus.fuzz_csr(seed)
    rows = fc.csr_rows(csr)
    assert fc.corpus_is_sharp(rows, b), f"CSR fuzz seed {seed} is not sharp: vet another"
    rng = np.random.default_rng(seed)
    m, n = csr.num_rows, b.shape[1]
    bd = padded_device(b, rng)
    a = ops.DeviceCSR.from_host(csr)
    for kernel in (0, 1, 2, 3, 4, 5, 6):
        out = padded_out(m, n, rng)
        check_by_tag(f"fuzz CSR kernel {kernel}", lambda: ops.spmm_csr(a, bd, out=out, kernel=kernel, acc="fast"), rows, b, oracle, 0, fuzz=True)
    coo = formats.csr_to_coo(csr)
    ac = ops.DeviceCOO.from_host(coo)
    for ws in (True, False):
        check_by_tag(f"fuzz COO workspace={ws}", lambda: ops.spmm_coo(ac, bd, workspace=ws, acc="fast"), fc.coo_rows(coo), b, oracle, 0xFFFFFFFF, fuzz=True)
    ellc = formats.csr_to_ell_colmajor(csr)
    ae = ops.DeviceELL.from_host(ellc)
    out = padded_out(m, n, rng)
    check_by_tag("fuzz ELL", lambda: ops.spmm_ell(ae, bd, out=out, acc="fast"), fc.ell_colmajor_rows(ellc), b, oracle, 0xFFFFFFFF, fuzz=True)
    TALLY["fuzz_cases"] += 1


def fuzz_bsr_case(oracle, seed):
    bsr, b = corpus.fuzz_bsr(seed)
    kept, skipped = fc.bsr_rows(bsr, False), fc.bsr_rows(bsr, True)
    assert fc.corpus_is_sharp(kept, b) and fc.corpus_is_sharp(skipped, b), f"BSR fuzz seed {seed} is not sharp: vet another"
    rng = np.random.default_rng(seed)
    bd = padded_device(b, rng)
    a = ops.DeviceBSR.from_host(bsr)
    out = padded_out(bsr.num_rows, b.shape[1], rng)
    check_by_tag("fuzz BSR kernel 1", lambda: ops.spmm_bsr(a, bd, out=out, kernel=1, acc="fast"), kept, b, oracle, 0xFFFFFFFF, fuzz=True)
    nz = ops.bsr_nonzeros(bsr)
    check_by_tag("fuzz BSR zero-skipping list", lambda: ops.spmm_bsr_nonzeros(nz, bd, acc="fast"), skipped, b, oracle, 0xFFFFFFFF, fuzz=True)
    TALLY["fuzz_cases"] += 1


@pytest.mark.parametrize("seed", corpus.fuzz_seeds(corpus.FUZZ_CSR_SEEDS, 12 * SCALE))
def test_fuzz_fast_csr_coo_ell(oracle, seed):
    fuzz_csr_case(oracle, seed)


@pytest.mark.parametrize("seed", corpus.fuzz_seeds(corpus.FUZZ_BSR_SEEDS, 8 * SCALE))
def test_fuzz_fast_bsr(oracle, seed):
    fuzz_bsr_case(oracle, seed)


def test_fuzz_compares_at_least_four_fifths_of_its_elements_bitwise(oracle):
    """The tag switch must not quietly move the fuzz onto the loose branch.  Counts what the fuzz tests of this session
    compared; run on its own it first runs one seed of each."""
    if TALLY["fuzz_cases"] == 0:
        fuzz_csr_case(oracle, corpus.FUZZ_CSR_SEEDS[0])
        fuzz_bsr_case(oracle, corpus.FUZZ_BSR_SEEDS[0])
    total = TALLY["fuzz_bitwise"] + TALLY["fuzz_bounded"]
    share = TALLY["fuzz_bitwise"] / total
    print(f"FAST fuzz: {TALLY['fuzz_cases']} cases, {TALLY['fuzz_bitwise']} of {total} elements compared bitwise: share {share:.3f}")
    print(f"FAST corpus: {TALLY['bitwise']} elements compared bitwise, {TALLY['bounded']} held to the any-order bound")
    for path in sorted(SEEN):
        print(f"  {path}: {', '.join(sorted(SEEN[path]))}")
    assert share >= 0.80, f"only {share:.3f} of the fuzz elements were compared bitwise"
