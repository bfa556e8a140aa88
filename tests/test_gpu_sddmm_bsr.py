"""SDDMM on a BSR pattern in bf16 (mispmm_sddmm_bsr_bf16) and the autograd function for the bf16 block-sparse product built on
it, on the GPU, against the numpy restatement and the bounds of tests/_sddmm_bsr_ref.py.

Worst |out - exact| / bound measured on the MI355X (`-s` prints every one): full-mantissa operands
fp32 out 0 (those sums are exactly representable), bf16 out 0.992; wide-exponent operands fp32 out 0.399, bf16 out 0.995."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, formats, ops, synth  # noqa: E402

from _sddmm_bsr_ref import (assert_within, block_rows, from_bits, full_mantissa, pattern, sddmm_bsr_exact, small_ints,  # noqa: E402
                            to_bits, wide_exponent)

pytestmark = pytest.mark.gpu

PATTERNS = ["ragged16", "ragged32"]
WIDE = [8, 24, 32, 40, 64, 72, 128, 264]      # N, ldx, ldy multiples of 8: 16-byte lanes
NARROW = [1, 3, 4, 12, 33, 100]               # element by element
# beyond the widths the contract lists: the chunk loop of either body (N above 256 / above 128), more than one pass of it.
# Integers in [-8, 8]: every sum stays below 2^16, exact in fp32 in any order.
LOOP = [512, 520, 259]     # 512: whole passes only -- the store follows the last product at once
BOUND_WIDTHS = [24, 40, 128, 264, 3, 33]      # one width per body either side of a 32-column step


@functools.lru_cache(maxsize=None)
def device_bsr(name):
    return ops.DeviceBSR.from_host(pattern(name))


@functools.lru_cache(maxsize=None)
def operands(name, n, kind="full"):
    """(x, y) on the host for (pattern, N): float32 arrays of bf16 numbers, shared by the tests that use them; read-only."""
    bsr = pattern(name)
    rng = np.random.default_rng(2000 + n)
    make = {"full": full_mantissa, "ints": small_ints, "wide": wide_exponent}[kind]
    return make(rng, (bsr.num_rows, n)), make(rng, (bsr.num_cols, n))


@functools.lru_cache(maxsize=None)
def reference(name, n, kind="full"):
    return sddmm_bsr_exact(pattern(name), *operands(name, n, kind))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(v):
    return dev(to_bits(v))


def host(out):
    """A result as float32 on the host, whichever out type."""
    a = out.cpu().numpy()
    return from_bits(a) if a.dtype == np.int16 else a


def body(n):
    return "wide" if n % 8 == 0 else "narrow"


@pytest.mark.parametrize("n", WIDE + NARROW + LOOP)
@pytest.mark.parametrize("name", PATTERNS)
def test_sddmm_bsr_is_exact_on_small_integers(name, n):
    a = device_bsr(name)
    x, y = operands(name, n, "ints")
    exact, _ = reference(name, n, "ints")
    xd, yd = bits(x), bits(y)
    for out_bf16 in (False, True):
        out = ops.sddmm_bsr_bf16(a, xd, yd, out_bf16=out_bf16)
        tag = capi.last_kernel()
        assert tag.startswith(f"sddmm_bsr<b{a.block_row_size},{body(n)},{'bf16' if out_bf16 else 'f32'},"), tag
        assert ("loop" in tag) == (n > (256 if body(n) == "wide" else 128)), tag
        assert out.shape == (a.num_blocks, a.block_row_size, a.block_row_size) and out.dtype == (torch.int16 if out_bf16 else torch.float32)
        want = synth.bf16_round(exact.astype(np.float32)) if out_bf16 else exact
        got = host(out)
        assert np.array_equal(got.astype(np.float64), want.astype(np.float64)), \
            f"{name} N={n} {tag}: {int((got != want).sum())} elements differ, first at {np.argwhere(got != want)[:3].tolist()}"


def test_sddmm_bsr_is_exact_on_activsg10k():
    bsr = pattern("ACTIVSg10K")
    a = ops.DeviceBSR.from_host(bsr)
    rng = np.random.default_rng(61)
    x, y = small_ints(rng, (bsr.num_rows, 128)), small_ints(rng, (bsr.num_cols, 128))
    exact, _ = sddmm_bsr_exact(bsr, x, y, dtype=np.float64)
    got = ops.sddmm_bsr_bf16(a, bits(x), bits(y)).cpu().numpy()
    assert capi.last_kernel().startswith("sddmm_bsr<b16,wide,f32,"), capi.last_kernel()
    assert np.array_equal(got.astype(np.float64), exact), f"{int((got != exact).sum())} of {exact.size} elements differ"


@pytest.mark.parametrize("n", BOUND_WIDTHS)
@pytest.mark.parametrize("name", PATTERNS)
def test_sddmm_bsr_within_the_stated_bound(name, n):
    a = device_bsr(name)
    x, y = operands(name, n)
    exact, scale = reference(name, n)
    xd, yd = bits(x), bits(y)
    for out_bf16 in (False, True):
        out = ops.sddmm_bsr_bf16(a, xd, yd, out_bf16=out_bf16)
        assert body(n) in capi.last_kernel()
        assert_within(host(out), out_bf16, n, exact, scale, f"{name} N={n} {capi.last_kernel()}")


@pytest.mark.parametrize("n", BOUND_WIDTHS)
@pytest.mark.parametrize("name", PATTERNS)
def test_sddmm_bsr_within_the_stated_bound_on_a_wide_exponent_range(name, n):
    """The same bound on operands whose exponents span 2^-8 .. 2^8.  The sums of full-mantissa operands in [0.5, 2) are all exactly
    representable in fp32 (products are multiples of 2^-16, sums stay below 2^8), so they test the fp32 out type for exactness
    only; here the accumulate inside the instruction has to round."""
    a = device_bsr(name)
    x, y = operands(name, n, "wide")
    exact, scale = reference(name, n, "wide")
    xd, yd = bits(x), bits(y)
    for out_bf16 in (False, True):
        out = ops.sddmm_bsr_bf16(a, xd, yd, out_bf16=out_bf16)
        assert_within(host(out), out_bf16, n, exact, scale, f"wide exponents {name} N={n} {capi.last_kernel()}")


@pytest.mark.parametrize("name,n,pad", [("ragged16", 40, 8), ("ragged16", 40, 3), ("ragged32", 72, 8), ("ragged32", 24, 3),
                                        ("ragged16", 264, 8), ("ragged16", 33, 3)])
def test_sddmm_bsr_strided_operands_and_out_sentinels(name, n, pad):
    """ldx, ldy > N with NaN in the gap columns (a kernel that reads a gap poisons its sum; a pad of 8 keeps the 16-byte lanes,
    a pad of 3 forces the element-wise body), and `out` as the head of a longer buffer whose tail must stay untouched."""
    a = device_bsr(name)
    x, y = operands(name, n)
    exact, scale = reference(name, n)
    nan = 0x7FC0
    xb = torch.full((a.num_rows, n + pad), nan, dtype=torch.int16, device="cuda")
    yb = torch.full((a.num_cols, n + 2 * pad), nan, dtype=torch.int16, device="cuda")
    xb[:, :n], yb[:, :n] = bits(x), bits(y)
    count = a.num_blocks * a.block_row_size ** 2
    shape = (a.num_blocks, a.block_row_size, a.block_row_size)
    for out_bf16 in (False, True):
        buf = torch.full((count + 37,), 0x1234, dtype=torch.int16, device="cuda") if out_bf16 else torch.full((count + 37,), -7.0, device="cuda")
        got = ops.sddmm_bsr_bf16(a, xb[:, :n], yb[:, :n], out_bf16=out_bf16, out=buf[:count].view(shape))
        assert got.data_ptr() == buf.data_ptr()
        assert ("narrow" if pad % 8 or n % 8 else "wide") in capi.last_kernel(), capi.last_kernel()
        assert bool((buf[count:] == (0x1234 if out_bf16 else -7.0)).all()), "elements behind the last block were written"
        assert_within(host(got), out_bf16, n, exact, scale, f"strided {name} N={n} pad={pad} {capi.last_kernel()}")


@pytest.mark.parametrize("which", ["x", "y"])
@pytest.mark.parametrize("name,n", [("ragged16", 64), ("ragged32", 40), ("ragged16", 264), ("ragged32", 256)])
def test_sddmm_bsr_misaligned_operand_takes_the_narrow_body(name, n, which):
    """An operand that starts one element into its buffer is not 16-byte aligned: element by element, and -- the same
    instruction on the same fragments in the same order -- the same bits."""
    a = device_bsr(name)
    x, y = operands(name, n)

    def shifted(v):
        flat = torch.full((v.size + 1,), 0x7FC0, dtype=torch.int16, device="cuda")
        flat[1:] = bits(v).reshape(-1)
        return flat[1:].view(v.shape)
    xd, yd = (shifted(x), bits(y)) if which == "x" else (bits(x), shifted(y))
    assert (xd.data_ptr() % 16 != 0) or (yd.data_ptr() % 16 != 0)
    for out_bf16 in (False, True):
        want = ops.sddmm_bsr_bf16(a, bits(x), bits(y), out_bf16=out_bf16)
        assert "wide" in capi.last_kernel(), capi.last_kernel()
        got = ops.sddmm_bsr_bf16(a, xd, yd, out_bf16=out_bf16)
        assert "narrow" in capi.last_kernel(), capi.last_kernel()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"misaligned {which} N={n}"


@pytest.mark.parametrize("name,n", [("ragged16", 40), ("ragged16", 33), ("ragged32", 72), ("ragged32", 3)])
def test_sddmm_bsr_nan_stays_in_its_row(name, n):
    """One NaN in X[r][.]: row r mod bS of every block of block row r / bS is NaN, every other element keeps its bits."""
    bsr, a = pattern(name), device_bsr(name)
    bs = bsr.block_row_size
    x, y = operands(name, n)
    brow = int(np.argmax(np.diff(bsr.block_row_ptrs.astype(np.int64))))        # the fullest block row
    r = brow * bs + bs - 3
    xn = x.copy()
    xn[r, n // 2] = np.nan
    hit = np.zeros((bsr.num_blocks, bs, bs), bool)
    hit[block_rows(bsr) == brow, r % bs, :] = True
    assert hit.sum() == bs * int(np.diff(bsr.block_row_ptrs.astype(np.int64)).max())
    for out_bf16 in (False, True):
        clean = ops.sddmm_bsr_bf16(a, bits(x), bits(y), out_bf16=out_bf16).cpu().numpy()
        got = ops.sddmm_bsr_bf16(a, bits(xn), bits(y), out_bf16=out_bf16).cpu().numpy()
        assert np.array_equal(np.isnan(host_f32(got)), hit), "NaN positions differ"
        assert np.array_equal(got[~hit], clean[~hit])


def host_f32(a):
    return from_bits(a) if a.dtype == np.int16 else a


@pytest.mark.parametrize("name", PATTERNS)
def test_sddmm_bsr_zero_width_writes_plus_zero(name):
    a = device_bsr(name)
    shape = (a.num_blocks, a.block_row_size, a.block_row_size)
    x, y = (torch.empty((r, 0), dtype=torch.int16, device="cuda") for r in (a.num_rows, a.num_cols))
    for out_bf16 in (False, True):
        out = torch.full(shape, -0.0, device="cuda")
        out = out.to(torch.bfloat16).view(torch.int16) if out_bf16 else out
        assert bool((out.view(torch.int16) < 0).any())                          # the sign bits are there
        ops.sddmm_bsr_bf16(a, x, y, out_bf16=out_bf16, out=out)
        assert capi.last_kernel().startswith("sddmm_bsr<")
        assert not out.view(torch.int16).cpu().numpy().any()                   # +0: no bit set, the sign bit included


def test_sddmm_bsr_empty_pattern_and_bad_arguments():
    empty = ops.DeviceBSR.from_host(formats.BSR(32, 48, 0, 16, 16, np.zeros(3, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 16, 16), np.float32)))
    x, y = torch.ones((32, 8), dtype=torch.int16, device="cuda"), torch.ones((48, 8), dtype=torch.int16, device="cuda")
    assert ops.sddmm_bsr_bf16(empty, x, y).shape == (0, 16, 16)
    assert ops.sddmm_bsr_bf16(empty, x, y, out_bf16=True).dtype == torch.int16
    a = device_bsr("ragged16")
    x, y = (torch.zeros((r, 8), dtype=torch.int16, device="cuda") for r in (a.num_rows, a.num_cols))
    for bad_x, bad_y in ((x.float(), y), (x, y.view(torch.bfloat16)), (x, y[:, :4]), (x[:-16], y), (x, y[:-16]), (x.t().contiguous().t(), y),
                         (x.reshape(-1), y), (x.cpu(), y), (x[:1].expand(a.num_rows, 8), y), (x, y[:1].expand(a.num_cols, 8))):
        with pytest.raises(ValueError):
            ops.sddmm_bsr_bf16(a, bad_x, bad_y)
    with pytest.raises(ValueError):
        ops.sddmm_bsr_bf16(a, x, y, out=torch.empty((a.num_blocks, 16, 16), dtype=torch.int16, device="cuda"))       # fp32 asked for
    with pytest.raises(ValueError):
        ops.sddmm_bsr_bf16(a, x, y, out_bf16=True, out=torch.empty((a.num_blocks, 16, 16), device="cuda"))
    with pytest.raises(ValueError):
        ops.sddmm_bsr_bf16(a, x, y, out=torch.empty((a.num_blocks, 256), device="cuda"))


@pytest.mark.parametrize("name,n", [("ragged16", 72), ("ragged32", 33)])
def test_sddmm_bsr_is_deterministic_and_replays_from_a_graph(name, n):
    a = device_bsr(name)
    xd, yd = (bits(v) for v in operands(name, n))
    for out_bf16 in (False, True):
        eager = ops.sddmm_bsr_bf16(a, xd, yd, out_bf16=out_bf16).clone()
        assert torch.equal(ops.sddmm_bsr_bf16(a, xd, yd, out_bf16=out_bf16).view(torch.int16), eager.view(torch.int16)), "second run"
        out = torch.empty_like(eager)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.sddmm_bsr_bf16(a, xd, yd, out_bf16=out_bf16, out=out)             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.sddmm_bsr_bf16(a, xd, yd, out_bf16=out_bf16, out=out)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16)), "graph replay"


# ---- autograd
def bf(v):
    """float32 host array of bf16 numbers -> bfloat16 device tensor (the conversion is exact)."""
    return dev(v).to(torch.bfloat16)


def with_data(bsr, data):
    return formats.BSR(bsr.num_rows, bsr.num_cols, bsr.nnz, bsr.block_row_size, bsr.block_col_size, bsr.block_row_ptrs, bsr.block_col_idxs, data)


OUT_DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("n", [8, 72])
@pytest.mark.parametrize("name", PATTERNS)
def test_autograd_forward_is_the_library_product(name, n, out_dtype):
    rng = np.random.default_rng(71)
    bsr = with_data(pattern(name), full_mantissa(rng, pattern(name).data.shape))
    a = autograd.TrainableBSR.from_host(bsr)
    assert a.blocks.dtype == torch.bfloat16 and np.array_equal(a.blocks.float().cpu().numpy(), bsr.data)
    b = bf(full_mantissa(rng, (bsr.num_cols, n)))
    c = autograd.spmm_bsr(a, a.blocks.clone().requires_grad_(True), b, out_dtype=out_dtype)
    assert c.dtype == out_dtype and c.shape == (bsr.num_rows, n) and c.grad_fn is not None
    want = ops.spmm_bsr_bf16(a.fwd, a.blocks.view(torch.int16), b.view(torch.int16), out_bf16=out_dtype == torch.bfloat16)
    assert torch.equal(c.detach().view(want.dtype).view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("n", [4, 72])
@pytest.mark.parametrize("name", PATTERNS)
def test_autograd_gradients_are_exact_on_small_integers(name, n, out_dtype):
    """Blocks, b and grad_c integers in [-4, 4]: every sum of either gradient is an integer below 2^24, exact in fp32."""
    bsr = pattern(name)                                   # its data: integers in [-4, 4]
    rng = np.random.default_rng(72)
    b_h, g_h = small_ints(rng, (bsr.num_cols, n), most=4), small_ints(rng, (bsr.num_rows, n), most=4)
    a = autograd.TrainableBSR.from_host(bsr)
    blocks, b = a.blocks.clone().requires_grad_(True), bf(b_h).requires_grad_(True)
    c = autograd.spmm_bsr(a, blocks, b, out_dtype=out_dtype)
    c.backward(dev(g_h).to(out_dtype))
    assert blocks.grad.dtype == torch.bfloat16 and b.grad.dtype == torch.bfloat16
    exact, _ = sddmm_bsr_exact(bsr, g_h, b_h, dtype=np.float64)
    assert np.array_equal(blocks.grad.float().cpu().numpy(), synth.bf16_round(exact.astype(np.float32)))
    want_b = bsr.to_dense().astype(np.float64).T @ g_h.astype(np.float64)
    assert np.array_equal(b.grad.float().cpu().numpy(), synth.bf16_round(want_b.astype(np.float32)))


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("name,n", [("ragged16", 40), ("ragged32", 72), ("ragged16", 132)])
def test_autograd_block_gradient_within_the_stated_bound(name, n, out_dtype):
    """grad_c already holds bf16 numbers, so rounding it changes nothing: blocks.grad is the bf16-out SDDMM of (grad_c, b).
    b.grad comes from the forward kernel on the transposed pattern: checked on integers only, no new tolerance here."""
    rng = np.random.default_rng(73)
    bsr = with_data(pattern(name), full_mantissa(rng, pattern(name).data.shape))
    b_h, g_h = full_mantissa(rng, (bsr.num_cols, n)), full_mantissa(rng, (bsr.num_rows, n))
    a = autograd.TrainableBSR.from_host(bsr)
    blocks, b = a.blocks.clone().requires_grad_(True), bf(b_h).requires_grad_(True)
    autograd.spmm_bsr(a, blocks, b, out_dtype=out_dtype).backward(dev(g_h).to(out_dtype))
    exact, scale = sddmm_bsr_exact(bsr, g_h, b_h)
    assert_within(blocks.grad.float().cpu().numpy(), True, n, exact, scale, f"blocks.grad {name} N={n} {out_dtype}")
    assert b.grad.shape == b.shape and bool(torch.isfinite(b.grad.float()).all())


@pytest.mark.parametrize("name", PATTERNS)
def test_autograd_sum_backward_takes_a_stride_zero_gradient(name):
    bsr = pattern(name)
    bs = bsr.block_row_size
    rng = np.random.default_rng(74)
    b_h = small_ints(rng, (bsr.num_cols, 12), most=4)
    a = autograd.TrainableBSR.from_host(bsr)
    blocks, b = a.blocks.clone().requires_grad_(True), bf(b_h).requires_grad_(True)
    autograd.spmm_bsr(a, blocks, b).sum().backward()
    # d sum(C) / d blocks[e][i][j] = sum_n B[c * bS + j][n];  d sum(C) / d B[k][n] = the sum of column k of A
    row_sums = synth.bf16_round(b_h.sum(axis=1))
    cols = bsr.block_col_idxs.astype(np.int64)
    want = np.broadcast_to(row_sums[cols[:, None] * bs + np.arange(bs)][:, None, :], (bsr.num_blocks, bs, bs))
    assert np.array_equal(blocks.grad.float().cpu().numpy(), want)
    col_sums = synth.bf16_round(bsr.to_dense().sum(axis=0).astype(np.float32))
    assert np.array_equal(b.grad.float().cpu().numpy(), np.repeat(col_sums[:, None], 12, axis=1))


def test_autograd_frozen_inputs_skip_their_kernel():
    bsr = pattern("ragged16")
    a = autograd.TrainableBSR.from_host(bsr)
    b_h = small_ints(np.random.default_rng(75), (bsr.num_cols, 8), most=4)
    # the tag of the last kernel is kept per thread: run the backward pass on this one
    with torch.autograd.set_multithreading_enabled(False):
        blocks, b = a.blocks.clone().requires_grad_(True), bf(b_h)
        c = autograd.spmm_bsr(a, blocks, b)
        assert capi.last_kernel().startswith("bsr_mfma_bf16"), capi.last_kernel()
        c.sum().backward()
        assert capi.last_kernel().startswith("sddmm_bsr<"), capi.last_kernel()      # the last and only product of this backward
        assert b.grad is None and blocks.grad is not None
        blocks, b = a.blocks.clone(), bf(b_h).requires_grad_(True)
        c = autograd.spmm_bsr(a, blocks, b)
        ops.sddmm_bsr_bf16(a.fwd, ops.f32_to_bf16(c.detach()), b.detach().view(torch.int16))   # leave an SDDMM tag behind ...
        assert capi.last_kernel().startswith("sddmm_bsr<")
        c.sum().backward()
        assert capi.last_kernel().startswith("bsr_mfma_bf16"), capi.last_kernel()   # ... which the product with A^T replaces
        assert blocks.grad is None and b.grad is not None
        blocks, b = a.blocks.clone().requires_grad_(True), bf(b_h).requires_grad_(True)
        autograd.spmm_bsr(a, blocks, b).sum().backward()
        assert blocks.grad is not None and b.grad is not None
    out = autograd.spmm_bsr(a, a.blocks, bf(b_h))
    assert out.grad_fn is None and not out.requires_grad
    with pytest.raises(ValueError, match="multiples of 4"):
        autograd.spmm_bsr(a, a.blocks, bf(b_h[:, :6]))                               # N = 6: declined up front, no library status
    for bad_blocks, bad_b in ((a.blocks, bf(b_h)[:, :4]), (a.blocks.float(), bf(b_h)), (a.blocks, bf(b_h).float()), (a.blocks[1:], bf(b_h)),
                              (a.blocks, bf(b_h)[:-16])):
        with pytest.raises(ValueError):
            autograd.spmm_bsr(a, bad_blocks, bad_b)
    with pytest.raises(ValueError):
        autograd.spmm_bsr(a, a.blocks, bf(b_h), out_dtype=torch.float16)
