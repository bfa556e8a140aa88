"""Bitwise comparison of fp32 results (REFERENCE mode's contract is "the oracle's bits", not "an equal value").

np.array_equal says -0.0 == +0.0 and, with equal_nan, that any NaN equals any NaN; a kernel that starts a sum from its first
product, or adds padding as -0, would pass it.  assert_same_bits compares the uint32 patterns wherever the expected value is not
a NaN, and requires a NaN wherever it is (the payload and sign of a NaN are not part of the contract)."""
import numpy as np

SENTINEL_BITS = 0x7FC0DEAD            # a quiet NaN with a payload no arithmetic produces: fills the gaps of strided outputs


def _f32(x):
    if hasattr(x, "detach"):          # a torch tensor, on whatever device
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    assert x.dtype == np.float32, f"expected float32, got {x.dtype}"
    return x


def assert_same_bits(got, want, what=""):
    got, want = _f32(got), _f32(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    nan = np.isnan(want)
    missing = nan & ~np.isnan(got)
    gb, wb = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = ~nan & (gb != wb)
    if missing.any() or bad.any():
        at = np.argwhere(missing | bad)[:4]
        desc = ", ".join(f"{tuple(int(i) for i in ix)}: got {got[tuple(ix)]!r} (0x{int(gb[tuple(ix)]):08x}) "
                         f"want {want[tuple(ix)]!r} (0x{int(wb[tuple(ix)]):08x})" for ix in at)
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ in their bits, {int(missing.sum())} NaNs missing; {desc}")


def sentinel_buffer(rows, cols, ld, torch, device="cuda"):
    """A [rows, ld] float32 buffer filled with SENTINEL_BITS; the caller writes through [:, :cols]."""
    buf = torch.empty((rows, ld), dtype=torch.float32, device=device)
    buf.view(torch.int32).fill_(SENTINEL_BITS)
    return buf


def assert_gap_untouched(buf, cols, what=""):
    """Columns cols.. of a strided output (and any slack after its last row) still hold SENTINEL_BITS."""
    if hasattr(buf, "detach"):
        buf = buf.detach().cpu().numpy()
    bits = np.ascontiguousarray(buf).view(np.uint32)
    gap = bits[..., cols:] if bits.ndim == 2 else bits
    assert np.all(gap == SENTINEL_BITS), f"{what}: {int((gap != SENTINEL_BITS).sum())} gap elements were written"


def assert_no_leak(got, want, what=""):
    """The bar of the FAST and bf16/MFMA paths on adversarial data: the same NaN and Inf positions (and signs of Inf) as the
    reference -- a poisoned operand that reaches no stored entry leaks nowhere -- and no -0.0 where the reference has +0.0."""
    got, want = _f32(got), _f32(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ at {np.argwhere(np.isnan(got) != np.isnan(want))[:4].tolist()}"
    inf_g, inf_w = np.isinf(got), np.isinf(want)
    assert np.array_equal(inf_g, inf_w), f"{what}: Inf positions differ at {np.argwhere(inf_g != inf_w)[:4].tolist()}"
    assert np.array_equal(np.signbit(got[inf_g]), np.signbit(want[inf_w])), f"{what}: Inf signs differ"
    neg0 = (got == 0) & np.signbit(got) & (want == 0) & ~np.signbit(want)
    assert not neg0.any(), f"{what}: -0.0 where the reference has +0.0 at {np.argwhere(neg0)[:4].tolist()}"
