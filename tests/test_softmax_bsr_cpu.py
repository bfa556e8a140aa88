"""Row softmax on a BSR pattern on a machine WITHOUT a GPU: the numpy restatement of the contract against torch.softmax on the
densified rows, the stated bounds against a plain float32 restatement (they must be satisfiable by a correct implementation),
the entry points' argument validation (which happens before any device work) and the Python layer's refusals."""
import ctypes

import numpy as np
import pytest

from mispmm import capi, ops

from _fma_chain import fma_exact
from _softmax_bsr_ref import (EDGE_UNSORTED, HELD, assert_inside, backward, backward_f32, bf16_round, bwd_bound, causal_mask,
                              edge_counts, fma32, forward, forward_f32, full_mantissa, fwd_bound, layout, lengths, pattern,
                              random_mask, row_sums, scores, to_rows, z_values)

PATTERNS = ["edges16", "edges32", "ragged16", "ragged32"]


def test_the_edge_patterns_hold_the_block_rows_they_claim():
    for bs in (16, 32):
        p = pattern(f"edges{bs}")
        c = HELD[bs]
        ptrs = p.block_row_ptrs.astype(np.int64)
        counts = np.diff(ptrs).tolist()
        assert counts == edge_counts(bs) == [0, 1, 2, 3, 4, 5, 8, 9, c - 1, c, c + 1, 2 * c + 1, 0]
        assert p.block_row_size == p.block_col_size == bs and counts[-1] == 0
        unsorted = [r for r in range(len(counts)) if np.any(np.diff(p.block_col_idxs[ptrs[r]:ptrs[r + 1]].astype(np.int64)) < 0)]
        assert tuple(unsorted) == EDGE_UNSORTED
    assert HELD[16] >= 27                      # ACTIVSg10K's mean block row (26.5 blocks of 16 x 16) is held


def test_layout_lists_every_element_once_row_by_row():
    for name in PATTERNS:
        p = pattern(name)
        bs = p.block_row_size
        row_ptrs, idx = layout(name)
        assert np.array_equal(np.sort(idx), np.arange(p.num_blocks * bs * bs))
        assert row_ptrs.shape[0] == p.num_rows + 1 and row_ptrs[-1] == idx.shape[0]
        e, rest = np.divmod(idx, bs * bs)
        i = rest // bs
        ptrs = p.block_row_ptrs.astype(np.int64)
        block_row = np.searchsorted(ptrs, e, side="right") - 1
        row = np.repeat(np.arange(p.num_rows), np.diff(row_ptrs))
        assert np.array_equal(block_row * bs + i, row)                       # matrix row R * bS + i owns element row i of its blocks
        assert np.array_equal(np.diff(row_ptrs), np.repeat(np.diff(ptrs) * bs, bs))
        assert np.array_equal(to_rows(name, lengths(name)), np.repeat(np.diff(row_ptrs), np.diff(row_ptrs)))


def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(3)
    a = full_mantissa(rng, 400)
    c = (full_mantissa(rng, 400) * np.float32(2.0) ** rng.integers(-30, 4, 400)).astype(np.float32)
    for scale in (np.float32(0.3), np.float32(0.125), np.float32(1.0)):
        want = np.array([fma_exact(scale, x, y, np.float32) for x, y in zip(a, c)], np.float32)
        assert np.array_equal(fma32(scale, a, c), want)
    # a * b = 2^-24 - 2^-70 and c = 1 + 2^-23: the exact sum lies just below the tie between 1 + 2^-23 and 1 + 2^-22, the
    # float64 sum ON it -- rounding twice goes to the even neighbour, 1 + 2^-22
    a, b, c = np.float32(2.0 ** -12 + 2.0 ** -35), np.float32(2.0 ** -12 - 2.0 ** -35), np.float32(1.0 + 2.0 ** -23)
    assert fma32(a, b, c)[()] == np.float32(fma_exact(a, b, c, np.float32)) == np.float32(1.0 + 2.0 ** -23)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(1.0 + 2.0 ** -22)
    assert np.isneginf(fma32(np.float32(0.3), np.float32(1.0), np.float32(-np.inf)))
    assert np.isnan(fma32(np.float32(0.3), np.float32(np.inf), np.float32(-np.inf)))


def _dense_rows(name, z):
    """[M, K] float64 with -Inf where A stores nothing, NaN-free unless z has one; and which rows store anything."""
    p = pattern(name)
    bs = p.block_row_size
    ptrs = p.block_row_ptrs.astype(np.int64)
    dense = np.full((p.num_rows, p.num_cols), -np.inf)
    for r in range(ptrs.shape[0] - 1):
        for e in range(ptrs[r], ptrs[r + 1]):
            c = int(p.block_col_idxs[e])
            dense[r * bs:(r + 1) * bs, c * bs:(c + 1) * bs] = z[e]
    return dense, np.repeat(np.diff(ptrs) > 0, bs)


def _undense(name, dense):
    p = pattern(name)
    bs = p.block_row_size
    ptrs = p.block_row_ptrs.astype(np.int64)
    out = np.empty((p.num_blocks, bs, bs))
    for r in range(ptrs.shape[0] - 1):
        for e in range(ptrs[r], ptrs[r + 1]):
            c = int(p.block_col_idxs[e])
            out[e] = dense[r * bs:(r + 1) * bs, c * bs:(c + 1) * bs]
    return out


@pytest.mark.parametrize("name", ["ragged16", "ragged32", "edges16"])
def test_restatement_is_torch_softmax_on_the_densified_rows(name):
    """Special values included: a NaN, a +Inf and an all -Inf row each make exactly their matrix row NaN -- the other rows of
    the same blocks stay -- and a -Inf beside a finite value is exactly +0."""
    torch = pytest.importorskip("torch")
    p = pattern(name)
    bs = p.block_row_size
    ptrs = p.block_row_ptrs.astype(np.int64)
    z = z_values(scores("narrow", name), random_mask(name), 0.3)
    full = [r for r in range(ptrs.shape[0] - 1) if ptrs[r + 1] - ptrs[r] >= 2][:3]
    assert len(full) == 3
    z[ptrs[full[0]] + 1, 3, 5] = np.nan
    z[ptrs[full[1]], bs - 1, 0] = np.inf
    z[ptrs[full[2]]:ptrs[full[2] + 1], 7, :] = -np.inf
    dead_rows = {full[0] * bs + 3, full[1] * bs + bs - 1, full[2] * bs + 7}
    got = forward(name, z, np.float64)[0]
    dense, stored = _dense_rows(name, z)
    want = _undense(name, torch.softmax(torch.from_numpy(dense), dim=1).numpy())
    assert np.array_equal(np.isnan(got), np.isnan(want))
    row_ptrs, _ = layout(name)
    nan_rows = set(np.repeat(np.arange(p.num_rows), np.diff(row_ptrs))[np.isnan(to_rows(name, got))].tolist())
    assert nan_rows == dead_rows
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=1e-14, atol=0)
    masked = np.isneginf(z) & ok
    assert masked.sum() > z.size // 8 and not got[masked].any() and not np.signbit(got[masked]).any()
    assert stored.sum() < p.num_rows                                          # some matrix rows store nothing: not in the arrays at all


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("kind", ["narrow", "wide", "equal"])
@pytest.mark.parametrize("name", PATTERNS)
def test_a_plain_float32_softmax_lies_inside_every_stated_bound(name, kind, with_mask):
    """The bounds are satisfiable: numpy's float32 arithmetic taken alone (exp, a left-to-right sum, division; the backward
    with rounded products), and its result rounded to bf16, stay inside them on every pattern and generator the GPU tests use."""
    length = lengths(name)
    for scale in (1.0, 0.125, 0.3):
        z = z_values(scores(kind, name), random_mask(name) if with_mask else None, scale)
        exact, t = forward(name, z)
        p32 = forward_f32(name, z)
        what = f"float32 numpy {name} {kind} mask={with_mask} scale={scale}"
        assert assert_inside(p32, exact, fwd_bound(False, length, t, exact), f"{what} forward") <= 1.0
        assert_inside(bf16_round(p32), exact, fwd_bound(True, length, t, exact), f"{what} forward bf16")
        sums, lens = row_sums(name, p32)
        assert np.all(np.abs(sums - 1) <= lens * 2.0 ** -24)
        dp = full_mantissa(np.random.default_rng(5), z.shape)
        for p in (p32, bf16_round(p32)):
            ds_exact, cap = backward(name, p, dp, scale)
            ds = backward_f32(name, p, dp, scale)
            assert_inside(ds, ds_exact, bwd_bound(False, length, p, dp, cap, scale, ds_exact), f"{what} backward")
            assert_inside(bf16_round(ds), ds_exact, bwd_bound(True, length, p, dp, cap, scale, ds_exact), f"{what} backward bf16")


def test_equal_scores_give_the_correctly_rounded_quotient():
    """exp2(0) = 1, the sum of L ones is exact, so the fp32 arithmetic of the kernel gives fl32(1 / L): what the GPU anchor
    compares with."""
    for name in PATTERNS:
        z = z_values(scores("equal", name), None, 0.3)
        length = lengths(name)
        assert np.array_equal(forward_f32(name, z), (np.float32(1.0) / length.astype(np.float32)).astype(np.float32))


def test_the_causal_mask_hides_the_upper_triangle_of_the_diagonal_blocks():
    for name in PATTERNS:
        p = pattern(name)
        m = causal_mask(name)
        ptrs = p.block_row_ptrs.astype(np.int64)
        rows = np.repeat(np.arange(ptrs.shape[0] - 1), np.diff(ptrs))
        diag = p.block_col_idxs.astype(np.int64) == rows
        assert diag.any() and not m[~diag].any()
        assert np.all(np.isneginf(m[diag]) == np.triu(np.ones(m.shape[1:], bool), k=1))


@pytest.mark.parametrize("fn", ["mispmm_softmax_bsr_f32", "mispmm_softmax_bsr_bwd_f32"])
def test_softmax_bsr_validates_before_any_device_work(fn):
    l = capi.lib()
    bwd = "_bwd_" in fn
    one = ctypes.c_void_p(16)   # never dereferenced: every call below must return from validation

    def call(mb, bs, nb, ptrs, a, b, scale, out, flag=0):
        if bwd:      # stream Mb bS nb rowPtrs p p_bf16 dp scale ds ds_bf16
            return getattr(l, fn)(None, mb, bs, nb, ptrs, a, flag, b, scale, out, flag)
        return getattr(l, fn)(None, mb, bs, nb, ptrs, a, b, scale, out, flag)    # b: the mask
    assert call(4, 16, 3, None, one, one, 1.0, one) == capi.ERR_INVALID_ARG
    assert call(4, 16, 3, one, None, one, 1.0, one) == capi.ERR_INVALID_ARG
    assert call(4, 32, 3, one, one, one, 1.0, None, 1) == capi.ERR_INVALID_ARG
    if bwd:
        assert call(4, 16, 3, one, one, None, 1.0, one) == capi.ERR_INVALID_ARG
    assert b"null" in l.mispmm_last_error() and fn[len("mispmm_"):].encode() in l.mispmm_last_error()
    for bs in (0, 1, 8, 17, 48, 64):
        assert call(4, bs, 3, one, one, one, 1.0, one) == capi.ERR_UNSUPPORTED
        assert b"16x16 or 32x32" in l.mispmm_last_error()
    for scale in (0.0, -1.0, float("inf"), float("nan"), -float("inf")):
        for bs in (16, 32):
            assert call(4, bs, 3, one, one, one, scale, one) == capi.ERR_INVALID_ARG
            assert b"scale" in l.mispmm_last_error()
    assert call(4, 16, 0, one, one, one, float("nan"), one) == capi.ERR_INVALID_ARG       # the scale is checked even for a no-op
    assert call(4, 16, 0, one, None, None, 0.5, None) == capi.OK                           # numBlocks == 0: a no-op
    assert call(0, 32, 0, None, None, None, 1.0, None, 1) == capi.OK                       # numBlockRows == 0
    assert call(0, 16, 5, None, None, None, 1.0, None) == capi.OK
    if not bwd:
        # a null mask is no error: with every other pointer null the refusal names those, never the mask
        assert call(4, 16, 3, None, None, None, 1.0, None) == capi.ERR_INVALID_ARG
        assert b"mask" not in l.mispmm_last_error()


def test_python_layer_without_a_gpu():
    torch = pytest.importorskip("torch")
    from mispmm import autograd
    bsr = pattern("ragged16")
    a = ops.DeviceBSR.from_host(bsr, device="cpu")
    s = torch.zeros((bsr.num_blocks, 16, 16))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.softmax_bsr(a, s)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.softmax_bsr(a, s, mask=s, out_bf16=True)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.softmax_bsr_bwd(a, s, s)
    t = autograd.TrainableBSR.from_host(bsr, device="cpu")
    q, k = torch.zeros((bsr.num_rows, 8), dtype=torch.bfloat16), torch.zeros((bsr.num_cols, 8), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.block_softmax(t, s)
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.block_sparse_attention(t, q, k, k)


class _OnDevice:
    """A stand-in that says it lives on the device, so that the checks behind the CPU refusal can run here; every call
    below must raise before anything would be read."""
    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_wrong_dtypes_shapes_and_strides_are_refused():
    torch = pytest.importorskip("torch")
    from mispmm import autograd
    bsr = pattern("ragged16")
    t = autograd.TrainableBSR.from_host(bsr, device="cpu")
    t.fwd.block_row_ptrs = _OnDevice(t.fwd.block_row_ptrs)
    dev = lambda *shape, dtype=torch.float32: _OnDevice(torch.zeros(*shape, dtype=dtype))   # noqa: E731
    bf = torch.bfloat16
    nb, m, k = bsr.num_blocks, bsr.num_rows, bsr.num_cols
    strided = lambda dtype=torch.float32: _OnDevice(torch.zeros((nb, 16, 32), dtype=dtype)[:, :, ::2])   # noqa: E731
    bad = [lambda: ops.softmax_bsr(t.fwd, dev(nb, 16, 16, dtype=torch.float64)),
           lambda: ops.softmax_bsr(t.fwd, dev(nb, 16, 16, dtype=torch.int16)),
           lambda: ops.softmax_bsr(t.fwd, dev(nb + 1, 16, 16)),
           lambda: ops.softmax_bsr(t.fwd, dev(nb, 256)),
           lambda: ops.softmax_bsr(t.fwd, dev(nb, 32, 32)),
           lambda: ops.softmax_bsr(t.fwd, strided()),
           lambda: ops.softmax_bsr(t.fwd, dev(nb, 16, 16), mask=dev(nb, 16, 16, dtype=torch.bool)),
           lambda: ops.softmax_bsr(t.fwd, dev(nb, 16, 16), mask=dev(nb, 16)),
           lambda: ops.softmax_bsr(t.fwd, dev(nb, 16, 16), mask=strided()),
           lambda: ops.softmax_bsr(t.fwd, dev(nb, 16, 16), out=dev(nb, 16, 16, dtype=torch.int16)),             # fp32 asked for
           lambda: ops.softmax_bsr(t.fwd, dev(nb, 16, 16), out_bf16=True, out=dev(nb, 16, 16)),
           lambda: ops.softmax_bsr(t.fwd, dev(nb, 16, 16), out=dev(nb - 1, 16, 16)),
           lambda: ops.softmax_bsr_bwd(t.fwd, dev(nb, 16, 16, dtype=torch.float16), dev(nb, 16, 16)),
           lambda: ops.softmax_bsr_bwd(t.fwd, dev(nb, 16, 16), dev(nb, 16, 16, dtype=torch.int16)),             # dp is fp32 only
           lambda: ops.softmax_bsr_bwd(t.fwd, dev(nb, 16, 16, dtype=torch.int16), dev(nb, 16, 15)),
           lambda: ops.softmax_bsr_bwd(t.fwd, strided(torch.int16), dev(nb, 16, 16)),
           lambda: ops.softmax_bsr_bwd(t.fwd, dev(nb, 16, 16), dev(nb, 16, 16), out=dev(nb, 16, 16, dtype=torch.int16)),
           lambda: ops.softmax_bsr_bwd(t.fwd, dev(nb, 16, 16), dev(nb, 16, 16), out_bf16=True, out=dev(nb, 16, 16)),
           lambda: autograd.block_softmax(t, dev(nb, 16, 16, dtype=torch.float64)),
           lambda: autograd.block_softmax(t, dev(nb, 256)),
           lambda: autograd.block_softmax(t, dev(nb, 16, 16), mask=dev(nb, 16, 16, dtype=torch.float64)),
           lambda: autograd.block_softmax(t, dev(nb, 16, 16), out_dtype=torch.float16),
           lambda: autograd.block_sparse_attention(t, dev(m, 8), dev(k, 8, dtype=bf), dev(k, 8, dtype=bf)),
           lambda: autograd.block_sparse_attention(t, dev(m, 8, dtype=bf), dev(k, 8), dev(k, 8, dtype=bf)),
           lambda: autograd.block_sparse_attention(t, dev(m, 8, dtype=bf), dev(k, 8, dtype=bf), dev(k, 8)),
           lambda: autograd.block_sparse_attention(t, dev(m + 16, 8, dtype=bf), dev(k, 8, dtype=bf), dev(k, 8, dtype=bf)),
           lambda: autograd.block_sparse_attention(t, dev(m, 8, dtype=bf), dev(k, 4, dtype=bf), dev(k, 8, dtype=bf)),
           lambda: autograd.block_sparse_attention(t, dev(m, 6, dtype=bf), dev(k, 6, dtype=bf), dev(k, 8, dtype=bf)),
           lambda: autograd.block_sparse_attention(t, dev(m, 8, dtype=bf), dev(k, 8, dtype=bf), dev(k, 10, dtype=bf)),
           lambda: autograd.block_sparse_attention(t, dev(m, 8, dtype=bf), dev(k, 8, dtype=bf), dev(k - 16, 8, dtype=bf)),
           lambda: autograd.block_sparse_attention(t, _OnDevice(torch.zeros((8, m), dtype=bf).t()), dev(k, 8, dtype=bf), dev(k, 8, dtype=bf)),
           lambda: autograd.block_sparse_attention(t, dev(m, 8, dtype=bf), dev(k, 8, dtype=bf), dev(k, 8, dtype=bf), mask=dev(nb, 16)),
           lambda: autograd.block_sparse_attention(t, dev(m, 8, dtype=bf), dev(k, 8, dtype=bf), dev(k, 8, dtype=bf), out_dtype=torch.float64)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was not refused")
