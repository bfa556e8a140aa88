"""The fp8 e4m3 product on column-compacted strips (libmispmm_bsrc_fp8.so, include/mispmm_bsrc_fp8.h) on a machine WITHOUT a
GPU: the fourteenth library and its two exports, every refusal of the device entry (they precede any device work) and of the
Python front, and the host helper against a numpy restatement.  strips_matrix() and to_bsr() also serve tests/test_gpu_bsrc_fp8.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_bsr_fp8, capi_bsrc_fp8, formats

from test_census_cpu import _symbol_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INV, UNS = capi.OK, capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced
PAD = 0xFFFFFFFF
K = 256                                    # 16 block columns of 16
# occupied columns per 16-row strip: empty, one, a full step, a second step nearly all padding, four full slots, empty | one
# extra step, four extra steps (wave 1 runs two).  The first six strips have no extra step; the last one uses column K - 1
COUNTS = (0, 1, 32, 33, 128, 0, 129, 225)


def strips_matrix(values):
    """[128, K] uint8: strip R holds COUNTS[R] occupied columns, about half the rows of each filled from values(shape)."""
    rng = np.random.default_rng(3)
    a = np.zeros((16 * len(COUNTS), K), dtype=np.uint8)
    for r, n in enumerate(COUNTS):
        cols = np.sort(rng.choice(K - 1, n, replace=False))
        cols[-1:] = K - 1 if r == len(COUNTS) - 1 else cols[-1:]
        keep = rng.random((16, n)) < 0.5
        keep[rng.integers(0, 16, n), np.arange(n)] = True                    # no column without a value
        a[16 * r:16 * r + 16, cols] = np.where(keep, values((16, n)), 0)
    return a


def to_bsr(a, bs):
    """(formats.BSR without data, blocks [num_blocks, bs, bs] uint8) of the dense bytes a: the blocks that hold a value."""
    import torch
    m, k = a.shape
    t = a.reshape(m // bs, bs, k // bs, bs).transpose(0, 2, 1, 3)
    keep = (t & 0x7F).any(axis=(2, 3))
    ptrs = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.uint32)
    return formats.BSR(m, k, 0, bs, bs, ptrs, np.nonzero(keep)[1].astype(np.uint32), None), torch.from_numpy(t[keep].copy())


def restated(a):
    """mispmm_bsr_compact_slots_fp8_host in numpy, from the dense bytes: (nSteps, used, extraPtrs, cols, tiles)."""
    strips = a.reshape(-1, 16, a.shape[1])
    occ = [np.flatnonzero((s & 0x7F).any(axis=0)) for s in strips]
    steps = np.array([-(-len(o) // 32) for o in occ])
    ep = np.concatenate([[0], np.cumsum(np.maximum(steps - 4, 0))])
    cols, tiles = np.full((4 * len(occ) + ep[-1], 32), PAD, dtype=np.uint32), np.zeros((4 * len(occ) + ep[-1], 16, 32), dtype=np.uint8)
    for r, o in enumerate(occ):
        for s in range(steps[r]):
            at, part = (4 * r + s if s < 4 else 4 * len(occ) + ep[r] + s - 4), o[32 * s:32 * s + 32]
            cols[at, :len(part)], tiles[at, :, :len(part)] = part, strips[r][:, part]
    return len(cols), int(steps.sum()), ep.astype(np.uint32), cols, tiles


def test_the_library_exports_exactly_what_its_header_declares():
    with open(os.path.join(ROOT, "include", "mispmm_bsrc_fp8.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_bsrc_fp8.SIGNATURES) == {"mispmm_bsr_compact_slots_fp8_host", "mispmm_bsrc_slots_fp8"}
    tool = _symbol_tool()
    if tool is not None:
        out = subprocess.run([tool, "-D", "--defined-only", capi_bsrc_fp8.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("mispmm_")} == declared
    assert capi_bsrc_fp8.last_kernel() == capi_bsrc_fp8.lib().mispmm_last_kernel().decode()
    for other in (capi.LIB_PATH, capi_bsr_fp8.LIB_PATH):
        assert not any(hasattr(ctypes.CDLL(other), name) for name in declared), other


def _call(**kw):
    a = dict(stream=None, strips=4, K=64, nSteps=16, ep=ONE, cols=ONE, tiles=ONE, B=ONE, N=8, ldb=8, rs=None, cs=None, C=ONE, ldc=8, bf16=0)
    a.update(kw)
    return capi_bsrc_fp8.lib().mispmm_bsrc_slots_fp8(*a.values())


def test_every_refusal_of_the_entry_point_in_its_order():
    err = capi_bsrc_fp8.last_error
    for name in ("ep", "cols", "tiles", "B", "C"):
        assert _call(**{name: None}) == INV and "bsrc_slots_fp8: null pointer" in err(), name
    for kw in (dict(N=12, ldb=16, ldc=16), dict(ldb=12), dict(ldc=20), dict(N=4, ldb=4, ldc=4)):
        assert _call(**kw) == UNS and "N, ldb and ldc must be multiples of 8" in err(), kw
    for kw in (dict(N=16), dict(N=16, ldb=16), dict(N=16, ldc=16)):
        assert _call(**kw) == INV and "leading dimension smaller than N" in err(), kw
    for kw in (dict(tiles=ONE + 4), dict(B=ONE + 4), dict(C=ONE + 8), dict(ep=ONE + 2), dict(cols=ONE + 1), dict(rs=ONE + 2), dict(cs=ONE + 1)):
        assert _call(**kw) == UNS and "tiles and B must be 8-byte aligned, C 16-byte, extraPtrs, cols and the scales 4-byte" in err(), kw
    assert _call(K=1 << 21, ldb=1 << 10) == UNS and "B spans 2 GiB or more" in err()
    for kw in (dict(strips=1 << 28, nSteps=1 << 30), dict(strips=1 << 27, nSteps=1 << 29, N=1 << 12, ldb=1 << 12, ldc=1 << 12)):
        assert _call(**kw) == UNS and "exceed the grid" in err(), kw
    assert _call(nSteps=15) == INV and "nSteps 15 is less than 4 slots per strip" in err()
    # the order: each refusal with the defect of the next one present as well
    assert _call(B=None, N=12) == INV and "null" in err()
    assert _call(N=12, ldb=8, ldc=8) == UNS and "multiples of 8" in err()
    assert _call(N=16, B=ONE + 4) == INV and "leading dimension" in err()
    assert _call(B=ONE + 4, K=1 << 21, ldb=1 << 10) == UNS and "aligned" in err()
    assert _call(K=1 << 21, ldb=1 << 10, strips=1 << 28) == UNS and "2 GiB" in err()
    assert _call(strips=1 << 28, nSteps=15) == UNS and "grid" in err()
    assert _call(strips=0, nSteps=0) == OK and _call(N=0, ldb=0, ldc=0) == OK and _call(strips=0, B=None) == INV


@pytest.mark.parametrize("bs", [16, 32])
def test_the_host_helper_lays_the_strips_out_as_its_numpy_restatement(bs):
    torch = pytest.importorskip("torch")
    from mispmm import bsrc_fp8
    a = strips_matrix(lambda shape: np.full(shape, 0x38, dtype=np.uint8))
    only = int(np.flatnonzero(a[16:32].any(axis=0))[0])                     # the one occupied column of strip 1
    a[16:32, only] = 0
    a[18, only], a[19, only ^ 1], a[20, only ^ 1] = 0x7F, 0x80, 0x00         # a NaN-only column; +-0 alone beside it in the same block
    a[:] = np.where(a == 0x38, np.random.default_rng(4).integers(1, 0x7F, a.shape), a)
    bsr, blocks = to_bsr(a, bs)
    d = bsrc_fp8.DeviceBSRCSlotsFP8.from_blocks(bsr, blocks, device="cpu")
    n_steps, used, ep, cols, tiles = restated(a)
    assert (d.num_steps, d.used_steps) == (n_steps, used) == (4 * 8 + 5, 1 + 1 + 2 + 4 + 5 + 8)
    assert np.array_equal(d.extra_ptrs.numpy().view(np.uint32), ep) and list(ep[-3:]) == [0, 1, 5]
    got_cols = d.cols.numpy().view(np.uint32).reshape(-1, 32)
    assert np.array_equal(got_cols, cols) and np.array_equal(d.tiles.numpy(), tiles)
    assert list(got_cols[4]) == [only] + [PAD] * 31 and (got_cols[0] == PAD).all() and got_cols[4 * 8 + 4, 0] != PAD
    live = np.where(got_cols == PAD, np.uint64(1) << 40, got_cols)
    assert (np.diff(live.astype(np.int64), axis=1) >= 0).all(), "ascending, padding behind"
    typed = bsrc_fp8.DeviceBSRCSlotsFP8.from_blocks(bsr, blocks.view(torch.float8_e4m3fn), device="cpu")
    assert torch.equal(typed.tiles, d.tiles)
    bsr.block_col_idxs[-1] = K // bs                                        # the ingest's checks and messages
    with pytest.raises(capi.MispmmError, match=rf"bsr check: blockColIdxs\[{bsr.num_blocks - 1}\] = {K // bs} is not below K / bC = {K // bs}"):
        bsrc_fp8.DeviceBSRCSlotsFP8.from_blocks(bsr, blocks, device="cpu")
    assert capi_bsrc_fp8.lib().mispmm_bsr_compact_slots_fp8_host(1, 16, 8, 0, ONE, ONE, ONE, ctypes.byref(ctypes.c_uint32()), None, None, None, None) == UNS
    assert "only 16x16 or 32x32 blocks (got 8x8)" in capi_bsrc_fp8.last_error()


def test_the_python_front_quantises_rows_and_refuses_wrong_operands():
    torch = pytest.importorskip("torch")
    from mispmm import bsrc_fp8
    from test_softmax_bsr_cpu import _OnDevice
    bsr, blocks = to_bsr(strips_matrix(lambda shape: np.full(shape, 0x38, dtype=np.uint8)), 16)
    rng = np.random.default_rng(6)
    bsr.data = rng.uniform(-3, 3, (bsr.num_blocks, 16, 16)).astype(np.float32) * (blocks.numpy() != 0)
    d = bsrc_fp8.DeviceBSRCSlotsFP8.from_host(bsr, device="cpu")
    absmax = np.abs(bsr.to_dense()).max(axis=1)
    assert np.array_equal(d.row_scale.numpy(), np.where(absmax > 0, absmax / np.float32(448.0), np.float32(1.0)))
    assert d.tiles.view(torch.float8_e4m3fn).float().abs().max() == 448.0 and d.used_steps == 21
    f, from_blocks = bsrc_fp8.spmm_bsrc_slots_fp8, bsrc_fp8.DeviceBSRCSlotsFP8.from_blocks
    dev = lambda *shape, dtype=torch.uint8: _OnDevice(torch.zeros(*shape, dtype=dtype))         # noqa: E731
    with pytest.raises(ValueError, match="no CPU path"):
        f(d, torch.zeros((K, 8), dtype=torch.uint8))
    d.extra_ptrs = _OnDevice(d.extra_ptrs)
    bad = [(lambda: from_blocks(bsr, blocks.to(torch.int8)), "blocks_fp8 must be a torch.float8_e4m3fn tensor or its bytes"),
           (lambda: from_blocks(formats.BSR(128, K, 0, 16, 32, bsr.block_row_ptrs, bsr.block_col_idxs, None), blocks), "blocks must be square"),
           (lambda: from_blocks(bsr, blocks[1:]), f"blocks_fp8 must be a contiguous host tensor of {blocks.numel()} elements"),
           (lambda: f(d, dev(K, 8, dtype=torch.float8_e5m2)), "b_fp8 must be a torch.float8_e4m3fn tensor or its bytes"),
           (lambda: f(d, dev(K - 1, 8)), f"b_fp8 has {K - 1} rows, A has {K} columns"),
           (lambda: f(d, dev(K, 8), row_scale=dev(127, dtype=torch.float32)), "row_scale must be a contiguous torch.float32 tensor of 128"),
           (lambda: f(d, dev(K, 8), col_scale=dev(9, dtype=torch.float32)), "col_scale must be a contiguous torch.float32 tensor of 8"),
           (lambda: f(d, dev(K, 8), out=dev(128, 16, dtype=torch.float32)), r"out has shape \(128, 16\), expected \(128, 8\)")]
    for g, words in bad:
        with pytest.raises(ValueError, match=words):
            g()
