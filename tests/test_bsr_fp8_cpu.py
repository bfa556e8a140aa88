"""The fp8 e4m3 block-sparse product (libmispmm_bsr_fp8.so, include/mispmm_bsr_fp8.h) on a machine WITHOUT a GPU: the
thirteenth library and its one export, every refusal of the entry point (they precede any device work) and of the Python
front with its text, and quantize_rows."""
import ctypes
import os
import re
import subprocess

import pytest

from mispmm import capi, capi_bsr_fp8

from test_census_cpu import _symbol_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INV, UNS = capi.OK, capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced


def test_the_library_exports_exactly_what_its_header_declares():
    assert os.path.exists(capi_bsr_fp8.LIB_PATH), f"{capi_bsr_fp8.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_bsr_fp8.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_bsr_fp8.SIGNATURES) == {"mispmm_bsr_fp8"}
    tool = _symbol_tool()
    if tool is not None:
        out = subprocess.run([tool, "-D", "--defined-only", capi_bsr_fp8.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("mispmm_")} == declared
    assert capi_bsr_fp8.last_kernel() == capi_bsr_fp8.lib().mispmm_last_kernel().decode()
    assert not hasattr(ctypes.CDLL(capi.LIB_PATH), "mispmm_bsr_fp8")


def _call(**kw):
    a = dict(stream=None, Mb=4, K=64, bS=16, numBlocks=3, ptrs=ONE, idxs=ONE, blocks=ONE, B=ONE, N=8, ldb=8, rs=None, cs=None, C=ONE, ldc=8, bf16=0)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_bsr_fp8.lib().mispmm_bsr_fp8(*a.values())


def test_every_refusal_of_the_entry_point_in_its_order():
    err = capi_bsr_fp8.last_error
    for name in ("ptrs", "B", "C"):
        assert _call(**{name: None}) == INV and "bsr_fp8: blockRowPtrs, B or C is null" in err(), name
    for name in ("idxs", "blocks"):
        assert _call(**{name: None}) == INV and "bsr_fp8: blockColIdxs or blocks is null" in err(), name
        assert _call(**{name: None}, numBlocks=0, Mb=0) == OK
    for bs in (0, 8, 17, 64):
        assert _call(bS=bs) == UNS and f"only 16x16 or 32x32 blocks (got {bs}x{bs})" in err()
    for kw in (dict(N=12, ldb=16, ldc=16), dict(ldb=12), dict(ldc=20), dict(N=4, ldb=4, ldc=4)):
        assert _call(**kw) == UNS and "N, ldb and ldc must be multiples of 8" in err(), kw
    for kw in (dict(N=16), dict(N=16, ldb=16), dict(N=16, ldc=16)):
        assert _call(**kw) == INV and "leading dimension smaller than N" in err(), kw
    for kw in (dict(blocks=ONE + 4), dict(B=ONE + 4), dict(C=ONE + 8), dict(rs=ONE + 2), dict(cs=ONE + 1)):
        assert _call(**kw) == UNS and "8-byte aligned, C 16-byte, the scales 4-byte" in err(), kw
    assert _call(K=1 << 21, ldb=1 << 10) == UNS and "B spans 2 GiB or more" in err()
    assert _call(Mb=0xFFFFFFFF, N=1 << 10, ldb=1 << 10, ldc=1 << 10) == UNS and "exceed the grid" in err()
    # the order: a null pointer before the block size, the block size before the multiples of 8, those before the leading dimensions
    assert _call(B=None, bS=8) == INV and "null" in err()
    assert _call(bS=8, N=12) == UNS and "blocks" in err()
    assert _call(N=12, ldb=8, ldc=8) == UNS and "multiples of 8" in err()
    assert _call(N=16, B=ONE + 4) == INV and "leading dimension" in err()
    # nothing to do is a no-op only once the shape has passed
    assert _call(Mb=0) == OK and _call(N=0, ldb=0, ldc=0) == OK and _call(Mb=0, bS=8) == UNS


def test_the_python_front_refuses_wrong_operands_with_value_errors():
    torch = pytest.importorskip("torch")
    from mispmm import bsr_fp8, ops
    from test_softmax_bsr_cpu import _OnDevice
    f = bsr_fp8.spmm_bsr_fp8
    dev = lambda *shape, dtype=torch.uint8: _OnDevice(torch.zeros(*shape, dtype=dtype))         # noqa: E731
    ints = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU path"):
        f(ops.DeviceBSR(32, 64, 16, 16, 2, ints, ints, None), torch.zeros(512, dtype=torch.uint8), torch.zeros((64, 8), dtype=torch.uint8))
    a = ops.DeviceBSR(32, 64, 16, 16, 2, _OnDevice(ints), _OnDevice(ints), None)
    f32 = torch.float32
    bad = [(lambda: f(a, dev(512, dtype=torch.int8), dev(64, 8)), "blocks_fp8 must be a torch.float8_e4m3fn tensor or its bytes"),
           (lambda: f(a, dev(512), dev(64, 8, dtype=torch.float8_e5m2)), "b_fp8 must be a torch.float8_e4m3fn tensor or its bytes"),
           (lambda: f(ops.DeviceBSR(32, 64, 16, 32, 2, a.block_row_ptrs, a.block_col_idxs, None), dev(1024), dev(64, 8)), "blocks must be square"),
           (lambda: f(a, dev(511), dev(64, 8)), "blocks_fp8 must be a contiguous torch.uint8 tensor of 512 elements"),
           (lambda: f(a, dev(512), dev(63, 8)), "b_fp8 has 63 rows, A has 64 columns"),
           (lambda: f(a, dev(512), _OnDevice(torch.zeros((8, 64), dtype=torch.uint8).t())), "b_fp8 must be a 2-D tensor of fp8 e4m3 bytes"),
           (lambda: f(a, dev(512), _OnDevice(torch.zeros(8, dtype=torch.uint8).expand(64, 8))), "b_fp8 must not overlap its own rows"),
           (lambda: f(a, dev(512), dev(64, 8), row_scale=dev(31, dtype=f32)), "row_scale must be a contiguous torch.float32 tensor of 32"),
           (lambda: f(a, dev(512), dev(64, 8), out_bf16=True, out=dev(32, 8, dtype=f32)), "out must be a 2-D int16 tensor of bf16 bits"),
           (lambda: f(a, dev(512), dev(64, 8), out=dev(32, 16, dtype=f32)), r"out has shape \(32, 16\), expected \(32, 8\)")]
    for g, words in bad:
        with pytest.raises(ValueError, match=words):
            g()


def test_quantize_rows_round_trips_within_half_an_e4m3_ulp_and_scales_a_zero_row_by_one():
    torch = pytest.importorskip("torch")
    from mispmm.bsr_fp8 import quantize_rows
    g = torch.Generator().manual_seed(2)
    x = torch.randn((33, 70), generator=g) * torch.logspace(-6, 6, 33)[:, None]
    x[5] = 0.0
    x[7, 3] = 0.0
    q, scale = quantize_rows(x)
    assert q.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and scale.shape == (33,)
    assert scale[5] == 1.0 and not q[5].view(torch.uint8).any()
    live = torch.arange(33) != 5
    assert torch.equal(scale[live], x[live].abs().amax(dim=1) / 448.0) and bool((q.to(torch.float32).abs().amax(dim=1)[live] == 448.0).all())
    # half an ulp of the scaled value y: 2^(floor(log2 |y|) - 3) / 2 with 3 mantissa bits, 2^-9 / 2 among the subnormals
    y = (x / scale[:, None]).to(torch.float64)
    ulp = 2.0 ** (torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -6))) - 3)
    assert bool(((q.to(torch.float64) - y).abs() <= ulp / 2).all())
    qt, st = quantize_rows(x.t())                                      # B's columns through a transpose
    assert qt.t().shape == x.shape and st.shape == (70,) and not qt.to(torch.float32).isnan().any()
