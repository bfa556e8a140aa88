"""The fp8 e4m3 fused block-sparse attention forward (libmispmm_attn_fp8.so, include/mispmm_attn_fp8.h) on a machine WITHOUT a
GPU: the fifteenth library and its one export, every refusal of the entry point (they precede any device work) and of the
Python front with its text, and quantize_heads."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_attn_fp8

from test_census_cpu import _symbol_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INV, UNS = capi.OK, capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced


def test_the_library_exports_exactly_what_its_header_declares():
    assert os.path.exists(capi_attn_fp8.LIB_PATH), f"{capi_attn_fp8.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn_fp8.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_attn_fp8.SIGNATURES) == {"mispmm_attn_bsr_fp8"}
    tool = _symbol_tool()
    if tool is not None:
        out = subprocess.run([tool, "-D", "--defined-only", capi_attn_fp8.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("mispmm_")} == declared
    assert capi_attn_fp8.last_kernel() == capi_attn_fp8.lib().mispmm_last_kernel().decode()
    assert not hasattr(ctypes.CDLL(capi.LIB_PATH), "mispmm_attn_bsr_fp8")


def _call(**kw):
    a = dict(stream=None, H=2, Mb=4, K=64, bS=16, numBlocks=3, ptrs=ONE, idxs=ONE, Q=ONE, ldq=32, q_head=2048, Kmat=ONE, ldk=32, k_head=2048,
             V=ONE, ldv=16, v_head=1024, D=32, Dv=16, mask=None, scale=0.25, qs=None, ks=None, vs=None, out=ONE, ldo=16, o_head=1024, bf16=0,
             lse=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_attn_fp8.lib().mispmm_attn_bsr_fp8(*a.values())


def test_every_refusal_of_the_entry_point_in_its_order():
    err = capi_attn_fp8.last_error
    for bs in (0, 8, 17, 64):
        assert _call(bS=bs) == UNS and f"attn_bsr_fp8: only 16x16 or 32x32 blocks (got bS={bs})" in err()
    for s in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(scale=s) == INV and "attn_bsr_fp8: scale must be finite and > 0" in err()
    for kw in (dict(D=0), dict(Dv=0), dict(D=12), dict(Dv=12), dict(D=144, ldq=144, ldk=144), dict(Dv=136, ldv=136, ldo=136)):
        assert _call(**kw) == UNS and "attn_bsr_fp8: D and Dv must be multiples of 8 from 8 to 128" in err(), kw
    assert _call(K=72) == INV and "K=72 is not a multiple of the block size 16" in err()
    for d in (8, 24, 120):
        assert _call(D=d, ldq=128, ldk=128) == UNS and f"attn_bsr_fp8: D must be a multiple of 16 from 16 to 128 (got D={d})" in err()
    for name in ("ptrs", "idxs", "Q", "Kmat", "V", "out"):
        assert _call(**{name: None}) == INV and "attn_bsr_fp8: blockRowPtrs, blockColIdxs, Q, K, V or out is null" in err(), name
    for kw in (dict(ldq=16), dict(ldk=16), dict(ldv=8), dict(ldo=8)):
        assert _call(**kw) == INV and "leading dimension smaller than the width" in err(), kw
    for kw in (dict(Q=ONE + 8), dict(Kmat=ONE + 8), dict(V=ONE + 4), dict(out=ONE + 8), dict(mask=ONE + 4), dict(ldq=40), dict(ldk=40),
               dict(ldv=20), dict(ldo=18), dict(ldo=20, bf16=1), dict(q_head=8), dict(k_head=24), dict(v_head=4), dict(o_head=2),
               dict(o_head=4, bf16=1)):
        assert _call(**kw) == UNS and "must be 16-byte aligned and V 8-byte" in err(), kw
    for name in ("qs", "ks", "vs"):
        assert _call(**{name: ONE + 2}) == UNS and "q_scale, k_scale and v_scale must be 4-byte aligned" in err(), name
    for kw in (dict(Mb=1 << 22), dict(K=1 << 26), dict(K=1 << 26, D=16, ldk=16, ldv=40)):
        assert _call(**kw) == UNS and "spans 2 GiB or more" in err(), kw
    assert _call(Mb=1 << 20, H=1 << 13) == UNS and "more work units than one launch takes" in err()
    # the order: the shape before the no-op, the no-op before the pointers, the pointers before the strides, those before alignment
    assert _call(bS=8, scale=0.0) == UNS and "blocks" in err()
    assert _call(scale=0.0, D=12) == INV and "scale" in err()
    assert _call(D=12, K=72) == UNS and "multiples of 8" in err()
    assert _call(K=72, D=24) == INV and "K=72" in err()
    assert _call(D=24, H=0) == UNS and "multiple of 16" in err()
    assert _call(H=0, Q=None) == OK and _call(Mb=0, Q=None) == OK
    assert _call(Q=None, ldq=16) == INV and "null" in err()
    assert _call(ldq=16, Kmat=ONE + 8) == INV and "leading dimension" in err()
    assert _call(Kmat=ONE + 8, qs=ONE + 2) == UNS and "16-byte aligned" in err()
    assert _call(qs=ONE + 2, K=1 << 26) == UNS and "4-byte aligned" in err()


def test_the_python_front_refuses_wrong_operands_with_value_errors():
    torch = pytest.importorskip("torch")
    from mispmm import attn_bsr_fp8, ops
    from test_softmax_bsr_cpu import _OnDevice
    f = attn_bsr_fp8.attention_bsr_fp8
    dev = lambda *shape, dtype=torch.uint8: _OnDevice(torch.zeros(*shape, dtype=dtype))         # noqa: E731
    ints = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU path"):
        f(ops.DeviceBSR(32, 64, 16, 16, 2, ints, ints, None), *(torch.zeros((n, 16), dtype=torch.uint8) for n in (32, 64, 64)))
    a = ops.DeviceBSR(32, 64, 16, 16, 2, _OnDevice(ints), _OnDevice(ints), None)
    f32 = torch.float32
    q, k, v = dev(32, 16), dev(64, 16), dev(64, 8)
    bad = [(lambda: f(a, dev(32, 16, dtype=torch.int16), k, v), "q must be a torch.float8_e4m3fn tensor or its bytes"),
           (lambda: f(ops.DeviceBSR(32, 64, 16, 32, 2, a.block_row_ptrs, a.block_col_idxs, None), q, k, v), "blocks must be square"),
           (lambda: f(a, dev(2, 32, 16), k, v), "q, k and v must all be 2-D or all"),
           (lambda: f(a, dev(2, 32, 16), dev(3, 64, 16), dev(2, 64, 8)), r"k must be \[64, width\] or \[2, 64, width\]"),
           (lambda: f(a, q, _OnDevice(torch.zeros(16, dtype=torch.uint8).expand(64, 16)), v), "k must not overlap its own rows"),
           (lambda: f(a, dev(32, 24), dev(64, 24), v), "takes D in multiples of 16 up to 128, not 24"),
           (lambda: f(a, q, k, dev(64, 136)), "takes Dv in multiples of 8 up to 128, not 136"),
           (lambda: f(a, q, k, v, k_scale=dev(2, dtype=f32)), "k_scale must be a contiguous torch.float32 tensor of 1 elements"),
           (lambda: f(a, q, k, v, out_bf16=True, out=dev(32, 8, dtype=f32)), "out must be a torch.int16 tensor of shape"),
           (lambda: f(a, q, k, v, lse=dev(31, dtype=f32)), "lse must be a contiguous float32 tensor of shape")]
    for g, words in bad:
        with pytest.raises(ValueError, match=words):
            g()


def test_quantize_heads_is_its_numpy_restatement():
    torch = pytest.importorskip("torch")
    from mispmm.attn_bsr_fp8 import quantize_heads
    g = torch.Generator().manual_seed(4)
    x = torch.randn((5, 9, 24), generator=g) * torch.logspace(-5, 5, 5)[:, None, None]
    x[2] = 0.0
    q, scale = quantize_heads(x)
    assert q.dtype == torch.float8_e4m3fn and q.shape == x.shape and scale.dtype == torch.float32 and scale.shape == (5,)
    xn = x.numpy()
    absmax = np.abs(xn).max(axis=(1, 2))
    want_scale = np.where(absmax > 0, absmax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    assert np.array_equal(scale.numpy(), want_scale) and scale[2] == 1.0 and not q[2].view(torch.uint8).any()
    want = torch.from_numpy(np.clip(xn / want_scale[:, None, None], -448.0, 448.0)).to(torch.float8_e4m3fn)
    assert torch.equal(q.view(torch.uint8), want.view(torch.uint8))
    q2, s2 = quantize_heads(x[1])                                         # a 2-D x is one head
    assert q2.shape == x[1].shape and torch.equal(q2.view(torch.uint8), q[1].view(torch.uint8)) and torch.equal(s2, scale[1:2])
