"""Decode attention on a paged fp8 e4m3 KV cache (libmispmm_attn_fp8_decode.so, include/mispmm_attn_fp8_decode.h) on a machine
WITHOUT a GPU: the seventeenth library and its two exports, the workspace formula, every refusal of the entry point with its
text and its place in the header's order (all precede any device work), the Python front's ValueErrors and the default rule."""
import ctypes
import glob
import os
import re

import pytest

from mispmm import capi, capi_attn_fp8_decode as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INV, UNS = capi.OK, capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced
NEED = 4 * 3 * 4 * 4 * (16 + 3)            # workspace bytes of _call()'s defaults: B = 3, H = 4, 4 splits, Dv = 16
NAMES = {"mispmm_attn_decode_fp8", "mispmm_attn_decode_fp8_workspace"}


def test_the_library_exports_what_its_header_declares_and_no_other_library_does():
    assert os.path.exists(cd.LIB_PATH), f"{cd.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn_fp8_decode.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert set(re.findall(r"\b(mispmm_[a-z0-9_]+)\s*\(", text)) == set(cd.SIGNATURES) == NAMES
    lib = cd.lib()                                   # raises where an export is missing
    assert cd.last_kernel() == lib.mispmm_last_kernel().decode()
    others = [p for p in glob.glob(os.path.join(os.path.dirname(capi.LIB_PATH), "libmispmm*.so")) if "_tune" not in p and "_x_" not in p
              and "_stamps" not in p and os.path.basename(p) != os.path.basename(cd.LIB_PATH)]
    assert len(others) == 16, others
    for other in others:
        assert not any(hasattr(ctypes.CDLL(other), name) for name in NAMES), other
    for b, h, g, dv, s in [(2, 4, 2, 64, 4), (1, 1, 1, 8, 1), (3, 6, 3, 72, 3), (0, 7, 7, 8, 2), (1 << 20, 1 << 10, 16, 128, 64)]:
        assert lib.mispmm_attn_decode_fp8_workspace(b, h, g, dv, s) == 4 * b * h * s * (dv + 3)      # the G real rows: g cancels


def _call(**kw):
    a = dict(stream=None, B=3, H=4, K=64, bS=16, numPages=3, ptrs=ONE, idxs=ONE, lens=ONE, Q=ONE, ldq=128, q_head=32, Kmat=ONE, ldk=32,
             k_head=2048, V=ONE, ldv=16, v_head=1024, D=32, Dv=16, scale=0.25, qs=None, ks=None, vs=None, out=ONE, ldo=64, o_head=16, bf16=0,
             lse=None, kv_group=2, splits=4, ws=ONE, ws_bytes=NEED)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return cd.lib().mispmm_attn_decode_fp8(*a.values())


REFUSALS = [(dict(kv_group=0), INV, "kv_group must be 1 to 16 and divide H (got kv_group=0, H=4)"),
            (dict(kv_group=3), INV, "kv_group must be 1 to 16 and divide H (got kv_group=3, H=4)"),
            (dict(kv_group=17, H=34), UNS, "kv_group above 16 is not supported (got kv_group=17)"),
            (dict(splits=0), INV, "splits must be 1 to 64 (got 0)"), (dict(splits=65), INV, "splits must be 1 to 64 (got 65)"),
            (dict(ws=None), INV, f"hold {NEED} bytes (got null"), (dict(ws=ONE + 8), INV, f"hold {NEED} bytes (got a misaligned pointer"),
            (dict(ws_bytes=NEED - 1), INV, f"hold {NEED} bytes (got an aligned pointer, {NEED - 1} bytes)"),
            (dict(splits=8), INV, f"hold {2 * NEED} bytes"),
            (dict(q_head=1 << 31), UNS, "the heads of a KV group of Q, or K or V of one head, span 2 GiB or more (2147483648, "),
            (dict(B=1 << 27, splits=64, ws_bytes=1 << 62), UNS, "134217728 sequences x 4 heads x 64 splits over 3 pages are more work units"),
            (dict(numPages=1 << 27), UNS, "over 134217728 pages are more work units than one launch takes")]


@pytest.mark.parametrize("kw, status, text", REFUSALS, ids=[str(r[0]) for r in REFUSALS])
def test_a_refusal_carries_its_text_before_any_device_work(kw, status, text):
    assert _call(**kw) == status
    err = cd.last_error()
    assert err.startswith("attn_decode_fp8: ") and text in err, err


def test_the_refusals_stand_in_the_order_of_the_header():
    err = cd.last_error          # each call is wrong in its rung and in the next: shape checks, kv_group, splits, workspace, no-op, the rest
    assert _call(bS=8, scale=0.0) == UNS and "only 16x16 or 32x32 blocks (got bS=8)" in err()
    assert _call(scale=0.0, D=12) == INV and "scale must be finite and > 0" in err()
    assert _call(D=12, K=72) == UNS and "multiples of 8 from 8 to 128" in err()
    assert _call(K=72, D=24) == INV and "K=72 is not a multiple of the block size 16" in err()
    assert _call(D=24, kv_group=0) == UNS and "D must be a multiple of 16 from 16 to 128 (got D=24)" in err()
    assert _call(kv_group=0, splits=0) == INV and "kv_group=0" in err()
    assert _call(kv_group=17, splits=0) == UNS and "kv_group=17" in err()
    assert _call(kv_group=3, splits=0) == INV and "kv_group=3" in err()
    assert _call(splits=0, ws=None) == INV and "splits" in err()
    assert _call(ws=None, H=0) == INV and "hold 0 bytes (got null" in err()
    assert _call(B=0, kv_group=0) == INV and "kv_group" in err()
    nothing = dict(ptrs=None, idxs=None, lens=None, Q=None, Kmat=None, V=None, out=None, ws_bytes=0)
    assert _call(H=0, **nothing) == OK and _call(B=0, **nothing) == OK
    assert _call(ws_bytes=NEED - 1, Q=None) == INV and "workspace" in err()
    for name in ("ptrs", "idxs", "Q", "Kmat", "V", "out"):
        assert _call(**{name: None}) == INV and "pagePtrs, pageIdxs, Q, K, V or out is null" in err(), name
    assert _call(Q=None, ldq=16) == INV and "null" in err()
    assert _call(ldq=16, Kmat=ONE + 8) == INV and "leading dimension smaller than the width" in err()
    assert _call(Kmat=ONE + 8, qs=ONE + 2) == UNS and "must be 16-byte aligned and V 8-byte" in err()
    assert _call(o_head=20, bf16=1, lens=ONE + 2) == UNS and "must be 16-byte aligned and V 8-byte" in err()
    assert _call(lens=ONE + 2, K=1 << 26) == UNS and "seqLens must be 4-byte aligned" in err()
    assert _call(K=1 << 26, numPages=1 << 27) == UNS and "span 2 GiB or more" in err()


def test_the_python_front_refuses_with_value_errors_and_the_default_rule_fills_the_card():
    torch = pytest.importorskip("torch")
    from mispmm import attn_decode_fp8 as front
    from test_softmax_bsr_cpu import _OnDevice
    f = front.attention_decode_fp8
    dev = lambda *shape, dtype=torch.uint8: _OnDevice(torch.zeros(*shape, dtype=dtype))         # noqa: E731
    i32 = lambda n: dev(n, dtype=torch.int32)                                                    # noqa: E731
    ptrs, idxs, q, k, v = i32(3), i32(5), dev(2, 4, 16), dev(2, 64, 16), dev(2, 64, 8)
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="splits must be None or an integer from 1 to 64"):
            f(ptrs, idxs, 16, q, k, v, splits=bad)
    with pytest.raises(ValueError, match="no CPU path"):
        f(torch.zeros(3, dtype=torch.int32), idxs, 16, q, k, v)
    need = 4 * 2 * 4 * 2 * (8 + 3)
    bad = [(lambda: f(ptrs, idxs, 8, q, k, v), "page_size must be 16 or 32, not 8"),
           (lambda: f(ptrs, idxs, 16, dev(4, 16), k, v), r"q must be \[B, H, D\]"),
           (lambda: f(ptrs, idxs, 32, q, dev(2, 48, 16), dev(2, 48, 8)), "the 48 rows of k must be a multiple of the page size 32"),
           (lambda: f(ptrs, idxs, 16, q, dev(3, 64, 16), dev(3, 64, 8)), "the 4 heads of q must be a multiple of the 3 heads of k and v"),
           (lambda: f(ptrs, idxs, 16, dev(2, 34, 16), k, v), "at most 16 query heads to a K / V head, not 17"),
           (lambda: f(ptrs, idxs, 16, q, k, dev(4, 64, 8)), r"v must be \[64, width\] or \[2, 64, width\]"),
           (lambda: f(ptrs, idxs, 16, q, k, dev(2, 64, 12)), "takes Dv in multiples of 8 up to 128, not 12"),
           (lambda: f(i32(4), idxs, 16, q, k, v), "page_ptrs must be a contiguous torch.int32 tensor of 3 elements"),
           (lambda: f(ptrs, idxs, 16, q, k, v, seq_lens=i32(3)), "seq_lens must be a contiguous torch.int32 tensor of 2 elements"),
           (lambda: f(ptrs, idxs, 16, q, k, v, k_scale=dev(4, dtype=torch.float32)), "k_scale must be a contiguous torch.float32 tensor of 2 elements"),
           (lambda: f(ptrs, idxs, 16, q, k, v, out=dev(4, 2, 8, dtype=torch.float32)), r"out must be a torch.float32 tensor of shape \(2, 4, 8\)"),
           (lambda: f(ptrs, idxs, 16, q, k, v, splits=2, workspace=dev(need - 1)), f"at least {need} bytes")]
    for g, words in bad:
        with pytest.raises(ValueError, match=words):
            g()
    assert front.workspace_bytes(2, 4, 2, 8, 2) == need
    rule = front.default_splits
    # B * Hkv waves against 1024; 32-key steps of the mean sequence against 4 to a segment; clamped to 1 .. 64
    assert rule(1, 8, 2048, 32) == 64 and rule(8, 8, 8 * 256, 32) == 16 and rule(8, 8, 8 * 512, 16) == 16 and rule(64, 8, 64 * 2048, 32) == 2
    assert rule(2048, 8, 2048 * 256, 32) == 1 and rule(1, 1, 7, 32) == 1 and rule(1, 1, 40, 16) == 5 and rule(0, 0, 0, 16) == 1
