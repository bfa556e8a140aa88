"""The split-row fp8 e4m3 fused attention forward with shared KV heads (libmispmm_attn_fp8_split.so,
include/mispmm_attn_fp8_split.h) on a machine WITHOUT a GPU: the sixteenth library and its two exports, the workspace formula,
every new refusal of the entry point with its text and its place among the inherited ones (all precede any device work), the
Python front's ValueErrors and the default rule."""
import ctypes
import os
import re
import subprocess
import types

import pytest

from mispmm import capi, capi_attn_fp8, capi_attn_fp8_split

from test_census_cpu import _symbol_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INV, UNS = capi.OK, capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced
NEED = 4 * 4 * 4 * 16 * 4 * (16 + 3)       # workspace bytes of _call()'s defaults: H = 4, 4 block rows of 16, 4 splits, Dv = 16
NAMES = {"mispmm_attn_bsr_fp8_split", "mispmm_attn_bsr_fp8_split_workspace"}


def test_the_library_exports_exactly_what_its_header_declares():
    assert os.path.exists(capi_attn_fp8_split.LIB_PATH), f"{capi_attn_fp8_split.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn_fp8_split.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert set(re.findall(r"\b(mispmm_[a-z0-9_]+)\s*\(", text)) == set(capi_attn_fp8_split.SIGNATURES) == NAMES
    lib = capi_attn_fp8_split.lib()                  # raises where an export is missing
    tool = _symbol_tool()
    if tool is not None:
        out = subprocess.run([tool, "-D", "--defined-only", capi_attn_fp8_split.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("mispmm_")} == NAMES
    assert capi_attn_fp8_split.last_kernel() == lib.mispmm_last_kernel().decode()
    for other in (capi.LIB_PATH, capi_attn_fp8.LIB_PATH):
        assert not any(hasattr(ctypes.CDLL(other), name) for name in NAMES), other


@pytest.mark.parametrize("h, mb, bs, dv, s", [(2, 4, 16, 64, 4), (1, 1, 32, 8, 1), (8, 2, 32, 128, 64), (3, 5, 16, 72, 3), (0, 7, 16, 8, 2),
                                              (1 << 13, 1 << 20, 32, 128, 64)])
def test_the_workspace_is_four_bytes_per_row_split_and_column_plus_three(h, mb, bs, dv, s):
    assert capi_attn_fp8_split.lib().mispmm_attn_bsr_fp8_split_workspace(h, mb, bs, dv, s) == 4 * h * mb * bs * s * (dv + 3)


def _call(**kw):
    a = dict(stream=None, H=4, Mb=4, K=64, bS=16, numBlocks=3, ptrs=ONE, idxs=ONE, Q=ONE, ldq=32, q_head=2048, Kmat=ONE, ldk=32, k_head=2048,
             V=ONE, ldv=16, v_head=1024, D=32, Dv=16, mask=None, scale=0.25, qs=None, ks=None, vs=None, out=ONE, ldo=16, o_head=1024, bf16=0,
             lse=None, kv_group=2, splits=4, ws=ONE, ws_bytes=NEED)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_attn_fp8_split.lib().mispmm_attn_bsr_fp8_split(*a.values())


REFUSALS = [(dict(kv_group=0), INV, "kv_group must be 1 or more and divide H (got kv_group=0, H=4)"),
            (dict(kv_group=3), INV, "kv_group must be 1 or more and divide H (got kv_group=3, H=4)"),
            (dict(kv_group=8), INV, "kv_group must be 1 or more and divide H (got kv_group=8, H=4)"),
            (dict(splits=0), INV, "splits must be 1 to 64 (got 0)"), (dict(splits=65), INV, "splits must be 1 to 64 (got 65)"),
            (dict(ws=None), INV, f"hold {NEED} bytes (got null"), (dict(ws=ONE + 8), INV, f"hold {NEED} bytes (got a misaligned pointer"),
            (dict(ws_bytes=NEED - 1), INV, f"hold {NEED} bytes (got an aligned pointer, {NEED - 1} bytes)"),
            (dict(splits=8), INV, f"hold {2 * NEED} bytes"),
            (dict(Mb=1 << 21, H=1 << 10, D=16, ldq=16, ldk=16, kv_group=1, splits=64, ws_bytes=1 << 62), UNS,
             "33554432 rows x 1024 heads x 64 splits are more work units than one launch takes")]


@pytest.mark.parametrize("kw, status, text", REFUSALS, ids=[str(r[0]) for r in REFUSALS])
def test_a_new_refusal_carries_its_text_before_any_device_work(kw, status, text):
    assert _call(**kw) == status
    err = capi_attn_fp8_split.last_error()
    assert err.startswith("attn_bsr_fp8_split: ") and text in err, err


def test_the_refusals_stand_in_the_order_of_the_header():
    err = capi_attn_fp8_split.last_error
    # the inherited shape checks first, in the order of mispmm_attn_bsr_fp8 ...
    assert _call(bS=8, scale=0.0) == UNS and "only 16x16 or 32x32 blocks (got bS=8)" in err()
    assert _call(scale=0.0, D=12) == INV and "scale must be finite and > 0" in err()
    assert _call(D=12, K=72) == UNS and "multiples of 8 from 8 to 128" in err()
    assert _call(K=72, D=24) == INV and "K=72 is not a multiple of the block size 16" in err()
    assert _call(D=24, ldq=128, ldk=128, kv_group=0) == UNS and "D must be a multiple of 16 from 16 to 128 (got D=24)" in err()
    # ... then kv_group, splits, the workspace, and only then the no-op ...
    assert _call(kv_group=3, splits=0) == INV and "kv_group" in err()
    assert _call(splits=0, ws=None) == INV and "splits" in err()
    assert _call(ws=None, H=0) == INV and "hold 0 bytes (got null" in err()
    assert _call(H=0, kv_group=0) == INV and "kv_group" in err()
    nothing = dict(ptrs=None, idxs=None, Q=None, Kmat=None, V=None, out=None, ws_bytes=0)
    assert _call(H=0, **nothing) == OK and _call(Mb=0, **nothing) == OK
    # ... then what mispmm_attn_bsr_fp8 refuses after its no-op, in its order
    assert _call(ws_bytes=NEED - 1, Q=None) == INV and "workspace" in err()
    for name in ("ptrs", "idxs", "Q", "Kmat", "V", "out"):
        assert _call(**{name: None}) == INV and "blockRowPtrs, blockColIdxs, Q, K, V or out is null" in err(), name
    assert _call(Q=None, ldq=16) == INV and "null" in err()
    assert _call(ldq=16, Kmat=ONE + 8) == INV and "leading dimension smaller than the width" in err()
    assert _call(Kmat=ONE + 8, qs=ONE + 2) == UNS and "must be 16-byte aligned and V 8-byte" in err()
    assert _call(qs=ONE + 2, K=1 << 26) == UNS and "q_scale, k_scale and v_scale must be 4-byte aligned" in err()
    assert _call(K=1 << 26, Mb=1 << 20, H=1 << 13, ws_bytes=1 << 62) == UNS and "spans 2 GiB or more" in err()


def test_the_python_front_refuses_with_value_errors_and_the_default_rule_keeps_full_cards_unsplit():
    torch = pytest.importorskip("torch")
    from mispmm import attn_bsr_fp8_split, ops
    from test_softmax_bsr_cpu import _OnDevice
    f = attn_bsr_fp8_split.attention_bsr_fp8_split
    dev = lambda *shape, dtype=torch.uint8: _OnDevice(torch.zeros(*shape, dtype=dtype))         # noqa: E731
    ints = torch.zeros(3, dtype=torch.int32)
    a = ops.DeviceBSR(32, 64, 16, 16, 2, _OnDevice(ints), _OnDevice(ints), None)
    q, k, v = dev(4, 32, 16), dev(2, 64, 16), dev(2, 64, 8)
    for bad in (0, 65, -1, 2.0, True, "many"):
        with pytest.raises(ValueError, match="splits must be None or an integer from 1 to 64"):
            f(a, q, k, v, splits=bad)
    with pytest.raises(ValueError, match="no CPU path"):
        f(ops.DeviceBSR(32, 64, 16, 16, 2, ints, ints, None), *(torch.zeros((n, 16), dtype=torch.uint8) for n in (32, 64, 64)), splits=2)
    need = 4 * 4 * 32 * 2 * (8 + 3)
    bad = [(lambda: f(a, q, dev(3, 64, 16), dev(3, 64, 8), splits=2), "the 4 heads of q must be a multiple of the 3 heads of k and v"),
           (lambda: f(a, q, k, dev(4, 64, 8), splits=2), r"v must be \[64, width\] or \[2, 64, width\]"),
           (lambda: f(a, dev(32, 16), k, v, splits=2), "q, k and v must all be 2-D or all"),
           (lambda: f(a, q, k, v, k_scale=dev(4, dtype=torch.float32), splits=2), "k_scale must be a contiguous torch.float32 tensor of 2 elements"),
           (lambda: f(a, q, k, v, splits=2, workspace=dev(need, dtype=torch.int8)), f"workspace must be a contiguous 1-D uint8 tensor of at least {need}"),
           (lambda: f(a, q, k, v, splits=2, workspace=dev(2, need)), "workspace must be a contiguous 1-D uint8 tensor"),
           (lambda: f(a, q, k, v, splits=2, workspace=dev(need - 1)), f"at least {need} bytes")]
    for g, words in bad:
        with pytest.raises(ValueError, match=words):
            g()
    rule = attn_bsr_fp8_split.default_splits
    from _softmax_bsr_ref import pattern
    assert rule(pattern("ACTIVSg10K"), 8) == 1
    two_rows = types.SimpleNamespace(num_rows=32, block_row_size=16, num_blocks=2 * 512)
    assert rule(two_rows, 1) == 64 and rule(two_rows, 256) == 2
