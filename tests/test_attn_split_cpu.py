"""The split-row fused attention forward (include/mispmm_attn_split.h) WITHOUT a GPU: the library, its binding and its kernel census,
every refusal of the entry point (all precede any device work), the no-op returns, the Python front's checks and default rule."""
import os
import re
import subprocess
import types

import pytest

from mispmm import capi, capi_attn_split

from test_census_cpu import _symbol_tool

INSTANCES = {"attn_bsr_split_kernel": 16, "attn_bsr_combine_kernel": 2}   # 2 block sizes x D2/D4 x T4/T8 x mask; out type
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced
NEED = 4 * 2 * 4 * 16 * 4 * (64 + 3)       # workspace bytes of _call()'s defaults: H = 2, 4 block rows of 16, 4 splits, Dv = 64


def test_the_library_exports_what_its_header_declares_and_holds_the_recorded_instances():
    assert os.path.exists(capi_attn_split.LIB_PATH), f"{capi_attn_split.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn_split.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_attn_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_attn_split.SIGNATURES) == {"mispmm_attn_bsr_split_bf16", "mispmm_attn_bsr_split_workspace"}
    lib = capi_attn_split.lib()                      # raises where an export is missing
    for name, (_, argtypes) in capi_attn_split.SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes
    assert lib.mispmm_attn_bsr_split_workspace(2, 4, 16, 64, 4) == NEED
    assert capi_attn_split.last_kernel() == lib.mispmm_last_kernel().decode()
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    out = subprocess.run([tool, "-C", capi_attn_split.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found == INSTANCES, f"kernel template: instances in the library {found}, recorded here {INSTANCES}"


def _call(**kw):
    a = dict(stream=None, H=2, mb=4, K=64, bs=16, nb=3, ptrs=ONE, cols=ONE, q=ONE, ldq=64, qh=4096, k=ONE, ldk=64, kh=4096, v=ONE, ldv=64, vh=4096,
             D=64, Dv=64, mask=None, scale=0.125, out=ONE, ldo=64, oh=4096, out_bf16=0, lse=None, splits=4, ws=ONE, ws_bytes=NEED)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_attn_split.lib().mispmm_attn_bsr_split_bf16(*a.values())


INVALID, UNSUPPORTED = capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
REFUSALS = [(dict(ptrs=None), INVALID, "null"), (dict(q=None), INVALID, "null"), (dict(out=None), INVALID, "null"),
            (dict(bs=8), UNSUPPORTED, "16x16 or 32x32"), (dict(D=12, ldq=16, ldk=16), UNSUPPORTED, "multiples of 8 from 8 to 128"),
            (dict(Dv=136, ldv=136, ldo=136), UNSUPPORTED, "multiples of 8 from 8 to 128"), (dict(scale=float("nan")), INVALID, "scale must be finite"),
            (dict(K=72), INVALID, "K=72 is not a multiple"), (dict(ldv=56), INVALID, "leading dimension smaller"),
            (dict(q=ONE + 2), UNSUPPORTED, "16-byte aligned"), (dict(ldo=66), UNSUPPORTED, "16-byte aligned"),
            (dict(oh=4100, out_bf16=1), UNSUPPORTED, "16-byte aligned"), (dict(K=1 << 24, ldk=64), UNSUPPORTED, "2 GiB"),
            (dict(mb=1 << 22, H=1 << 10, ldq=8, D=8, ldk=8, splits=64), UNSUPPORTED, "x 64 splits are more work units"),
            (dict(splits=0), INVALID, "splits must be 1 to 64 (got 0)"), (dict(splits=65), INVALID, "splits must be 1 to 64 (got 65)"),
            (dict(ws=None), INVALID, f"hold {NEED} bytes (got null"), (dict(ws=ONE + 8), INVALID, "a misaligned pointer"),
            (dict(ws_bytes=NEED - 1), INVALID, f"hold {NEED} bytes (got an aligned pointer, {NEED - 1} bytes)"),
            (dict(splits=8), INVALID, f"hold {2 * NEED} bytes")]


@pytest.mark.parametrize("kw,status,text", REFUSALS, ids=[str(r[0]) for r in REFUSALS])
def test_a_bad_argument_is_refused_with_its_message_before_any_device_work(kw, status, text):
    assert _call(**kw) == status
    err = capi_attn_split.last_error()
    assert err.startswith("attn_bsr_split_bf16: ") and text in err, err


def test_no_ops_return_before_any_pointer_is_looked_at():
    nothing = dict(ptrs=None, cols=None, q=None, k=None, v=None, out=None, ws=None, ws_bytes=0)
    assert _call(H=0, **nothing) == capi.OK and _call(mb=0, **nothing) == capi.OK
    assert _call(H=0, splits=0) == INVALID and _call(mb=0, D=12) == UNSUPPORTED        # ... but after the checks that need none


def test_the_python_front_refuses_bad_splits_and_the_default_rule_keeps_full_cards_on_one_wave():
    torch = pytest.importorskip("torch")
    from mispmm import attn_bsr_split, autograd, ops
    from _softmax_bsr_ref import pattern
    bsr = pattern("ragged16")
    a, t = ops.DeviceBSR.from_host(bsr, device="cpu"), autograd.TrainableBSR.from_host(bsr, device="cpu")
    q = torch.zeros((bsr.num_rows, 8), dtype=torch.int16)
    for bad in (0, 65, -1, 2.0, True, "many"):
        with pytest.raises(ValueError, match="splits must be None or an integer from 1 to 64"):
            attn_bsr_split.attention_bsr_split_bf16(a, q, q, q, splits=bad)
    with pytest.raises(ValueError, match="no CPU path"):
        attn_bsr_split.attention_bsr_split_bf16(a, q, q, q, splits=2)
    qb = q.view(torch.bfloat16)
    with pytest.raises(ValueError, match="needs fused=True"):
        autograd.block_sparse_attention(t, qb, qb, qb, splits=2)
    assert attn_bsr_split.default_splits(pattern("ACTIVSg10K"), 8) == 1
    two_rows = types.SimpleNamespace(num_rows=32, block_row_size=16, num_blocks=2 * 512)
    assert attn_bsr_split.default_splits(two_rows, 1) == 64 and attn_bsr_split.default_splits(two_rows, 256) == 2
