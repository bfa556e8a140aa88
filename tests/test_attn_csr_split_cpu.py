"""The split-row fused attention forward on a CSR pattern (include/mispmm_attn_csr_split.h) WITHOUT a GPU: the library and its
binding, the workspace formula, every refusal of both entry points (all precede any device work), the no-op returns, the Python
fronts' checks, the default rule, and the segment bounds of the header restated in numpy."""
import os
import re
import types

import numpy as np
import pytest

from mispmm import capi, capi_attn_csr_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced
NEED = 4 * 2 * 100 * 4 * (64 + 2)          # workspace bytes of _call()'s defaults: H = 2, M = 100, 4 splits, Dv = 64
INVALID, UNSUPPORTED = capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
EXPORTS = {"f32": "mispmm_attn_csr_split_f32", "bf16": "mispmm_attn_csr_split_bf16"}


def test_the_library_exports_what_its_header_declares_and_the_workspace_formula():
    with open(os.path.join(ROOT, "include", "mispmm_attn_csr_split.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_attn_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_attn_csr_split.SIGNATURES) == {*EXPORTS.values(), "mispmm_attn_csr_split_workspace", "mispmm_attn_csr_split_last_partial"}
    need = capi_attn_csr_split.lib().mispmm_attn_csr_split_workspace        # lib() raises where an export is missing
    assert need(2, 100, 64, 4) == NEED and need(0, 5, 8, 2) == 0
    assert need(1, 1, 1, 1) == 4 * (4 + 2) and need(3, 5, 5, 2) == 4 * 30 * (8 + 2) and need(1, 7, 253, 256) == 4 * 7 * 256 * (256 + 2)
    assert need(8, 1 << 20, 256, 256) == 4 * 8 * (1 << 20) * 256 * 258 > 1 << 32


def _call(kind="f32", **kw):
    a = dict(stream=None, H=2, M=100, K=64, nnz=500, ptrs=ONE, cols=ONE, q=ONE, qh=6400, ldq=64, k=ONE, kh=4096, ldk=64, D=64, v=ONE, vh=4096, ldv=64,
             Dv=64, scale=0.125, bias=None, bh=0, out=ONE, oh=6400, ldo=64, **({"out_bf16": 0} if kind == "bf16" else {}),
             lse=None, splits=4, min_batches=4, ws=ONE, ws_bytes=NEED)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return getattr(capi_attn_csr_split.lib(), EXPORTS[kind])(*a.values())


TINY = dict(ldq=1, ldo=1, D=1, Dv=1, ldk=1, ldv=1)
REFUSALS = [(dict(D=257, ldq=257, ldk=257), UNSUPPORTED, "D and Dv must be from 1 to 256"), (dict(Dv=0), UNSUPPORTED, "D and Dv must be from 1 to 256"),
            (dict(scale=float("inf")), INVALID, "scale must be finite"), (dict(min_batches=0), INVALID, "min_batches must be at least 1"),
            (dict(splits=0), INVALID, "splits must be 1 to 256 (got 0)"), (dict(splits=257), INVALID, "splits must be 1 to 256 (got 257)"),
            (dict(ptrs=None), INVALID, "is null"), (dict(q=None), INVALID, "is null"), (dict(out=None), INVALID, "is null"), (dict(cols=None), INVALID, "is null"),
            (dict(ldv=56), INVALID, "leading dimension smaller"), (dict(K=1 << 28), UNSUPPORTED, "2 GiB"),
            (dict(M=1 << 25, splits=128, **TINY), UNSUPPORTED, "2^32 work items"),
            (dict(M=1 << 24, H=1 << 12, splits=128, **TINY), UNSUPPORTED, "more workgroups than one launch takes"),
            (dict(ws=None), INVALID, f"hold {NEED} bytes (got null"), (dict(ws=ONE + 8), INVALID, "a misaligned pointer"),
            (dict(ws_bytes=NEED - 1), INVALID, f"hold {NEED} bytes (got an aligned pointer, {NEED - 1} bytes)"), (dict(splits=8), INVALID, f"hold {2 * NEED} bytes")]


@pytest.mark.parametrize("kind", EXPORTS)
@pytest.mark.parametrize("kw,status,text", REFUSALS, ids=[str(r[0]) for r in REFUSALS])
def test_a_bad_argument_is_refused_with_its_message_before_any_device_work(kw, status, text, kind):
    before = capi.last_kernel()
    assert _call(kind, **kw) == status
    err = capi_attn_csr_split.last_error()
    assert err.startswith(f"attn_csr_split_{kind}: ") and text in err, err
    assert capi.last_kernel() == before


def test_bf16_bases_must_be_2_byte_aligned_and_no_ops_return_before_any_pointer_is_looked_at():
    for odd in (dict(q=ONE + 1), dict(out=ONE + 1, out_bf16=1)):
        assert _call("bf16", **odd) == INVALID and "2-byte aligned" in capi_attn_csr_split.last_error()
    nothing = dict(ptrs=None, cols=None, q=None, k=None, v=None, out=None, ws=None, ws_bytes=0)
    for kind in EXPORTS:
        assert _call(kind, H=0, **nothing) == capi.OK and _call(kind, M=0, **nothing) == capi.OK
        assert _call(kind, H=0, splits=0) == INVALID and _call(kind, M=0, D=300) == UNSUPPORTED       # ... but after the checks that need none


def test_the_python_fronts_refuse_bad_keywords_and_the_default_rule_keeps_short_rows_on_one_launch():
    torch = pytest.importorskip("torch")
    from mispmm import attn_csr_split, autograd, ops
    import _attn_csr_ref as ref
    from _softmax_ref import matrix
    csr = matrix("long")
    a, t = ops.DeviceCSR.from_host(csr, plan=False, device="cpu"), autograd.TrainableCSR.from_host(csr, device="cpu")
    q, kv = torch.zeros((csr.num_rows, 8)), torch.zeros((csr.num_cols, 8))
    for front, cast in ((attn_csr_split.attention_csr_split, torch.float32), (attn_csr_split.attention_csr_split_bf16, torch.int16)):
        for bad in (0, 257, -1, 2.0, True, "many"):
            with pytest.raises(ValueError, match="splits must be None or an integer from 1 to 256"):
                front(a, q.to(cast), kv.to(cast), kv.to(cast), splits=bad)
    split = attn_csr_split.attention_csr_split
    bad_ws = (torch.zeros(64), torch.zeros((8, 8), dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)[::2])
    for kw, text in [(dict(splits=2, min_batches=0), "min_batches must be a positive integer"), (dict(splits=2), "no CPU path"), (dict(), "no CPU path"),
                     *((dict(splits=2, workspace=ws), "workspace must be a contiguous 1-D uint8 tensor") for ws in bad_ws)]:
        with pytest.raises(ValueError, match=text):
            split(a, q, kv, kv, **kw)
    for kw in (dict(splits=2), dict()):                                   # the operand checks are the one-launch front's, on both paths
        with pytest.raises(ValueError, match="q must be a float32 tensor"):
            split(a, q.double(), kv, kv, **kw)
    with pytest.raises(ValueError, match="needs fused=True"):
        autograd.sparse_attention(t, q, kv, kv, splits=2)
    with pytest.raises(ValueError, match="splits must be None or an integer"):
        autograd.sparse_attention(t, q, kv, kv, fused=True, splits=0)
    with pytest.raises(ValueError, match="splits must be None or an integer"):
        autograd.sparse_attention_bf16(t, q.bfloat16(), kv.bfloat16(), kv.bfloat16(), splits="many")
    rule = attn_csr_split.default_splits
    pat = lambda m, nnz: types.SimpleNamespace(num_rows=m, nnz=nnz)                       # noqa: E731
    assert rule(csr, 1, 8) == 1 and rule(pat(8192, 8192 * 14), 8, 64) == 1              # short rows: the one-launch kernel
    assert rule(pat(64, 64 * 8192), 1, 128) == 32                                       # decoding: min(2048 // 64, 1024 // 4)
    assert rule(pat(64, 64 * 8192), 8, 128) == 4 and rule(pat(64, 64 * 8192), 8, 64, wide=8) == 16
    assert rule(pat(64, 64 * 256), 1, 64) == 8 and rule(pat(1 << 16, (1 << 16) * 4096), 1, 64) == 1
    for w in (4, 32, 36, 68, 128, 132, 256):                                             # the rule's G is the library's, as the tags restate it
        assert f"G{attn_csr_split._group(w, 4)},V4" in ref.tag_of(4, w, True) and f"G{attn_csr_split._group(2 * w, 8)},V4" in ref.tag_of(4, w, True)


def test_the_segments_of_the_header_tile_every_row():
    """S' = min(splits, max(1, n // min_batches)); segment s starts at s (n // S') + s (n mod S') // S': for all n <= 300, splits
    <= 9, min_batches <= 5 the segments tile 0 .. n - 1, none is empty, each holds min_batches batches unless S' = 1."""
    for n, splits, mb in np.ndindex(301, 9, 5):
        s_ = min(splits + 1, max(1, n // (mb + 1)))
        s = np.arange(s_ + 1)
        start = s * (n // s_) + s * (n % s_) // s_
        assert np.array_equal(start, s * n // s_) and start[0] == 0 and start[-1] == n
        assert (n == 0 or np.diff(start).min() >= 1) and (s_ == 1 or np.diff(start).min() >= mb + 1), (n, splits, mb)
