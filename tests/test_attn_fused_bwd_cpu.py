"""The fused block-sparse attention backward on a machine WITHOUT a GPU: the third library, its header and its binding, the entry
point's argument validation (which precedes any device work), the census of the library's kernel instances, and the two passes
as built, restated in numpy float32 (tests/_attn_fused_bwd_ref.py), against the derived tolerances the GPU tests use."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

pytest.importorskip("torch")

from mispmm import capi, capi_attn, capi_attn_bwd  # noqa: E402

import _attn_fused_bwd_ref as ref  # noqa: E402
import _attn_fused_ref as fwd_ref  # noqa: E402
from _softmax_bsr_ref import HELD, bf16_round  # noqa: E402
from test_census_cpu import _symbol_tool  # noqa: E402

INSTANCES = {"attn_bwd_rows_kernel": 16, "attn_bwd_cols_kernel": 16}       # __device_stub__ symbols per kernel template
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mispmm_attn_bsr_bwd_bf16"


def _declared(header):
    with open(os.path.join(ROOT, "include", header), encoding="utf-8") as f:
        raw = f.read()
    return raw, set(re.findall(r"\b(mispmm_attn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", raw, flags=re.S)))


def _symbols(path):
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    return subprocess.run([tool, "-C", path], capture_output=True, text=True, check=True).stdout


def test_the_third_library_exports_what_its_header_declares_and_the_binding_binds_it():
    assert os.path.exists(capi_attn_bwd.LIB_PATH), f"{capi_attn_bwd.LIB_PATH} is not built"
    _, declared = _declared("mispmm_attn_bwd.h")
    assert declared == set(capi_attn_bwd.SIGNATURES) == {ENTRY}
    handle = ctypes.CDLL(capi_attn_bwd.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in mispmm_attn_bwd.h but not exported"
    lib = capi_attn_bwd.lib()
    for name, (_, argtypes) in capi_attn_bwd.SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes and len(argtypes) == 43
    assert capi_attn_bwd.last_kernel() == lib.mispmm_last_kernel().decode()
    # the other two headers, bindings and libraries know nothing of the new entry point
    for header in ("mispmm.h", "mispmm_attn.h"):
        assert "attn_bsr_bwd" not in _declared(header)[0]
    assert not any("bwd" in n for n in capi_attn.SIGNATURES) and not any(n.startswith("mispmm_attn") for n in capi.SIGNATURES)
    for path in (capi.LIB_PATH, capi_attn.LIB_PATH):
        out = _symbols(path)
        assert "attn_bsr_bwd" not in out and "attn_bwd" not in out, path
    exported = set(re.findall(r"\bT (mispmm_[a-z0-9_]+)", _symbols(capi_attn_bwd.LIB_PATH)))
    assert exported == {ENTRY}


ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced


def _call(**kw):
    a = dict(stream=None, H=2, mb=4, K=64, bs=16, nb=3, ptrs=ONE, cols=ONE, tptrs=ONE, tcols=ONE, perm=ONE,
             q=ONE, ldq=64, qh=4096, k=ONE, ldk=64, kh=4096, v=ONE, ldv=64, vh=4096, g=ONE, ldg=64, gh=4096,
             out=ONE, ldo=64, oh=4096, out_bf16=0, lse=ONE, delta=ONE, D=64, Dv=64, mask=None, scale=0.125,
             dq=ONE, lddq=64, dqh=4096, dk=ONE, lddk=64, dkh=4096, dv=ONE, lddv=64, dvh=4096, grads_bf16=0)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_attn_bwd.lib().mispmm_attn_bsr_bwd_bf16(*a.values())


def test_every_kind_of_bad_argument_is_refused_with_its_message_before_any_device_work():
    err = capi_attn_bwd.last_error
    for name in ("ptrs", "cols", "q", "k", "v", "g", "lse"):
        assert _call(**{name: None}) == capi.ERR_INVALID_ARG, name
        assert "attn_bsr_bwd_bf16" in err() and "null" in err()
    for name in ("tptrs", "tcols"):
        for gone in (dict(dq=None), dict(dq=None, dk=None), dict(dq=None, dv=None)):
            assert _call(**{name: None}, **gone) == capi.ERR_INVALID_ARG, name
            assert "attn_bsr_bwd_bf16" in err() and "tBlockRowPtrs or tBlockColIdxs is null" in err()
    assert _call(perm=None, mask=ONE) == capi.ERR_INVALID_ARG and "attn_bsr_bwd_bf16: perm is null" in err()
    for name in ("out", "delta"):
        for gone in (dict(), dict(dk=None, dv=None), dict(dq=None, dv=None)):
            assert _call(**{name: None}, **gone) == capi.ERR_INVALID_ARG, name
            assert "attn_bsr_bwd_bf16: out or delta is null" in err()
    for bs in (0, 8, 17, 64):
        assert _call(bs=bs, K=64 * 17) == capi.ERR_UNSUPPORTED
        assert "attn_bsr_bwd_bf16" in err() and "16x16 or 32x32" in err() and f"bS={bs}" in err()
    for kw in (dict(D=12, ldq=16, ldk=16), dict(D=136, ldq=136, ldk=136), dict(Dv=0), dict(D=0), dict(Dv=132, ldv=136, ldo=136), dict(Dv=20)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "attn_bsr_bwd_bf16" in err() and "multiples of 8 from 8 to 128" in err()
    for scale in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert _call(scale=scale) == capi.ERR_INVALID_ARG
        assert "attn_bsr_bwd_bf16: scale must be finite and > 0" in err()
    for name in ("ldq", "ldk", "ldv", "ldg", "ldo", "lddq", "lddk", "lddv"):
        assert _call(**{name: 56}) == capi.ERR_INVALID_ARG, name
        assert "attn_bsr_bwd_bf16: leading dimension smaller than the width" in err()
    misaligned = [dict(q=ONE + 2), dict(k=ONE + 8), dict(v=ONE + 4), dict(g=ONE + 8), dict(out=ONE + 4), dict(lse=ONE + 4), dict(delta=ONE + 8),
                  dict(mask=ONE + 4), dict(dq=ONE + 8), dict(dk=ONE + 4), dict(dv=ONE + 2),
                  dict(ldq=68), dict(ldk=100), dict(ldv=100), dict(ldg=68), dict(qh=4100), dict(kh=4100), dict(vh=4100), dict(gh=4100),
                  dict(ldo=66), dict(ldo=68, out_bf16=1), dict(oh=4100, out_bf16=1), dict(oh=4098),
                  dict(lddq=66), dict(lddk=66), dict(lddv=66), dict(lddq=68, grads_bf16=1), dict(lddk=68, grads_bf16=1), dict(lddv=68, grads_bf16=1),
                  dict(dqh=4098), dict(dkh=4100, grads_bf16=1), dict(dvh=4098)]
    for kw in misaligned:
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "attn_bsr_bwd_bf16" in err() and "16-byte aligned" in err()
    assert _call(K=72) == capi.ERR_INVALID_ARG and "attn_bsr_bwd_bf16: K=72 is not a multiple of the block size 16" in err()
    assert _call(bs=32, K=48) == capi.ERR_INVALID_ARG and "not a multiple" in err()
    # 2 GiB: every operand alone.  2^23 rows (keys) of 64 bf16 span 1 GiB; a row stride of 136 takes it past 2 GiB
    names = ["Q", "K", "V", "dO", "out", "dQ", "dK", "dV"]
    for which, kw in (("Q", dict(mb=1 << 19, ldq=136)), ("dO", dict(mb=1 << 19, ldg=136)), ("out", dict(mb=1 << 19, ldo=136)),
                      ("dQ", dict(mb=1 << 19, lddq=136)), ("K", dict(K=1 << 23, ldk=136)), ("V", dict(K=1 << 23, ldv=136)),
                      ("dK", dict(K=1 << 23, lddk=136)), ("dV", dict(K=1 << 23, lddv=136))):
        assert _call(out_bf16=1, grads_bf16=1, **kw) == capi.ERR_UNSUPPORTED, which
        assert "attn_bsr_bwd_bf16" in err() and "2 GiB" in err()
        sizes = {n: int(re.search(rf"\b{n} (\d+)", err()).group(1)) for n in names}
        assert [n for n in names if sizes[n] > 0x7FFFFFFF] == [which], (which, sizes)


def test_no_ops_return_before_any_pointer_is_looked_at():
    gone = dict(ptrs=None, cols=None, tptrs=None, tcols=None, perm=None, q=None, k=None, v=None, g=None, out=None, lse=None, delta=None)
    assert _call(H=0, dq=None, dk=None, dv=None, **gone) == capi.OK
    assert _call(mb=0, **gone) == capi.OK
    assert _call(dq=None, dk=None, dv=None, **gone) == capi.OK                # all three outputs null
    assert _call(H=0, scale=float("nan")) == capi.ERR_INVALID_ARG              # ... but after the checks that need none
    assert _call(mb=0, D=12) == capi.ERR_UNSUPPORTED
    assert _call(dq=None, dk=None, dv=None, bs=8) == capi.ERR_UNSUPPORTED
    assert _call(dq=None, dk=None, dv=None, K=72) == capi.ERR_INVALID_ARG


def test_the_third_library_holds_the_recorded_instances_and_the_tag_table_lists_each():
    out = _symbols(capi_attn_bwd.LIB_PATH)
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found == INSTANCES, f"kernel template: instances in the library {found}, recorded here {INSTANCES}"
    tags = set()
    for which, args in set(re.findall(r"__device_stub__attn_bwd_(rows|cols)_kernel<([^>]*)>", out)):
        bs, ds, dsv, mask = (s.strip() for s in args.split(","))
        tags.add(f"attn_bsr_bwd_{which}<b{bs},{'mask' if mask == 'true' else 'nomask'},D{ds},V{dsv}>")
    assert tags == set(ref.TAGS), (sorted(tags - set(ref.TAGS)), sorted(set(ref.TAGS) - tags))
    assert len(ref.TAGS) == sum(INSTANCES.values())
    for tag, (bs, d, dv, mask) in ref.TAGS.items():
        assert tag in (ref.rows_tag(bs, d, dv, mask), ref.cols_tag(bs, d, dv, mask))
        assert ref.tag_of(bs, d, dv, mask) == ref.rows_tag(bs, d, dv, mask) + " + " + ref.cols_tag(bs, d, dv, mask)
        # the smallest shape: one step of 8 less in D or Dv is refused (a width of 0) or lands on another tag
        for dd, ddv in ((d - 8, dv), (d, dv - 8)):
            assert dd == 0 or ddv == 0 or tag not in (ref.rows_tag(bs, dd, ddv, mask), ref.cols_tag(bs, dd, ddv, mask))
    assert _call(D=0) == capi.ERR_UNSUPPORTED and _call(Dv=0) == capi.ERR_UNSUPPORTED
    assert ref.tag_of(16, 8, 8, False, (True, False, False)) == ref.rows_tag(16, 8, 8, False)
    assert ref.tag_of(16, 8, 8, False, (False, False, True)) == ref.cols_tag(16, 8, 8, False)


def test_the_transposed_edge_patterns_have_the_block_columns_the_column_pass_must_meet():
    for bs in (16, 32):
        c = HELD[bs]
        a, at, perm = ref.bwd_pattern(f"edgesT{bs}")
        per_column = np.diff(at.block_row_ptrs.astype(np.int64))
        assert sorted(set(per_column.tolist())) == sorted({0, 1, 2, 3, 4, 5, 8, 9, c - 1, c, c + 1, 2 * c + 1})
        assert per_column[0] == 0 and per_column[-1] == 0
        assert a.num_rows <= 1120 and a.num_cols <= 416
        assert sorted(perm.tolist()) == list(range(a.num_blocks))
        lead = ref.mask_of(f"edgesT{bs}", "leading")
        assert np.isneginf(lead).all(axis=(1, 2)).any() and not np.isneginf(lead).all()
    for name in ("ragged16", "ragged32", "edges16", "edges32"):                    # none of the four has an empty block column
        assert np.diff(ref.bwd_pattern(name)[1].block_row_ptrs.astype(np.int64)).min() >= 1


def test_the_forward_restated_here_is_the_forward_restatement():
    for name in fwd_ref.PATTERNS:
        q, k, v, _ = (x[0] for x in ref.operands(name, 40, 72))
        for kind in ("none", "causal"):
            mask = ref.mask_of(name, kind)
            mine, theirs = ref.forward_f32(name, q, k, v, mask, 0.2), fwd_ref.fused_f32(name, q, k, v, mask, 0.2)
            assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
        assert np.array_equal(ref.mask_of(name, "causal"), fwd_ref.mask_of(name, "causal"))
        assert np.array_equal(ref.mask_of(name, "leading"), fwd_ref.mask_of(name, "leading"))


@pytest.mark.parametrize("d,dv", [(8, 64), (40, 72)])
@pytest.mark.parametrize("kind", ref.MASKS)
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_the_backward_as_built_lies_inside_the_derived_tolerances(name, kind, d, dv):
    """numpy float32, pass by pass as the kernels go, on the restated forward's out (fp32 and rounded to bf16) and lse: dq, dk and
    dv, fp32 and rounded to bf16, inside bwd_tolerances against float64 dense masked attention."""
    from test_gpu_softmax_bsr import _dense_attention
    q, k, v, g = (x[0] for x in ref.operands(name, d, dv))
    mask, scale = ref.mask_of(name, kind), d ** -0.5
    want = _dense_attention(ref.bwd_pattern(name)[0], q, k, v, g, scale, mask)[1:]
    out, lse = ref.forward_f32(name, q, k, v, mask, scale)
    for out_bf16 in (False, True):
        stored_out = bf16_round(out) if out_bf16 else out
        for grads_bf16 in (False, True):
            got = ref.backward_f32(name, q, k, v, g, stored_out, lse, mask, scale, grads_bf16)
            tols = ref.bwd_tolerances(name, q, k, v, g, scale, mask, out_bf16, grads_bf16)
            for what, x, w, tol in zip(("dq", "dk", "dv"), got, want, tols):
                assert not np.isnan(x).any()
                err = np.abs(x.astype(np.float64) - w)
                print(f"restated backward {name} D={d} Dv={dv} {kind} out_bf16={out_bf16} grads_bf16={grads_bf16} {what}: "
                      f"max |err| / tolerance = {float(np.max(err / tol)):.3g}")
                assert np.all(err <= tol), f"{what}: the restatement breaks the bound"


@pytest.mark.parametrize("name", ["ragged32", "edgesT16"])
def test_the_restatement_on_a_rounded_float32_grad_out_lies_inside_the_tolerance_with_its_rounding_term(name):
    """grad_out with 24 significant bits, rounded to bf16 before the passes as the Python layer does; the float64 reference keeps
    it unrounded and bwd_tolerances(g_rounded=True) carries E_g = 2^-8 |grad_out|."""
    from test_gpu_softmax_bsr import _dense_attention
    d, dv = 40, 72
    q, k, v, _ = (x[0] for x in ref.operands(name, d, dv))
    bsr = ref.bwd_pattern(name)[0]
    rng = np.random.default_rng(91)
    g32 = (np.where(rng.random((bsr.num_rows, dv)) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, (bsr.num_rows, dv))).astype(np.float32)
    mask, scale = ref.mask_of(name, "causal"), d ** -0.5
    want = _dense_attention(bsr, q, k, v, g32, scale, mask)[1:]
    out, lse = ref.forward_f32(name, q, k, v, mask, scale)
    got = ref.backward_f32(name, q, k, v, bf16_round(g32), out, lse, mask, scale, True)
    tight = ref.bwd_tolerances(name, q, k, v, g32, scale, mask, False, True)
    for what, x, w, tol, t0 in zip(("dq", "dk", "dv"), got, want, ref.bwd_tolerances(name, q, k, v, g32, scale, mask, False, True, g_rounded=True), tight):
        err = np.abs(x.astype(np.float64) - w)
        print(f"restated backward, float32 grad_out {name} {what}: max |err| / tolerance = {float(np.max(err / tol)):.3g}")
        assert np.all(err <= tol) and np.all(tol >= t0) and np.any(tol > t0)


def test_masked_elements_and_empty_rows_and_columns_give_plus_zero_in_the_restatement():
    name, d, dv = "edgesT16", 8, 64
    a, at, _ = ref.bwd_pattern(name)
    q, k, v, g = (x[0] for x in ref.operands(name, d, dv))
    out, lse = ref.forward_f32(name, q, k, v, None, 0.3)
    dq, dk, dvv = ref.backward_f32(name, q, k, v, g, out, lse, None, 0.3, False)
    empty_cols = np.repeat(np.diff(at.block_row_ptrs.astype(np.int64)) == 0, 16)
    assert empty_cols.any() and not dk[empty_cols].view(np.uint32).any() and not dvv[empty_cols].view(np.uint32).any()
    assert dk[~empty_cols].any(axis=1).all() and dvv[~empty_cols].any(axis=1).all()
    empty_rows = np.repeat(np.diff(a.block_row_ptrs.astype(np.int64)) == 0, 16)
    assert not dq[empty_rows].view(np.uint32).any()


def test_python_layer_refuses_without_a_gpu_and_fused_backward_needs_fused():
    import torch
    from mispmm import autograd, ops
    from test_softmax_bsr_cpu import _OnDevice
    bsr, tbsr, perm = ref.bwd_pattern("ragged16")
    a, at = ops.DeviceBSR.from_host(bsr, device="cpu"), ops.DeviceBSR.from_host(tbsr, device="cpu")
    m, kk = bsr.num_rows, bsr.num_cols
    z = lambda *shape, dtype=torch.int16: torch.zeros(*shape, dtype=dtype)   # noqa: E731
    with pytest.raises(ValueError, match="no CPU path"):
        ops.attention_bsr_bwd_bf16(a, at, None, z(m, 8), z(kk, 8), z(kk, 8), z(m, 8, dtype=torch.float32), z(m, dtype=torch.float32), z(m, 8))
    t = autograd.TrainableBSR.from_host(bsr, device="cpu")
    bfz = lambda *shape: torch.zeros(*shape, dtype=torch.bfloat16)   # noqa: E731
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.block_sparse_attention(t, bfz(m, 8), bfz(kk, 8), bfz(kk, 8), fused=True, fused_backward=True)
    t.fwd.block_row_ptrs = _OnDevice(t.fwd.block_row_ptrs)
    dev = lambda *shape, dtype=torch.bfloat16: _OnDevice(torch.zeros(*shape, dtype=dtype))   # noqa: E731
    with pytest.raises(ValueError, match="needs fused=True"):
        autograd.block_sparse_attention(t, dev(m, 8), dev(kk, 8), dev(kk, 8), fused_backward=True)
    with pytest.raises(ValueError, match="needs fused=True"):
        autograd.block_sparse_attention(t, dev(m, 8), dev(kk, 8), dev(kk, 8), fused=False, fused_backward=True)
    # the ops call: shapes, types and strides are refused before the library is reached
    a.block_row_ptrs, at.block_row_ptrs = _OnDevice(a.block_row_ptrs), _OnDevice(at.block_row_ptrs)
    i16 = lambda *shape: dev(*shape, dtype=torch.int16)   # noqa: E731
    f32 = lambda *shape: dev(*shape, dtype=torch.float32)   # noqa: E731
    good = dict(q=i16(m, 8), k=i16(kk, 8), v=i16(kk, 16), out=f32(m, 16), lse=f32(m), grad_out=i16(m, 16))
    bad = [dict(q=i16(m, 12), k=i16(kk, 12)), dict(v=i16(kk, 136), out=f32(m, 136), grad_out=i16(m, 136)), dict(grad_out=i16(m, 8)),
           dict(grad_out=f32(m, 16)), dict(out=dev(m, 16)), dict(out=f32(m, 8)), dict(lse=f32(m + 1)), dict(lse=i16(m)), dict(k=i16(kk, 16)),
           dict(q=i16(2, m, 8)), dict(mask=f32(3, 16)), dict(dq=f32(m, 8)), dict(dv=i16(kk, 8)), dict(delta=f32(m, 1)), dict(need=(True, True)),
           dict(perm=dev(3, dtype=torch.int64)), dict(mask=f32(bsr.num_blocks, 16, 16))]
    for i, kw in enumerate(bad):
        args = {**good, **kw}
        extra = {n: args.pop(n) for n in ("mask", "dq", "dv", "delta", "need", "perm") if n in args}
        with pytest.raises(ValueError):
            ops.attention_bsr_bwd_bf16(a, at, extra.pop("perm", None), args["q"], args["k"], args["v"], args["out"], args["lse"], args["grad_out"], **extra)
            pytest.fail(f"case {i} was not refused")
    with pytest.raises(ValueError, match="pattern of A\\^T"):
        ops.attention_bsr_bwd_bf16(a, a, None, *good.values())


@pytest.mark.parametrize("name,kind", [("ragged16", "causal"), ("edges32", "leading"), ("ragged32", "none")])
def test_the_blockwise_chain_tolerance_is_the_composed_one(name, kind):
    from test_gpu_softmax_bsr import _attention_tolerances
    q, k, v, g = (x[0] for x in ref.operands(name, 40, 72))
    mask, scale = ref.mask_of(name, kind), 40 ** -0.5
    want = _attention_tolerances(name, q, k, v, g, scale, mask, True)[1:]
    for what, x, w in zip(("dq", "dk", "dv"), ref.chain_grad_tolerances(name, q, k, v, g, scale, mask), want):
        assert np.allclose(x, w, rtol=1e-10, atol=0), what
