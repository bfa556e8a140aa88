"""The fused block-sparse attention forward on a machine WITHOUT a GPU: the second library and its binding, the entry point's
argument validation (which precedes any device work), the census of the new library's kernel instances, and the algorithm as
built, restated in numpy float32 (tests/_attn_fused_ref.py), against the tolerances the GPU tests use."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_attn

import _attn_fused_ref as ref
from _softmax_bsr_ref import bf16_round, pattern
from test_census_cpu import _symbol_tool

INSTANCES = {"attn_bsr_kernel": 32}       # __device_stub__ symbols of libmispmm_attn.so per kernel template
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_second_library_exports_what_its_header_declares_and_the_binding_binds_it():
    assert os.path.exists(capi_attn.LIB_PATH), f"{capi_attn.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_attn_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_attn.SIGNATURES) == {"mispmm_attn_bsr_bf16"}
    handle = ctypes.CDLL(capi_attn.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in mispmm_attn.h but not exported"
    lib = capi_attn.lib()
    for name, (_, argtypes) in capi_attn.SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes
    # the tag and the error text are read through the handle of the library loaded here
    assert capi_attn.last_kernel() == lib.mispmm_last_kernel().decode()
    with open(os.path.join(ROOT, "include", "mispmm.h"), encoding="utf-8") as f:
        assert "mispmm_attn" not in f.read()
    assert not any(n.startswith("mispmm_attn") for n in capi.SIGNATURES)


ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced


def _call(**kw):
    a = dict(stream=None, H=2, mb=4, K=64, bs=16, nb=3, ptrs=ONE, cols=ONE, q=ONE, ldq=64, qh=4096, k=ONE, ldk=64, kh=4096, v=ONE, ldv=64, vh=4096,
             D=64, Dv=64, mask=None, scale=0.125, out=ONE, ldo=64, oh=4096, out_bf16=0, lse=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_attn.lib().mispmm_attn_bsr_bf16(*a.values())


def test_every_kind_of_bad_argument_is_refused_with_its_message_before_any_device_work():
    err = capi_attn.last_error
    for name in ("ptrs", "cols", "q", "k", "v", "out"):
        assert _call(**{name: None}) == capi.ERR_INVALID_ARG, name
        assert "attn_bsr_bf16" in err() and "null" in err()
    for bs in (0, 8, 17, 64):
        assert _call(bs=bs, K=64 * 17) == capi.ERR_UNSUPPORTED
        assert "16x16 or 32x32" in err() and f"bS={bs}" in err()
    for kw in (dict(D=12, ldq=16, ldk=16), dict(D=136, ldq=136, ldk=136), dict(Dv=0), dict(D=0), dict(Dv=132, ldv=136, ldo=136), dict(Dv=20)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "multiples of 8 from 8 to 128" in err()
    for scale in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert _call(scale=scale) == capi.ERR_INVALID_ARG
        assert "scale must be finite and > 0" in err()
    for kw in (dict(ldq=56), dict(ldk=56), dict(ldv=56), dict(ldo=56)):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert "leading dimension smaller than the width" in err()
    for kw in (dict(q=ONE + 2), dict(k=ONE + 8), dict(v=ONE + 4), dict(out=ONE + 4), dict(mask=ONE + 4), dict(ldq=68), dict(ldv=100), dict(kh=4100),
               dict(ldo=66), dict(ldo=68, out_bf16=1), dict(oh=4100, out_bf16=1)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "16-byte aligned" in err()
    assert _call(K=72) == capi.ERR_INVALID_ARG and "K=72 is not a multiple of the block size 16" in err()
    assert _call(bs=32, K=48) == capi.ERR_INVALID_ARG and "not a multiple" in err()
    # a head of K or V that spans 2 GiB or more
    assert _call(K=1 << 24, ldk=64) == capi.ERR_UNSUPPORTED and "2 GiB" in err()
    assert _call(K=1 << 24, ldk=8, D=8, ldq=8, ldv=64) == capi.ERR_UNSUPPORTED and "2 GiB" in err()       # V alone
    assert _call(mb=1 << 20, ldq=1024) == capi.ERR_UNSUPPORTED and "2 GiB" in err()


def test_no_ops_return_before_any_pointer_is_looked_at():
    assert _call(H=0, ptrs=None, cols=None, q=None, k=None, v=None, out=None) == capi.OK
    assert _call(mb=0, ptrs=None, cols=None, q=None, k=None, v=None, out=None) == capi.OK
    assert _call(H=0, scale=float("nan")) == capi.ERR_INVALID_ARG          # ... but after the checks that need none
    assert _call(mb=0, D=12) == capi.ERR_UNSUPPORTED
    assert _call(H=0, bs=8) == capi.ERR_UNSUPPORTED


def _symbols():
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    return subprocess.run([tool, "-C", capi_attn.LIB_PATH], capture_output=True, text=True, check=True).stdout


def test_the_new_library_holds_the_recorded_instances_and_the_tag_table_lists_each():
    out = _symbols()
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found == INSTANCES, f"kernel template: instances in the library {found}, recorded here {INSTANCES}"
    tags = set()
    for args in set(re.findall(r"__device_stub__attn_bsr_kernel<([^>]*)>", out)):
        bs, ds, tpl, mask, out_bf16 = (s.strip() for s in args.split(","))
        tags.add(f"attn_bsr<b{bs},{'bf16' if out_bf16 == 'true' else 'f32'},{'mask' if mask == 'true' else 'nomask'},D{ds},T{tpl}>")
    assert tags == set(ref.TAGS), (sorted(tags - set(ref.TAGS)), sorted(set(ref.TAGS) - tags))
    assert len(ref.TAGS) == INSTANCES["attn_bsr_kernel"]
    for tag, (bs, d, dv, mask, out_bf16) in ref.TAGS.items():
        assert ref.tag_of(bs, d, dv, mask, out_bf16) == tag
        # the smallest shape: one step of 8 less in D or Dv is refused or lands on another tag
        for dd, ddv in ((d - 8, dv), (d, dv - 8)):
            assert dd == 0 or ddv == 0 or ref.tag_of(bs, dd, ddv, mask, out_bf16) != tag
    # csrc/ and the first library are untouched by the new kernel: no attn symbol there
    first = subprocess.run([_symbol_tool(), "-C", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "attn_bsr" not in first


def test_the_leading_mask_blanks_whole_steps():
    for name in ref.PATTERNS:
        p = pattern(name)
        m = ref.leading_mask(name)
        ptrs = p.block_row_ptrs.astype(np.int64)
        whole = 0
        for lo, hi in zip(ptrs[:-1], ptrs[1:]):
            n = hi - lo
            blank = np.isneginf(m[lo:hi]).all(axis=(1, 2))
            assert blank.sum() == ((n + 1) // 2 if n >= 2 else 0) and not blank[-1:].any() and not np.isneginf(m[lo:hi][~blank]).any()
            whole += int(blank.sum() * p.block_row_size >= 32)
        assert whole >= 3


@pytest.mark.parametrize("kind", ref.MASKS)
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_the_algorithm_as_built_lies_inside_the_tolerances(name, kind):
    """numpy float32, step by step as the kernel goes: out inside the composed tolerance of the three-launch chain (fp32 and
    rounded to bf16), lse inside the bound of tests/_attn_fused_ref.py."""
    pytest.importorskip("torch")
    from test_gpu_softmax_bsr import _attention_tolerances, _dense_attention
    d, dv = 40, 72
    q, k, v = (x[0] for x in ref.operands(name, d, dv))
    mask, scale = ref.mask_of(name, kind), d ** -0.5
    g = np.zeros((q.shape[0], dv), np.float32)
    want = _dense_attention(pattern(name), q, k, v, g, scale, mask)[0]
    out, lse = ref.fused_f32(name, q, k, v, mask, scale)
    assert not np.isnan(out).any()
    for out_bf16 in (False, True):
        tol = _attention_tolerances(name, q, k, v, g, scale, mask, out_bf16)[0]
        err = np.abs((bf16_round(out) if out_bf16 else out).astype(np.float64) - want)
        print(f"restated {name} {kind} bf16={out_bf16}: max |err| / tolerance = {float(np.max(err / tol)):.3g}")
        assert np.all(err <= tol)
    exact, tol = ref.lse_reference(name, q, k, mask, scale)
    stored = np.isfinite(exact)
    assert np.array_equal(np.isneginf(lse), ~stored) and np.array_equal(np.isneginf(exact), ~stored)
    err = np.abs(lse[stored].astype(np.float64) - exact[stored])
    print(f"restated {name} {kind} lse: max |err| / tolerance = {float(np.max(err / tol[stored])):.3g}")
    assert np.all(err <= tol[stored])
    assert not out[~stored].any()


def test_the_restatement_returns_a_constant_column_of_v_to_fp32_accuracy():
    """The divisor is the sum of the weights the product multiplies by: with V constant, out is that constant to within
    (L + 16) 2^-24 relative, not 2^-9 -- and a divisor summed from the UNROUNDED weights would not be."""
    name, d = "edges16", 64
    q, k, _ = (x[0] for x in ref.operands(name, d, 8))
    p = pattern(name)
    length = np.repeat(np.diff(p.block_row_ptrs.astype(np.int64)) * 16, 16).astype(np.float64)
    for value in (1.0, -0.34765625):
        v = np.full((p.num_cols, 8), value, np.float32)
        out, _ = ref.fused_f32(name, q, k, v, None, d ** -0.5)
        rows = length > 0
        rel = np.abs(out[rows].astype(np.float64) / value - 1.0)
        assert np.all(rel <= ((length[rows] + 16) * 2.0 ** -24)[:, None]), float(rel.max())


def test_special_values_in_the_restatement_are_torchs():
    torch = pytest.importorskip("torch")
    name, d, dv = "ragged16", 8, 8
    p = pattern(name)
    q, k, v = (x[0] for x in ref.operands(name, d, dv))
    ptrs = p.block_row_ptrs.astype(np.int64)
    base = np.zeros((p.num_blocks, 16, 16), np.float32)
    r = 3                                                      # 7 blocks: four steps, the last a half step
    for what, want_lse in (("nan", np.nan), ("+inf", np.inf), ("all -inf", -np.inf), ("both", np.nan)):
        m = base.copy()
        if what in ("nan", "both"):
            m[ptrs[r] + 3, 5, 7] = np.nan
        if what in ("+inf", "both"):
            m[ptrs[r] + 1, 5, 0] = np.inf
        if what == "all -inf":
            m[ptrs[r]:ptrs[r + 1], 5, :] = -np.inf
        out, lse = ref.fused_f32(name, q, k, v, m, 0.3)
        clean, clean_lse = ref.fused_f32(name, q, k, v, base, 0.3)
        hit = np.zeros(out.shape[0], bool)
        hit[r * 16 + 5] = True
        assert np.array_equal(np.isnan(out), np.broadcast_to(hit[:, None], out.shape)), what
        assert np.array_equal(out[~hit], clean[~hit]) and np.array_equal(lse[~hit], clean_lse[~hit])
        z = torch.tensor([want_lse])
        assert np.array_equal(lse[hit], z.numpy().astype(np.float32), equal_nan=True), (what, lse[hit])


def test_python_layer_refuses_without_a_gpu_and_names_the_width_limit():
    torch = pytest.importorskip("torch")
    from mispmm import autograd, ops
    from test_softmax_bsr_cpu import _OnDevice
    bsr = pattern("ragged16")
    a = ops.DeviceBSR.from_host(bsr, device="cpu")
    q = torch.zeros((bsr.num_rows, 8), dtype=torch.int16)
    k = torch.zeros((bsr.num_cols, 8), dtype=torch.int16)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.attention_bsr_bf16(a, q, k, k)
    t = autograd.TrainableBSR.from_host(bsr, device="cpu")
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.block_sparse_attention(t, q.view(torch.bfloat16), k.view(torch.bfloat16), k.view(torch.bfloat16), fused=True)
    t.fwd.block_row_ptrs = _OnDevice(t.fwd.block_row_ptrs)
    a.block_row_ptrs = _OnDevice(a.block_row_ptrs)
    m, kk = bsr.num_rows, bsr.num_cols
    dev = lambda *shape, dtype=torch.bfloat16: _OnDevice(torch.zeros(*shape, dtype=dtype))   # noqa: E731
    for dq, dvv in ((12, 8), (136, 8), (8, 4), (8, 132), (8, 0)):
        with pytest.raises(ValueError, match="multiples of 8 up to 128"):
            autograd.block_sparse_attention(t, dev(m, dq), dev(kk, dq), dev(kk, dvv), fused=True)
        with pytest.raises(ValueError, match="multiples of 8 up to 128"):
            ops.attention_bsr_bf16(a, dev(m, dq, dtype=torch.int16), dev(kk, dq, dtype=torch.int16), dev(kk, dvv, dtype=torch.int16))
    bad = [lambda: autograd.block_sparse_attention(t, dev(m, 8, dtype=torch.float32), dev(kk, 8), dev(kk, 8), fused=True),
           lambda: autograd.block_sparse_attention(t, dev(2, m, 8), dev(kk, 8), dev(kk, 8), fused=True),
           lambda: autograd.block_sparse_attention(t, dev(2, m, 8), dev(3, kk, 8), dev(2, kk, 8), fused=True),
           lambda: autograd.block_sparse_attention(t, dev(m, 8), dev(kk, 16), dev(kk, 8), fused=True),
           lambda: autograd.block_sparse_attention(t, dev(m + 16, 8), dev(kk, 8), dev(kk, 8), fused=True),
           lambda: autograd.block_sparse_attention(t, _OnDevice(torch.zeros((8, m), dtype=torch.bfloat16).t()), dev(kk, 8), dev(kk, 8), fused=True),
           lambda: autograd.block_sparse_attention(t, dev(m, 8), dev(kk, 8), dev(kk, 8), mask=dev(3, 16, dtype=torch.float32), fused=True),
           lambda: ops.attention_bsr_bf16(a, dev(m, 8), dev(kk, 8), dev(kk, 8)),                                   # bits are int16
           lambda: ops.attention_bsr_bf16(a, dev(m, 8, dtype=torch.int16), dev(kk - 16, 8, dtype=torch.int16), dev(kk, 8, dtype=torch.int16)),
           lambda: ops.attention_bsr_bf16(a, dev(m, 8, dtype=torch.int16), dev(kk, 8, dtype=torch.int16), dev(kk, 8, dtype=torch.int16),
                                          out=dev(m, 8, dtype=torch.int16)),                                        # fp32 asked for
           lambda: ops.attention_bsr_bf16(a, dev(m, 8, dtype=torch.int16), dev(kk, 8, dtype=torch.int16), dev(kk, 8, dtype=torch.int16),
                                          lse=dev(m + 1, dtype=torch.float32))]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was not refused")


@pytest.mark.parametrize("name,kind", [("ragged16", "causal"), ("edges32", "leading"), ("ragged32", "none")])
def test_the_blockwise_tolerance_is_the_composed_one(name, kind):
    pytest.importorskip("torch")
    from test_gpu_softmax_bsr import _attention_tolerances
    q, k, v = (x[0] for x in ref.operands(name, 40, 72))
    mask, scale = ref.mask_of(name, kind), 40 ** -0.5
    for out_bf16 in (False, True):
        want = _attention_tolerances(name, q, k, v, np.zeros((q.shape[0], 72), np.float32), scale, mask, out_bf16)[0]
        assert np.allclose(ref.out_tolerance(name, q, k, v, scale, mask, out_bf16), want, rtol=1e-10, atol=0)
