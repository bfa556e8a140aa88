"""Fused attention on a CSR pattern on a machine WITHOUT a GPU: the fifth library and its binding, the entry point's argument
validation (which precedes any device work), the census of the kernel's instances and tags, and the algorithm as built,
restated in numpy float32 (tests/_attn_csr_ref.py::fused_f32), inside both tolerances and the derived tight check on every
case the GPU suite runs."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_attn_csr

import _attn_csr_mutants as mut
import _attn_csr_ref as ref
import _attn_csr_tight as tight
from _softmax_ref import matrix
from test_census_cpu import _symbol_tool

INSTANCES = {"attn_csr_kernel": 10}       # __device_stub__ symbols of libmispmm_attn_csr.so per kernel template
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_has_one_export_and_header_and_binding_agree():
    assert os.path.exists(capi_attn_csr.LIB_PATH), f"{capi_attn_csr.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn_csr.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_attn_csr_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_attn_csr.SIGNATURES) == {"mispmm_attn_csr_f32"}
    # the declaration's parameter types, in order, against the binding's argtypes
    params = re.search(r"mispmm_attn_csr_f32\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    kinds = {"mispmm_stream_t": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
    assert want == capi_attn_csr.SIGNATURES["mispmm_attn_csr_f32"][1]
    tool = _symbol_tool()
    if tool is not None:
        dyn = subprocess.run([tool, "-D", "--defined-only", capi_attn_csr.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in dyn.splitlines() if " T " in line and "mispmm_" in line}
        assert exported == {"mispmm_attn_csr_f32"}, exported
    lib = capi_attn_csr.lib()
    assert lib.mispmm_attn_csr_f32.argtypes == capi_attn_csr.SIGNATURES["mispmm_attn_csr_f32"][1]
    # the tag and the error text are read through the handle of the library loaded here
    assert capi_attn_csr.last_kernel() == lib.mispmm_last_kernel().decode()
    with open(os.path.join(ROOT, "include", "mispmm.h"), encoding="utf-8") as f:
        assert "mispmm_attn_csr_f32(" not in f.read()
    assert not any(n.startswith("mispmm_attn_csr") for n in capi.SIGNATURES)


ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced


def _call(**kw):
    """Every call made through here is refused or a no-op: the pointers are fake."""
    a = dict(stream=None, H=2, M=4, K=64, nnz=8, ptrs=ONE, cols=ONE, q=ONE, qh=4096, ldq=64, k=ONE, kh=4096, ldk=64, D=64, v=ONE, vh=4096, ldv=64,
             Dv=64, scale=0.125, bias=None, bh=0, out=ONE, oh=4096, ldo=64, lse=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_attn_csr.lib().mispmm_attn_csr_f32(*a.values())


def test_every_kind_of_bad_argument_is_refused_with_its_message_before_any_device_work():
    err = capi_attn_csr.last_error
    for name in ("ptrs", "cols", "q", "k", "v", "out"):
        assert _call(**{name: None}) == capi.ERR_INVALID_ARG, name
        assert "attn_csr_f32" in err() and "null" in err()
    for kw in (dict(D=257, ldq=257, ldk=257), dict(Dv=257, ldv=257, ldo=257), dict(D=0), dict(Dv=0)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "from 1 to 256" in err()
    for scale in (float("nan"), float("inf"), -float("inf")):
        assert _call(scale=scale) == capi.ERR_INVALID_ARG
        assert "scale must be finite" in err()
    for kw in (dict(ldq=56), dict(ldk=56), dict(ldv=56), dict(ldo=56)):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert "leading dimension smaller than the width" in err()
    # one head of an operand spanning 2 GiB or more, as sddmm_csr declines it
    for kw in (dict(K=1 << 24, ldk=64), dict(K=1 << 24, ldk=8, D=8, ldq=8), dict(M=1 << 21, ldq=1024), dict(M=1 << 24, ldo=64),
               dict(nnz=1 << 30, bias=ONE)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "2 GiB" in err()
    assert _call(M=(1 << 25) + 1, H=1 << 12, ldq=1, ldo=1, D=1, Dv=1, ldk=1, ldv=1) == capi.ERR_UNSUPPORTED and "workgroups" in err()


def test_no_ops_return_before_any_pointer_is_looked_at():
    nothing = dict(ptrs=None, cols=None, q=None, k=None, v=None, out=None)
    assert _call(H=0, **nothing) == capi.OK
    assert _call(M=0, **nothing) == capi.OK
    assert _call(H=0, scale=float("nan")) == capi.ERR_INVALID_ARG          # ... but after the checks that need none
    assert _call(M=0, D=300, ldq=300, ldk=300) == capi.ERR_UNSUPPORTED


def _symbols():
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    return subprocess.run([tool, "-C", capi_attn_csr.LIB_PATH], capture_output=True, text=True, check=True).stdout


def test_the_library_holds_the_recorded_instances_and_the_tag_table_lists_each():
    out = _symbols()
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found == INSTANCES, f"kernel template: instances in the library {found}, recorded here {INSTANCES}"
    tags = set()
    for args in set(re.findall(r"__device_stub__attn_csr_kernel<([^>]*)>", out)):
        elem, *consts = (s.strip() for s in args.split(","))          # the element policy, then G, VEC, NCH
        assert elem.endswith("::ElemF32"), args
        g, vec, nch = (int(s) for s in consts)
        tags.add(f"attn_csr<f32,G{g},V{vec},C{nch}>")
    assert tags == set(ref.TAGS), (sorted(tags - set(ref.TAGS)), sorted(set(ref.TAGS) - tags))
    assert len(ref.TAGS) == INSTANCES["attn_csr_kernel"]
    for tag, (d, dv, aligned) in ref.TAGS.items():
        assert ref.tag_of(d, dv, aligned) == tag
        # the smallest shape: one step less in either width is refused or lands on another tag
        step = 4 if "V4" in tag else 1
        for dd, ddv in ((d - step, dv), (d, dv - step)):
            assert dd == 0 or ddv == 0 or ref.tag_of(dd, ddv, aligned) != tag
        # ... and the widest of every tag's range is still inside 256
        assert max(d, dv) <= 256
    assert ref.tag_of(256, 256, True) == "attn_csr<f32,G64,V4,C1>" and ref.tag_of(256, 255, True) == "attn_csr<f32,G64,V1,C4>"
    # csrc/ and the first library are untouched by the new kernel: no such symbol there
    first = subprocess.run([_symbol_tool(), "-C", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "attn_csr" not in first


def test_the_cases_are_what_the_issue_lists_and_their_scores_are_exact():
    assert len(ref.CASES) == 2 * 7 * 3 * 2 and len({c.id for c in ref.CASES}) == len(ref.CASES)
    lens = np.diff(matrix("edges").row_ptrs.astype(np.int64))
    assert lens.shape[0] == 32 and {0, 1, 7, 8, 9, 257, 300, 1025} <= set(lens.tolist()) and lens[0] == 0 and lens[-1] == 0
    for case in ref.CASES:
        op, csr = ref.operands(case), matrix(case.name)
        assert tight.exact_scores(csr, op["q"], op["k"], op["scale"], op["bias"]), case.id
        assert op["k"].shape[0] == 1 and op["v"].shape[0] == 1                       # shared by the heads: head stride 0
        if case.bias == "masked":
            ptrs = csr.row_ptrs.astype(np.int64)
            masked = np.isneginf(op["bias"])
            whole = [r for r in range(csr.num_rows) if ptrs[r + 1] - ptrs[r] > 16 and masked[ptrs[r]:ptrs[r] + 16].all()]
            assert len(whole) >= 3 and op["bias"].ndim == 1
            assert all(np.isfinite(op["bias"][ptrs[r + 1] - 1]) for r in range(csr.num_rows) if ptrs[r + 1] > ptrs[r])
        if case.bias == "finite" and case.heads > 1:
            assert op["bias"].shape == (case.heads, csr.nnz)


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.id)
def test_the_algorithm_as_built_lies_inside_both_tolerances_and_the_tight_check(case):
    got = mut.restated(case)
    assert not np.isnan(got["out"]).any()
    results = {what: check(got, case) for what, check in mut.CHECKS.items()}
    print(f"restated {case.id}: worst |err| / tolerance: " + ", ".join(f"{what} {worst:.3g}" for what, (_, worst) in results.items()))
    for what, (ok, worst) in results.items():
        assert ok and worst <= 1.0, (what, worst)


@pytest.mark.parametrize("name", ["long", "ragged"])
def test_the_out_tolerance_is_the_chains_on_a_single_head_without_a_bias(name):
    pytest.importorskip("torch")
    from test_gpu_softmax import _attention_tolerances
    from _softmax_ref import full_mantissa
    csr = matrix(name)
    rng = np.random.default_rng(46)
    for d in (8, 64):
        q, k, v = (full_mantissa(rng, (n, d), np.float32) for n in (csr.num_rows, csr.num_cols, csr.num_cols))
        want = _attention_tolerances(csr, q, k, v, np.zeros((csr.num_rows, d), np.float32), d ** -0.5, "fast")[0]
        assert np.allclose(ref.out_tolerance(csr, q[None], k[None], v[None], d ** -0.5)[0], want, rtol=1e-10, atol=0)


def test_the_entrywise_reference_is_dense_masked_attention():
    for case in (ref.Case("edges", 3, 5, "masked", 3), ref.Case("ragged", 8, 64, "finite", 1)):
        op, csr = ref.operands(case), matrix(case.name)
        args = (csr, op["q"], op["k"], op["v"], op["scale"], op["bias"])
        assert np.allclose(ref.attention_f64(*args)[0], ref.dense_f64(*args), rtol=1e-12, atol=1e-15)


def test_special_values_in_the_restatement_are_torchs():
    torch = pytest.importorskip("torch")
    case = ref.Case("edges", 8, 8, "finite", 1)
    op, csr = dict(ref.operands(case)), matrix("edges")
    ptrs = csr.row_ptrs.astype(np.int64)
    lens = np.diff(ptrs)
    r = int(np.argwhere(lens == 33)[0, 0])
    clean = ref.fused_f32(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"])
    for what, want_lse in (("nan", np.nan), ("+inf", np.inf), ("all -inf", -np.inf), ("both", np.nan)):
        b = op["bias"].copy()
        if what in ("nan", "both"):
            b[ptrs[r] + 20] = np.nan
        if what in ("+inf", "both"):
            b[ptrs[r] + 3] = np.inf
        if what == "all -inf":
            b[ptrs[r]:ptrs[r + 1]] = -np.inf
        out, lse = ref.fused_f32(csr, op["q"], op["k"], op["v"], op["scale"], b)
        hit = np.zeros(csr.num_rows, bool)
        hit[r] = True
        assert np.array_equal(np.isnan(out[0]), np.broadcast_to(hit[:, None], out[0].shape)), what
        assert np.array_equal(out[0][~hit], clean[0][0][~hit]) and np.array_equal(lse[0][~hit], clean[1][0][~hit])
        z = torch.logsumexp(torch.tensor([{"nan": [np.nan, 0.0], "+inf": [np.inf, 0.0], "all -inf": [-np.inf, -np.inf], "both": [np.inf, np.nan]}[what]]), dim=1)
        assert np.array_equal(lse[0][hit], z.numpy().astype(np.float32), equal_nan=True) and (np.isnan(want_lse) or lse[0][r] == want_lse), what


def test_python_layer_refuses_without_a_gpu():
    torch = pytest.importorskip("torch")
    from mispmm import autograd, ops
    csr = matrix("long")
    a = ops.DeviceCSR.from_host(csr, device="cpu")
    q, k = torch.zeros((csr.num_rows, 8)), torch.zeros((csr.num_cols, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.attention_csr(a, q, k, k)
    t = autograd.TrainableCSR.from_host(csr, device="cpu")
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.sparse_attention(t, q, k, k, fused=True)
