"""Fused bf16 attention on a CSR pattern on a machine WITHOUT a GPU: the seventh library and its binding, the entry point's
argument validation (which precedes any device work), the census of the kernel's instances and tags, the contract restated in
numpy (tests/_attn_csr_bf16_ref.py) inside both tolerances and the derived tight check on every case the GPU suite runs, the
bf16-specific faults those checks must notice, and the refusals of the Python layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_attn_csr, capi_attn_csr_bf16

import _attn_csr_bf16_ref as bref
import _attn_csr_tight as tight
from _softmax_ref import matrix
from test_census_cpu import _symbol_tool

NAME = "mispmm_attn_csr_bf16"
INSTANCES = {"attn_csr_kernel": 9}       # __device_stub__ symbols of libmispmm_attn_csr_bf16.so per kernel template
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_has_one_export_and_header_and_binding_agree():
    assert os.path.exists(capi_attn_csr_bf16.LIB_PATH), f"{capi_attn_csr_bf16.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn_csr_bf16.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_attn_csr_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_attn_csr_bf16.SIGNATURES) == {NAME}
    # the declaration's parameter types, in order, against the binding's argtypes
    params = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    kinds = {"mispmm_stream_t": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
             "int": ctypes.c_int}
    want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
    assert want == capi_attn_csr_bf16.SIGNATURES[NAME][1] and len(want) == 26
    tool = _symbol_tool()
    if tool is not None:
        dyn = subprocess.run([tool, "-D", "--defined-only", capi_attn_csr_bf16.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in dyn.splitlines() if " T " in line and "mispmm_" in line}
        assert exported == {NAME}, exported
    lib = capi_attn_csr_bf16.lib()
    assert getattr(lib, NAME).argtypes == capi_attn_csr_bf16.SIGNATURES[NAME][1]
    # the tag and the error text are read through the handle of the library loaded here
    assert capi_attn_csr_bf16.last_kernel() == lib.mispmm_last_kernel().decode()
    for header in ("mispmm.h", "mispmm_attn_csr.h"):
        with open(os.path.join(ROOT, "include", header), encoding="utf-8") as f:
            assert NAME + "(" not in f.read()
    assert NAME not in capi.SIGNATURES and NAME not in capi_attn_csr.SIGNATURES


ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced


def _call(**kw):
    """Every call made through here is refused or a no-op: the pointers are fake."""
    a = dict(stream=None, H=2, M=4, K=64, nnz=8, ptrs=ONE, cols=ONE, q=ONE, qh=4096, ldq=64, k=ONE, kh=4096, ldk=64, D=64, v=ONE, vh=4096, ldv=64,
             Dv=64, scale=0.125, bias=None, bh=0, out=ONE, oh=4096, ldo=64, out_bf16=0, lse=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return getattr(capi_attn_csr_bf16.lib(), NAME)(*a.values())


def test_every_kind_of_bad_argument_is_refused_with_its_message_before_any_device_work():
    err = capi_attn_csr_bf16.last_error
    for name in ("ptrs", "cols", "q", "k", "v", "out"):
        assert _call(**{name: None}) == capi.ERR_INVALID_ARG, name
        assert "attn_csr_bf16" in err() and "null" in err()
    for kw in (dict(D=257, ldq=257, ldk=257), dict(Dv=257, ldv=257, ldo=257), dict(D=0), dict(Dv=0)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "attn_csr_bf16" in err() and "from 1 to 256" in err()
    for scale in (float("nan"), float("inf"), -float("inf")):
        assert _call(scale=scale) == capi.ERR_INVALID_ARG
        assert "scale must be finite" in err()
    for kw in (dict(ldq=56), dict(ldk=56), dict(ldv=56), dict(ldo=56)):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert "leading dimension smaller than the width" in err()
    # an odd base address of a bf16 operand; an fp32 out is not held to it here, a bf16 out is
    for kw in (dict(q=ONE + 1), dict(k=ONE + 1), dict(v=ONE + 1), dict(out=ONE + 1, out_bf16=1)):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert "2-byte aligned" in err()
    # one head of an operand spanning 2 GiB or more IN BYTES of its element type.  K = 2^24 rows of 64 bf16: 2^30 elements,
    # 2^31 bytes -- refused; one row less is 2^31 - 128 bytes and passes this check (the next test).  An fp32 out of 2^23 rows
    # of 64 is 2^31 bytes; a bf16 out reaches that at 2^24 rows.
    for kw in (dict(K=1 << 24, ldk=64), dict(K=1 << 27, ldk=8, D=8, ldq=8, ldv=1, Dv=1, ldo=1), dict(K=1 << 24, ldv=64),
               dict(M=1 << 24, ldq=64, out_bf16=1), dict(M=1 << 23, ldo=64, ldq=8, D=8, ldk=8), dict(M=1 << 24, ldo=64, out_bf16=1, ldq=8, D=8, ldk=8), dict(nnz=1 << 29, bias=ONE)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "2 GiB" in err()
        spans = [int(s) for s in re.search(r"\(([\d, ]+) bytes\)", err()).group(1).split(",")]
        assert max(spans) > 0x7FFFFFFF and max(spans) // 2 <= 0x7FFFFFFF or "nnz" in kw, "over the limit in bytes, under it in elements"
    assert _call(M=(1 << 25) + 1, H=1 << 12, ldq=1, ldo=1, D=1, Dv=1, ldk=1, ldv=1) == capi.ERR_UNSUPPORTED and "workgroups" in err()


def test_sizes_just_under_the_byte_limit_pass_the_size_check():
    # counted in bytes of the element type: (2^24 - 1) rows of 64 bf16 are 2^31 - 128 bytes.  The next check to fail is made to
    # be the odd base, which comes after the sizes: the message shows the size check let the shape through.
    err = capi_attn_csr_bf16.last_error
    for kw in (dict(K=(1 << 24) - 1, ldk=64), dict(M=(1 << 24) - 1, ldo=64, out_bf16=1, ldq=8, D=8, ldk=8), dict(M=(1 << 23) - 1, ldo=64, ldq=8, D=8, ldk=8)):
        assert _call(q=ONE + 1, **kw) == capi.ERR_INVALID_ARG, kw
        assert "2-byte aligned" in err()


def test_no_ops_return_before_any_pointer_is_looked_at():
    nothing = dict(ptrs=None, cols=None, q=None, k=None, v=None, out=None)
    assert _call(H=0, **nothing) == capi.OK
    assert _call(M=0, **nothing) == capi.OK
    assert _call(M=0, q=ONE + 1) == capi.OK
    assert _call(H=0, scale=float("nan")) == capi.ERR_INVALID_ARG          # ... but after the checks that need none
    assert _call(M=0, D=300, ldq=300, ldk=300) == capi.ERR_UNSUPPORTED


def _symbols(path):
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    return subprocess.run([tool, "-C", path], capture_output=True, text=True, check=True).stdout


def test_the_library_holds_nine_instances_of_one_template_and_the_tag_table_lists_each():
    out = _symbols(capi_attn_csr_bf16.LIB_PATH)
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found == INSTANCES, f"kernel template: instances in the library {found}, recorded here {INSTANCES}"
    tags = set()
    for args in set(re.findall(r"__device_stub__attn_csr_kernel<([^>]*)>", out)):
        elem, *consts = (s.strip() for s in args.split(","))          # the element policy, then G, VEC, NCH
        assert elem.endswith("::ElemBf16"), args
        g, vec, nch = (int(s) for s in consts)
        tags.add(f"attn_csr_bf16<G{g},V{vec},C{nch}>")
    assert tags == set(bref.TAGS), (sorted(tags - set(bref.TAGS)), sorted(set(bref.TAGS) - tags))
    assert len(bref.TAGS) == INSTANCES["attn_csr_kernel"] == 3 + 6
    for tag, (d, dv, aligned) in bref.TAGS.items():
        assert bref.tag_of(d, dv, aligned) == tag
        # the smallest shape: one step less in either width is refused or lands on another tag
        step = 8 if "V8" in tag else 1
        for dd, ddv in ((d - step, dv), (d, dv - step)):
            assert dd == 0 or ddv == 0 or bref.tag_of(dd, ddv, aligned) != tag
        assert max(d, dv) <= 256
    assert bref.tag_of(256, 256, True) == "attn_csr_bf16<G32,V8,C1>" and bref.tag_of(256, 252, True) == "attn_csr_bf16<G64,V1,C4>"
    assert bref.tag_of(100, 36, True) == "attn_csr_bf16<G64,V1,C2>"           # multiples of 4 are not enough: there is no 8-byte form
    # every case of the suite lands on a tag of the table, and the V8 / V1 split is the one the issue lists
    assert {bref.tag_of(d, dv, True).split(",")[1] for d, dv in bref.WIDTHS[:5]} == {"V8"}
    assert {bref.tag_of(d, dv, True).split(",")[1] for d, dv in bref.WIDTHS[5:]} == {"V1"}
    assert bref.tag_of(1, 129, True).endswith("C4>")
    # the other libraries are untouched by the new kernel: no such symbol there
    for path in (capi.LIB_PATH, capi_attn_csr.LIB_PATH):
        assert "attn_csr_bf16" not in _symbols(path), path


def test_the_cases_are_what_the_issue_lists_and_their_operands_are_bf16_with_exact_scores():
    assert len(bref.CASES) == 2 * 9 * 3 * 2 and len({c.id for c in bref.CASES}) == len(bref.CASES)
    assert set(bref.WIDTHS) == {(8, 64), (64, 8), (40, 72), (128, 128), (256, 256), (3, 5), (1, 1), (100, 36), (1, 129)}
    for case in bref.CASES:
        op, csr = bref.operands(case), matrix(case.name)
        for n in ("q", "k", "v"):
            assert bref.is_bf16(op[n]), (case.id, n)                                 # q and k survive the rounding: 8 significant bits
            assert np.array_equal(bref.widen(bref.to_bits(op[n])), op[n])
        assert np.all((np.abs(op["q"]) * 256 >= 64) & (np.abs(op["q"]) * 256 <= 192)) and np.array_equal(op["q"] * 256, np.rint(op["q"] * 256))
        assert tight.exact_scores(csr, op["q"], op["k"], op["scale"], op["bias"]), case.id
        assert op["k"].shape == (1, csr.num_cols, case.d) and op["v"].shape == (1, csr.num_cols, case.dv)
        assert np.unique(np.abs(op["v"])).size > 100 or case.dv * csr.num_cols < 2000     # v has more than a grid's values
        if case.bias == "finite" and case.heads > 1:
            assert op["bias"].shape == (case.heads, csr.nnz)
        if case.bias == "masked":
            assert np.isneginf(op["bias"]).any() and op["bias"].ndim == 1


@pytest.mark.parametrize("case", bref.CASES, ids=lambda c: c.id)
def test_the_restatement_lies_inside_both_tolerances_and_the_tight_check(case):
    got = bref.restated(case)
    assert not np.isnan(got["out"]).any()
    results = {what: check(got, case) for what, check in bref.CHECKS.items()}
    print(f"restated {case.id}: worst |err| / tolerance: " + ", ".join(f"{what} {worst:.3g}" for what, (_, worst) in results.items()))
    for what, (ok, worst) in results.items():
        assert ok and worst <= 1.0, (what, worst)


# a fault and cases on which it must be noticed: even widths for the pair swaps, ldk != ldv for the stride
FAULT_CASES = {
    "k_pair_swapped": (bref.Case("edges", 8, 64, "none", 1), bref.Case("ragged", 40, 72, "finite", 3)),
    "v_pair_swapped": (bref.Case("edges", 8, 64, "none", 1), bref.Case("ragged", 100, 36, "masked", 1)),
    "out_truncated": (bref.Case("edges", 3, 5, "none", 1), bref.Case("ragged", 128, 128, "finite", 3)),
    "v_at_k_offset": (bref.Case("edges", 40, 72, "none", 1), bref.Case("ragged", 64, 8, "masked", 3)),
}


@pytest.mark.parametrize("fault", sorted(bref.FAULTS))
def test_the_checks_notice_every_bf16_specific_fault(fault):
    assert set(FAULT_CASES) == set(bref.FAULTS)
    for case in FAULT_CASES[fault]:
        assert case in bref.CASES
        if fault == "v_at_k_offset":
            assert case.d + bref.PAD != case.dv + bref.PAD, "the case must have ldk != ldv"
        got = bref.restated(case, fault)
        results = {what: check(got, case) for what, check in bref.CHECKS.items()}
        caught = [what for what, (ok, _) in results.items() if not ok]
        print(f"{fault} on {case.id}: rejected by {caught}")
        assert caught, f"{fault} ({bref.FAULTS[fault]}) passes every check on {case.id}"
        # ... and the fault is what they reject: the honest restatement of the same case passes them all
        assert all(ok for ok, _ in (check(bref.restated(case), case) for check in bref.CHECKS.values()))
    # truncation is no rounding to nearest even: it is caught by the rounding check and by no other (the fp32 out is honest)
    if fault == "out_truncated":
        assert caught == ["rounded_once"]


def test_python_layer_refuses_every_defect_on_cpu_tensors_and_cpu_tensors_as_such():
    torch = pytest.importorskip("torch")
    from mispmm import autograd, ops
    from mispmm.attn_csr_bf16 import attention_csr_bf16
    csr = matrix("long")
    a = ops.DeviceCSR.from_host(csr, device="cpu")
    m, kk, nnz = csr.num_rows, csr.num_cols, csr.nnz
    bits = lambda *shape: torch.zeros(shape, dtype=torch.int16)            # noqa: E731
    q, k, v = bits(m, 8), bits(kk, 8), bits(kk, 16)

    def refused(match, **kw):
        args = dict(q=q, k=k, v=v)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            attention_csr_bf16(a, args.pop("q"), args.pop("k"), args.pop("v"), **args)

    # wrong dtype
    refused("q must be an int16 tensor of bf16 bits", q=torch.zeros((m, 8)))
    refused("k must be an int16 tensor of bf16 bits", k=torch.zeros((kk, 8), dtype=torch.bfloat16))
    refused("v must be an int16 tensor of bf16 bits", v=torch.zeros((kk, 16), dtype=torch.int32))
    refused("bias must be a float32", bias=torch.zeros(nnz, dtype=torch.float64))
    refused("lse must be a contiguous float32", lse=torch.zeros(m, dtype=torch.float64))
    # wrong rank
    refused("q must be", q=bits(m * 8))
    refused("q, k and v must all be 2-D", k=bits(1, kk, 8))
    refused("v must be", v=bits(1, 1, kk, 16))
    # wrong shape against a
    refused("q must be", q=bits(m + 1, 8))
    refused("k must be", k=bits(kk - 1, 8))
    refused("v must be", q=bits(2, m, 8), k=bits(2, kk, 8), v=bits(3, kk, 16))
    refused("same number of columns", k=bits(kk, 16))
    refused("widths from 1 to 256: v", v=bits(kk, 264))
    refused("bias must have shape", bias=torch.zeros(nnz + 1))
    refused("bias must have shape", bias=torch.zeros((2, nnz)))
    refused("out must be a float32 tensor .* of shape", out=torch.zeros((m, 8)))
    refused("lse must be a contiguous float32", lse=torch.zeros(m + 1))
    # column stride != 1
    refused("q must have unit column stride", q=bits(m, 16)[:, ::2])
    refused("v must have unit column stride", v=bits(16, kk).t())
    refused("bias must have unit stride", bias=torch.zeros(2 * nnz)[::2])
    refused("out must have unit column stride", out=torch.zeros((m, 32))[:, ::2])
    # rows that overlap
    refused("k must not overlap its own rows", k=bits(1, 8).expand(kk, 8))
    refused("out must have unit column stride and rows", out=torch.zeros((1, 16)).expand(m, 16))
    # negative strides cannot be made by torch views; the check stands for tensors that come from elsewhere (it is exercised
    # through a stand-in below)
    class Reversed:                                                         # what a flipped view of another library looks like
        dtype, shape, is_cuda = torch.int16, (kk, 8), False

        def dim(self):
            return 2

        def unsqueeze(self, _):
            return Reversed3()

    class Reversed3(Reversed):
        shape = (1, kk, 8)

        def dim(self):
            return 3

        def stride(self, i=None):
            s = (0, -8, 1)
            return s if i is None else s[i]
    refused("k must not have a negative stride", k=Reversed())
    # an out whose dtype does not fit out_bf16
    refused("out must be an int16 tensor of bf16 bits", out=torch.zeros((m, 16)), out_bf16=True)
    refused("out must be a float32 tensor", out=bits(m, 16), out_bf16=False)
    # a non-contiguous lse
    refused("lse must be a contiguous float32", lse=torch.zeros((m, 2))[:, 0])
    # a float64 matrix
    with pytest.raises(ValueError, match="float32 DeviceCSR"):
        attention_csr_bf16(ops.DeviceCSR.from_host(csr, device="cpu", dtype=torch.float64), q, k, v)
    # CPU tensors as such: well-formed operands, every combination of results
    refused("no CPU path")
    refused("no CPU path", bias=torch.zeros(nnz), out=torch.zeros((m, 16)), lse=torch.zeros(m), return_lse=True)
    refused("no CPU path", out=bits(m, 16), out_bf16=True)
    refused("no CPU path", q=bits(2, m, 8), k=bits(1, kk, 8).expand(2, kk, 8), v=bits(2, kk, 16), bias=torch.zeros((2, nnz)))
    t = autograd.TrainableCSR.from_host(csr, device="cpu")
    qb, kb, vb = (x.view(torch.bfloat16) for x in (q, k, v))
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.sparse_attention_bf16(t, qb, kb, vb)
