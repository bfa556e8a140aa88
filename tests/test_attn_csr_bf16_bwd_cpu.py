"""The fused bf16 backward of attention on a CSR pattern on a machine WITHOUT a GPU: the eighth library and its binding, the
entry point's argument validation (which precedes any device work), the census of the two kernels' instances and tags, both
passes as built restated in numpy (tests/_attn_csr_bf16_bwd_ref.py) inside the derived tolerances and the tight check on every
case the GPU suite runs, the faults those checks must notice, and the refusals of the Python layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_attn_csr_bf16, capi_attn_csr_bf16_bwd, capi_attn_csr_bwd

import _attn_csr_bf16_bwd_ref as bb
import _attn_csr_bf16_ref as fref
import _attn_csr_tight as tight
from _softmax_ref import matrix
from test_census_cpu import _symbol_tool

NAME = "mispmm_attn_csr_bf16_bwd"
INSTANCES = {"attn_csr_bwd_row_kernel": 9, "attn_csr_bwd_col_kernel": 9}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_has_one_export_and_header_and_binding_agree():
    assert os.path.exists(capi_attn_csr_bf16_bwd.LIB_PATH), f"{capi_attn_csr_bf16_bwd.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn_csr_bf16_bwd.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_attn_csr_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_attn_csr_bf16_bwd.SIGNATURES) == {NAME}
    params = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    kinds = {"mispmm_stream_t": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
             "int": ctypes.c_int}
    want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
    assert want == capi_attn_csr_bf16_bwd.SIGNATURES[NAME][1] and len(want) == 42
    tool = _symbol_tool()
    if tool is not None:
        dyn = subprocess.run([tool, "-D", "--defined-only", capi_attn_csr_bf16_bwd.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in dyn.splitlines() if " T " in line and "mispmm_" in line}
        assert exported == {NAME}, exported
    lib = capi_attn_csr_bf16_bwd.lib()
    assert getattr(lib, NAME).argtypes == capi_attn_csr_bf16_bwd.SIGNATURES[NAME][1]
    assert capi_attn_csr_bf16_bwd.last_kernel() == lib.mispmm_last_kernel().decode()
    for header in ("mispmm.h", "mispmm_attn_csr.h", "mispmm_attn_csr_bwd.h", "mispmm_attn_csr_bf16.h"):
        with open(os.path.join(ROOT, "include", header), encoding="utf-8") as f:
            assert NAME + "(" not in f.read()
    for other in (capi, capi_attn_csr_bwd, capi_attn_csr_bf16):
        assert NAME not in other.SIGNATURES


ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced
FAR = 1 << 40                              # fake pointers far apart: no two operands overlap


def _call(**kw):
    """Every call made through here is refused or a no-op: the pointers are fake."""
    far = lambda i: FAR * (i + 1)                                        # noqa: E731
    a = dict(stream=None, H=2, M=4, K=64, nnz=8, ptrs=ONE, cols=ONE, tptrs=ONE, tcols=ONE, perm=ONE, q=far(0), qh=4096, ldq=64, k=far(1), kh=4096,
             ldk=64, D=64, v=far(2), vh=4096, ldv=64, Dv=64, scale=0.125, bias=None, bh=0, out=far(3), oh=4096, ldo=64, lse=far(4), g=far(5), gh=4096,
             ldg=64, delta=far(6), grads_bf16=1, dq=far(7), dqh=4096, lddq=64, dk=far(8), dkh=4096, lddk=64, dv=far(9), dvh=4096, lddv=64)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return getattr(capi_attn_csr_bf16_bwd.lib(), NAME)(*a.values())


def test_every_kind_of_bad_argument_is_refused_with_its_message_before_any_device_work():
    err = capi_attn_csr_bf16_bwd.last_error
    for kw in (dict(D=257, ldq=257, ldk=257), dict(Dv=257, ldv=257, ldo=257), dict(D=0), dict(Dv=0)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "attn_csr_bf16_bwd" in err() and "from 1 to 256" in err()
    for scale in (float("nan"), float("inf"), -float("inf")):
        assert _call(scale=scale) == capi.ERR_INVALID_ARG
        assert "attn_csr_bf16_bwd: scale must be finite" in err()
    for name in ("ptrs", "cols", "q", "k", "v"):
        assert _call(**{name: None}) == capi.ERR_INVALID_ARG, name
        assert err() == "attn_csr_bf16_bwd: rowPtrs, colIdxs, Q, K or V is null"
    for name in ("out", "lse", "g", "delta"):
        assert _call(**{name: None}) == capi.ERR_INVALID_ARG, name
        assert err() == "attn_csr_bf16_bwd: out, lse, grad_out or delta is null"
    assert _call(delta=None, dq=None, dk=None, q=FAR + 1) == capi.ERR_INVALID_ARG and "2-byte aligned" in err()      # dV alone needs no delta
    for kw in (dict(tptrs=None), dict(tcols=None), dict(tcols=None, dq=None, dk=None)):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert err() == "attn_csr_bf16_bwd: dK and dV need the pattern of A^T: tRowPtrs or tColIdxs is null"
    assert _call(bias=FAR * 20, perm=None) == capi.ERR_INVALID_ARG
    assert err() == "attn_csr_bf16_bwd: with a bias, dK and dV need perm, which is null"
    for kw in (dict(ldq=56), dict(ldk=56), dict(ldv=56), dict(ldo=56), dict(ldg=56), dict(lddq=56), dict(lddk=56), dict(lddv=56)):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert "attn_csr_bf16_bwd: leading dimension smaller than the width" in err()
    assert _call(lddq=56, dq=None, q=FAR + 1) == capi.ERR_INVALID_ARG and "2-byte aligned" in err()  # an output not asked for is not looked at
    # one head of an operand spanning 2 GiB or more IN BYTES of its own element type.  2^24 rows of 64 bf16: 2^30 elements,
    # 2^31 bytes -- refused; the fp32 out reaches that at 2^23 rows of 64, the bias at 2^29 entries.
    small = dict(ldq=8, D=8, ldk=8, lddq=8, lddk=8)
    for kw, who in ((dict(K=1 << 24, ldk=64), 1), (dict(K=1 << 24, ldv=64, **small), 2), (dict(M=1 << 24, ldq=64, ldo=1, ldg=1, Dv=1, ldv=1, lddv=1), 0),
                    (dict(M=1 << 24, ldg=64, ldo=64, **small), 3), (dict(M=1 << 23, ldo=64, **small), 3), (dict(nnz=1 << 29, bias=FAR * 20), 5)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "attn_csr_bf16_bwd: Q, K, V, out, grad_out or bias of one head spans 2 GiB or more" in err()
        spans = [int(s) for s in re.search(r"\(([\d, ]+) bytes\)", err()).group(1).split(",")]
        assert len(spans) == 6 and spans[who] > 0x7FFFFFFF, (kw, spans)
        if "nnz" not in kw and kw.get("M") != 1 << 23:
            assert max(spans[i] for i in (0, 1, 2, 4)) // 2 <= 0x7FFFFFFF, "over the limit in bytes, under it in elements"
    assert _call(M=(1 << 25) + 1, H=1 << 12, ldq=1, ldo=1, ldg=1, D=1, Dv=1, ldk=1, ldv=1, lddq=1, lddk=1, lddv=1) == capi.ERR_UNSUPPORTED \
        and "attn_csr_bf16_bwd" in err() and "workgroups" in err()
    # an odd base address of a bf16 operand; an fp32 gradient is not held to it here, a bf16 gradient is
    for kw in (dict(q=FAR + 1), dict(k=2 * FAR + 1), dict(v=3 * FAR + 1), dict(g=6 * FAR + 1), dict(dq=8 * FAR + 1), dict(dk=9 * FAR + 1),
               dict(dv=10 * FAR + 1)):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert err() == "attn_csr_bf16_bwd: Q, K, V, grad_out and bf16 gradients must be 2-byte aligned"
    assert _call(dq=8 * FAR + 1, grads_bf16=0, dk=FAR) == capi.ERR_INVALID_ARG and "overlaps an input" in err()
    # overlaps, on extents in BYTES of each operand's own type: H = 2 heads of Q (4 rows of 64 bf16 at head stride 4096) end
    # (4096 + 3 * 64 + 64) * 2 = 8704 bytes past the base; a gradient that begins on the last byte pair is refused, one that
    # begins right behind is not.  In elements of 4 bytes the same operand would reach twice as far.
    q = FAR
    end = (4096 + 3 * 64 + 64) * 2
    for kw in (dict(dq=q), dict(dk=q + end - 2), dict(dv=q + 2), dict(delta=q + end - 4)):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert err() == "attn_csr_bf16_bwd: dQ, dK, dV or delta overlaps an input"
    # ... and of out (fp32: 4 bytes an element) and lse (H * M floats)
    o_end = (4096 + 3 * 64 + 64) * 4
    assert _call(dq=4 * FAR + o_end - 2) == capi.ERR_INVALID_ARG and "overlaps an input" in err()
    assert _call(dk=5 * FAR + 2 * 4 * 4 - 2) == capi.ERR_INVALID_ARG and "overlaps an input" in err()
    # a bf16 gradient's own extent: dQ covers (4096 + 3 * 64 + 64) * 2 bytes, an fp32 one twice that
    for kw, code in ((dict(dk=8 * FAR + end - 2), "one another"), (dict(delta=8 * FAR + end - 2), "one another"),
                     (dict(dk=8 * FAR + 2 * end - 4, grads_bf16=0), "one another")):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert err() == "attn_csr_bf16_bwd: dQ, dK, dV and delta overlap one another"


def test_sizes_just_under_the_byte_limit_pass_the_size_check():
    # counted in bytes of the element type: (2^24 - 1) rows of 64 bf16 are 2^31 - 128 bytes.  The next check to fail is made to
    # be the odd base, which comes after the sizes: the message shows the size check let the shape through.
    err = capi_attn_csr_bf16_bwd.last_error
    small = dict(ldq=8, D=8, ldk=8, lddq=8, lddk=8)
    for kw in (dict(K=(1 << 24) - 1, ldk=64), dict(M=(1 << 24) - 1, ldg=64, ldo=32, Dv=32, ldv=32, lddv=32, **small), dict(M=(1 << 23) - 1, ldo=64, **small),
               dict(nnz=(1 << 29) - 1, bias=FAR * 20)):
        assert _call(q=FAR + 1, **kw) == capi.ERR_INVALID_ARG, kw
        assert "2-byte aligned" in err()
    # an extent just behind an input does not overlap it: refused for the odd base only
    end = (4096 + 3 * 64 + 64) * 2
    assert _call(dq=FAR + end, g=6 * FAR + 1) == capi.ERR_INVALID_ARG and "2-byte aligned" in err()


def test_no_ops_return_before_any_pointer_is_looked_at():
    nothing = dict(ptrs=None, cols=None, tptrs=None, tcols=None, perm=None, q=None, k=None, v=None, out=None, lse=None, g=None, delta=None)
    assert _call(H=0, **nothing) == capi.OK
    assert _call(M=0, **nothing) == capi.OK
    assert _call(dq=None, dk=None, dv=None, **nothing) == capi.OK
    assert _call(M=0, q=FAR + 1) == capi.OK
    assert _call(H=0, scale=float("nan")) == capi.ERR_INVALID_ARG          # ... but after the checks that need none
    assert _call(M=0, D=300, ldq=300, ldk=300) == capi.ERR_UNSUPPORTED


def _symbols(path):
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    return subprocess.run([tool, "-C", path], capture_output=True, text=True, check=True).stdout


def test_the_library_holds_nine_instances_per_pass_and_the_tag_table_lists_each():
    out = _symbols(capi_attn_csr_bf16_bwd.LIB_PATH)
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found == INSTANCES, f"kernel templates: instances in the library {found}, recorded here {INSTANCES}"
    tags = set()
    for kind in ("row", "col"):
        for args in set(re.findall(rf"__device_stub__attn_csr_bwd_{kind}_kernel<([^>]*)>", out)):
            elem, *consts = (s.strip() for s in args.split(","))          # the element policy, then G, VEC, NCH
            assert elem.endswith("::ElemBf16"), args
            g, vec, nch = (int(s) for s in consts)
            tags.add(f"attn_csr_bf16_bwd_{kind}<G{g},V{vec},C{nch}>")
    assert tags == set(bb.TAGS), (sorted(tags - set(bb.TAGS)), sorted(set(bb.TAGS) - tags))
    assert len(bb.TAGS) == sum(INSTANCES.values()) == 18
    for tag, (d, dv, aligned) in bb.TAGS.items():
        assert tag in bb.tags_of(d, dv, aligned)
        assert [t.split("<")[1] for t in bb.tags_of(d, dv, aligned)] == [fref.tag_of(d, dv, aligned).split("<")[1]] * 2      # the forward's list, both passes
    assert bb.tags_of(64, 64, True, (True, False, False)) == ["attn_csr_bf16_bwd_row<G8,V8,C1>"]
    assert bb.tags_of(64, 64, True, (False, False, True)) == ["attn_csr_bf16_bwd_col<G8,V8,C1>"]
    assert bb.tags_of(64, 64, True, (False, True, False)) == ["attn_csr_bf16_bwd_row<G8,V8,C1>", "attn_csr_bf16_bwd_col<G8,V8,C1>"]
    assert bb.fp32_tag("attn_csr_bf16_bwd_col<G64,V1,C4>") == "attn_csr_bwd_col<f32,G64,V1,C4>" and bb.fp32_tag("attn_csr_bf16_bwd_row<G8,V8,C1>") is None
    # the lane group the restatement follows is the host's choice
    for d, dv in bb.WIDTHS:
        for aligned in (True, False):
            vec = 8 if aligned and d % 8 == 0 and dv % 8 == 0 else 1
            g, c = bb.lanes_of(d, dv, vec)
            assert fref.tag_of(d, dv, aligned) == f"attn_csr_bf16<G{g},V{vec},C{c}>"
    # the other libraries are untouched by the new kernels: no such symbol there
    for path in (capi.LIB_PATH, capi_attn_csr_bf16.LIB_PATH, capi_attn_csr_bwd.LIB_PATH):
        assert "attn_csr_bf16_bwd" not in _symbols(path), path


def test_the_cases_are_what_the_issue_lists_and_their_operands_are_bf16_with_exact_scores():
    assert len(bb.CASES) == 3 * 9 * 3 * 2 and len({c.id for c in bb.CASES}) == len(bb.CASES)
    assert bb.PATTERNS == ("edges", "edgesT", "ragged") and bb.WIDTHS == fref.WIDTHS
    # the rows of `edges` (the row pass) and the columns of `edgesT` (the column pass) have these many entries
    want = {0, 1, 7, 8, 9, 255, 256, 257, 300, 1025}
    assert want <= set(np.diff(bb.matrix("edges").row_ptrs.astype(np.int64)).tolist())
    t = bb.matrix("edgesT")
    assert want <= set(np.bincount(t.col_idxs.astype(np.int64), minlength=t.num_cols).tolist())
    for case in bb.CASES:
        op, csr = bb.operands(case), bb.matrix(case.name)
        for n in ("q", "k", "v", "g"):
            assert fref.is_bf16(op[n]), (case.id, n)
            assert np.array_equal(fref.widen(fref.to_bits(op[n])), op[n])
        assert tight.exact_scores(csr, op["q"], op["k"], op["scale"], op["bias"]), case.id
        assert op["q"].shape == (case.heads, csr.num_rows, case.d) and op["g"].shape == (case.heads, csr.num_rows, case.dv)
        assert op["k"].shape == (1, csr.num_cols, case.d) and op["v"].shape == (1, csr.num_cols, case.dv)
        for n in ("v", "g"):
            assert np.unique(np.abs(op[n])).size > 100 or op[n].size < 2000, (case.id, n)       # more than a grid's values
        if case.bias == "finite" and case.heads > 1:
            assert op["bias"].shape == (case.heads, csr.nnz)
        if case.bias == "masked":
            assert np.isneginf(op["bias"]).any() and op["bias"].ndim == 1
        g1 = bb.one_hot_g(case)
        assert fref.is_bf16(g1) and np.all((g1 != 0).sum(axis=2) == 1)


def test_the_lane_dot_is_the_chain_and_the_tree_of_the_header():
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((3, 40)).astype(np.float32), rng.standard_normal((3, 40)).astype(np.float32)
    from _softmax_bsr_ref import fma32
    # V8, G8: lane l sums columns 8 l .. 8 l + 7 ascending from +0; lanes 5 .. 7 hold nothing
    lanes = []
    for lane in range(8):
        acc = np.zeros(3, np.float32)
        for c in range(8 * lane, min(8 * lane + 8, 40)):
            acc = fma32(x[:, c], y[:, c], acc).astype(np.float32)
        lanes.append(acc)
    f = np.float32
    want = (((lanes[0] + lanes[1]).astype(f) + (lanes[2] + lanes[3]).astype(f)).astype(f) + ((lanes[4] + lanes[5]).astype(f) + (lanes[6] + lanes[7]).astype(f)).astype(f)).astype(f)
    assert np.array_equal(bb.lane_dot(x, y, 8, 8, 1), want)
    # V1, G64: one column a lane, a plain pairwise tree
    acc = np.zeros((3, 64), np.float32)
    acc[:, :40] = x * y
    while acc.shape[1] > 1:
        acc = (acc[:, 0::2] + acc[:, 1::2]).astype(f)
    assert np.array_equal(bb.lane_dot(x, y, 64, 1, 1), acc[:, 0])
    assert bb.lanes_of(100, 36, 1) == (64, 2) and bb.lanes_of(1, 129, 1) == (64, 4) and bb.lanes_of(256, 256, 8) == (32, 1)


@pytest.mark.parametrize("case", bb.CASES, ids=lambda c: c.id)
def test_the_restatement_lies_inside_the_tolerances_and_the_tight_check(case):
    got = bb.restated(case)
    assert bb.coverage(case, got["out"], got["lse"]) == 1.0
    results = {what: check(got, case) for what, check in bb.CHECKS.items()}
    print(f"restated {case.id} (V{bb.vec_of(case)}): worst |err| / tolerance (dq, dk, dv): "
          + "; ".join(f"{what} " + ", ".join(f"{w:.3g}" for w in worst) for what, (_, worst) in results.items()))
    for what, (ok, worst) in results.items():
        assert ok and max(worst) <= 1.0, (what, worst)
    if bb.vec_of(case) == 8 and case.heads == 1:        # the same operands on element lanes (an odd stride): the same bounds
        got = bb.restated(case, None, 1)
        for what, check in bb.CHECKS.items():
            assert check(got, case)[0], (what, "V1")


# a fault and cases on which it must be noticed: even widths for the pair swaps, more than one head for the stride (grad_out is
# a view of [M, H, Dv + 8] storage: ldg = H (Dv + 8) against ldv = Dv + 8)
FAULT_CASES = {
    "q_pair_swapped": (bb.Case("edges", 8, 64, "none", 1), bb.Case("ragged", 40, 72, "finite", 3)),
    "g_pair_swapped": (bb.Case("edgesT", 8, 64, "none", 1), bb.Case("ragged", 100, 36, "masked", 1)),
    "g_at_v_stride": (bb.Case("edges", 40, 72, "none", 3), bb.Case("ragged", 64, 8, "masked", 3)),
    "grads_truncated": (bb.Case("edges", 3, 5, "none", 1), bb.Case("ragged", 128, 128, "finite", 3)),
    "out_read_as_bf16": (bb.Case("edgesT", 8, 64, "none", 1), bb.Case("ragged", 3, 5, "finite", 3)),
}
FP32_FAULT_CASES = {f: (bb.Case("edges", 8, 64, "finite", 3),) for f in bb.FP32_FAULTS}


def _caught(case, fault):
    got = bb.restated(case, fault)
    return [what for what, check in bb.CHECKS.items() if not check(got, case)[0]]


@pytest.mark.parametrize("fault", sorted(bb.FAULTS))
def test_the_checks_notice_every_bf16_specific_fault(fault):
    assert set(FAULT_CASES) == set(bb.FAULTS)
    for case in FAULT_CASES[fault]:
        assert case in bb.CASES
        if fault == "g_at_v_stride":
            assert case.heads * (case.dv + bb.PAD) != case.dv + bb.PAD, "the case must have ldg != ldv"
        caught = _caught(case, fault)
        print(f"{fault} on {case.id}: rejected by {caught}")
        assert caught, f"{fault} ({bb.FAULTS[fault]}) passes every check on {case.id}"
        assert not _caught(case, None), "the honest restatement of the same case passes them all"
        # truncation is no rounding to nearest even: the rounding check catches it, the checks of the fp32 gradients cannot (they
        # are honest), and the bf16 bound may (a truncation is off by up to a whole unit, 2^-7, where the bound allows half)
        if fault == "grads_truncated":
            assert "rounded_once" in caught and not {"bwd_tolerances", "tight_backward"} & set(caught)


@pytest.mark.parametrize("fault", sorted(bb.FP32_FAULTS))
def test_the_checks_notice_the_fp32_backwards_faults_too(fault):
    for case in FP32_FAULT_CASES[fault]:
        assert case in bb.CASES
        caught = _caught(case, fault)
        print(f"{fault} on {case.id}: rejected by {caught}")
        assert "bwd_tolerances" in caught or "tight_backward" in caught, f"{fault} passes the numerical checks on {case.id}"


@pytest.mark.parametrize("variant", sorted(bb.HONEST))
def test_honest_variants_pass(variant):
    for case in (bb.Case("edges", 8, 64, "finite", 3), bb.Case("edgesT", 100, 36, "masked", 1), bb.Case("ragged", 128, 128, "none", 1)):
        assert not _caught(case, variant), (variant, case.id)


def test_python_layer_refuses_every_defect_on_cpu_tensors_and_cpu_tensors_as_such():
    torch = pytest.importorskip("torch")
    from mispmm import autograd, ops
    from mispmm.attn_csr_bf16 import attention_csr_bf16_bwd
    csr = matrix("long")
    t_csr, perm_np = bb.bref.transpose(csr)
    a = ops.DeviceCSR.from_host(csr, device="cpu")
    at = ops.DeviceCSR.from_host(t_csr, device="cpu")
    perm = torch.from_numpy(perm_np.astype(np.int32))
    m, kk, nnz = csr.num_rows, csr.num_cols, csr.nnz
    bits = lambda *shape: torch.zeros(shape, dtype=torch.int16)            # noqa: E731
    good = dict(q=bits(m, 8), k=bits(kk, 8), v=bits(kk, 16), out=torch.zeros((m, 16)), lse=torch.zeros(m), grad_out=bits(m, 16))

    def refused(match, at_=at, perm_=perm, **kw):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            attention_csr_bf16_bwd(a, at_, perm_, *(args.pop(n) for n in ("q", "k", "v", "out", "lse", "grad_out")), **args)

    # wrong dtype
    refused("q must be an int16 tensor of bf16 bits", q=torch.zeros((m, 8)))
    refused("k must be an int16 tensor of bf16 bits", k=torch.zeros((kk, 8), dtype=torch.bfloat16))
    refused("v must be an int16 tensor of bf16 bits", v=torch.zeros((kk, 16), dtype=torch.int32))
    refused("grad_out must be an int16 tensor of bf16 bits", grad_out=torch.zeros((m, 16)))
    refused("out must be a float32 tensor", out=bits(m, 16))
    refused("bias must be a float32", bias=torch.zeros(nnz, dtype=torch.float64))
    refused("lse must be a contiguous float32", lse=torch.zeros(m, dtype=torch.float64))
    refused("delta must be a contiguous float32", delta=torch.zeros(m, dtype=torch.float64))
    refused("perm must hold", perm_=torch.zeros(nnz))
    # a dq= / dk= / dv= of the wrong dtype for grads_bf16
    refused("dq must be an int16 tensor of bf16 bits", dq=torch.zeros((m, 8)))
    refused("dk must be an int16 tensor of bf16 bits", dk=torch.zeros((kk, 8)), grads_bf16=True)
    refused("dv must be a float32 tensor", dv=bits(kk, 16), grads_bf16=False)
    # wrong rank
    refused("q must be", q=bits(m * 8))
    refused("must all be 2-D or all", k=bits(1, kk, 8))
    refused("must all be 2-D or all", grad_out=bits(1, m, 16))
    refused("v must be", v=bits(1, 1, kk, 16))
    # wrong shape
    refused("q must be", q=bits(m + 1, 8))
    refused("k must be", k=bits(kk - 1, 8))
    refused("same number of columns", k=bits(kk, 16))
    refused("widths from 1 to 256: v", v=bits(kk, 264))
    refused("out must have shape", out=torch.zeros((m, 8)))
    refused("grad_out must have shape", grad_out=bits(m + 1, 16))
    refused("dq must have shape", dq=bits(m, 16))
    refused("dv must have shape", dv=bits(m, 16))
    refused("bias must have shape", bias=torch.zeros(nnz + 1))
    refused("lse must be a contiguous float32", lse=torch.zeros(m + 1))
    refused("delta must be a contiguous float32", delta=torch.zeros(m + 1))
    refused("perm must hold", perm_=perm[:-1])
    refused("A\\^T", at_=a)
    refused("three flags", need=(True, True))
    # column stride != 1
    refused("q must have unit column stride", q=bits(m, 16)[:, ::2])
    refused("grad_out must have unit column stride", grad_out=bits(m, 32)[:, ::2])
    refused("out must have unit column stride", out=torch.zeros((m, 32))[:, ::2])
    refused("dk must have unit column stride", dk=bits(kk, 16)[:, ::2])
    refused("bias must have unit stride", bias=torch.zeros(2 * nnz)[::2])
    # rows that overlap
    refused("k must not overlap its own rows", k=bits(1, 8).expand(kk, 8))
    refused("grad_out must not overlap its own rows", grad_out=bits(1, 16).expand(m, 16))
    refused("dv must not overlap its own rows", dv=bits(1, 16).expand(kk, 16))
    # negative strides cannot be made by torch views; the check stands for tensors that come from elsewhere
    class Reversed:
        dtype, shape, is_cuda = torch.int16, (m, 16), False

        def dim(self):
            return 2

        def unsqueeze(self, _):
            return Reversed3()

    class Reversed3(Reversed):
        shape = (1, m, 16)

        def dim(self):
            return 3

        def stride(self, i=None):
            s = (0, -16, 1)
            return s if i is None else s[i]
    refused("grad_out must not have a negative stride", grad_out=Reversed())
    # a non-contiguous lse or delta
    refused("lse must be a contiguous float32", lse=torch.zeros((m, 2))[:, 0])
    refused("delta must be a contiguous float32", delta=torch.zeros((m, 2))[:, 0])
    # a missing perm with a bias where dk or dv is needed -- and not where dq alone is
    refused("with a bias, dk and dv need perm", perm_=None, bias=torch.zeros(nnz))
    refused("no CPU path", perm_=None, bias=torch.zeros(nnz), need=(True, False, False))
    # a float64 matrix
    with pytest.raises(ValueError, match="float32 DeviceCSR"):
        attention_csr_bf16_bwd(ops.DeviceCSR.from_host(csr, device="cpu", dtype=torch.float64), at, perm, *good.values())
    # CPU tensors as such: well-formed operands
    refused("no CPU path")
    refused("no CPU path", bias=torch.zeros(nnz), dq=bits(m, 8), dk=bits(kk, 8), dv=bits(kk, 16), delta=torch.zeros(m))
    refused("no CPU path", grads_bf16=False, dq=torch.zeros((m, 8)), need=(True, False, False))
    refused("no CPU path", q=bits(2, m, 8), k=bits(1, kk, 8).expand(2, kk, 8), v=bits(2, kk, 16), out=torch.zeros((2, m, 16)), lse=torch.zeros((2, m)),
            grad_out=bits(2, m, 16), bias=torch.zeros((2, nnz)))
    # the keyword of autograd: refused with a float32 out at the call, naming the reason, before anything else is looked at
    t = autograd.TrainableCSR.from_host(csr, device="cpu")
    qb, kb, vb = (good[n].view(torch.bfloat16) for n in ("q", "k", "v"))
    with pytest.raises(ValueError, match="grad_out would be float32"):
        autograd.sparse_attention_bf16(t, qb, kb, vb, fused_backward=True, out_dtype=torch.float32)
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.sparse_attention_bf16(t, qb, kb, vb, fused_backward=True)
