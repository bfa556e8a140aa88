"""The bias gradient of the fused CSR attention on a machine WITHOUT a GPU: the tenth library and its binding, the entry points'
argument validation (which precedes any device work), the census of the kernel's instances and tags, the float64 reference
against torch autograd, the kernel as built restated in numpy (tests/_attn_csr_dbias_ref.py) inside the derived tolerance on
every case the GPU suite runs, the floor under P that lets the GPU suite's exact check leave no row out, the faults the checks
must notice, and the refusals of the Python layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_attn_csr_bf16_bwd, capi_attn_csr_bwd, capi_attn_csr_dbias

import _attn_csr_bwd_ref as bref
import _attn_csr_dbias_ref as db
import _attn_csr_ref as ref
from _sddmm_ref import entry_rows
from _softmax_ref import matrix
from test_census_cpu import _symbol_tool

NAMES = {"mispmm_attn_csr_dbias_f32": "attn_csr_dbias_f32", "mispmm_attn_csr_dbias_bf16": "attn_csr_dbias_bf16"}
INSTANCES = {"f32": 10, "bf16": 9}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_has_its_two_exports_and_header_and_binding_agree():
    assert os.path.exists(capi_attn_csr_dbias.LIB_PATH), f"{capi_attn_csr_dbias.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn_csr_dbias.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_attn_csr_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_attn_csr_dbias.SIGNATURES) == set(NAMES)
    kinds = {"mispmm_stream_t": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    order = {}
    for name in NAMES:
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert want == capi_attn_csr_dbias.SIGNATURES[name][1] and len(want) == 30, name
        order[name] = [p.split()[-1].lstrip("*") for p in params]
        pointee = {p.split()[-1].lstrip("*"): p.replace("*", " ").split()[-2] for p in params if "*" in p}
        elem = "float" if name.endswith("_f32") else "uint16_t"
        assert [pointee[n] for n in ("Q", "Kmat", "V", "grad_out")] == [elem] * 4 and [pointee[n] for n in ("out", "lse", "bias", "dBias")] == ["float"] * 4
    assert order["mispmm_attn_csr_dbias_f32"] == order["mispmm_attn_csr_dbias_bf16"], "one argument order for both element types"
    tool = _symbol_tool()
    if tool is not None:
        dyn = subprocess.run([tool, "-D", "--defined-only", capi_attn_csr_dbias.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in dyn.splitlines() if " T " in line and "mispmm_" in line}
        assert exported == set(NAMES), exported
    lib = capi_attn_csr_dbias.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes == capi_attn_csr_dbias.SIGNATURES[name][1]
    assert capi_attn_csr_dbias.last_kernel() == lib.mispmm_last_kernel().decode()
    for header in ("mispmm.h", "mispmm_attn_csr.h", "mispmm_attn_csr_bwd.h", "mispmm_attn_csr_bf16.h", "mispmm_attn_csr_bf16_bwd.h"):
        with open(os.path.join(ROOT, "include", header), encoding="utf-8") as f:
            assert "mispmm_attn_csr_dbias" not in f.read()
    for other in (capi, capi_attn_csr_bwd, capi_attn_csr_bf16_bwd):
        assert not set(NAMES) & set(other.SIGNATURES)


ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced
FAR = 1 << 40                              # fake pointers far apart: no two operands overlap


def _call(name, **kw):
    """Every call made through here is refused or a no-op: the pointers are fake."""
    far = lambda i: FAR * (i + 1)                                        # noqa: E731
    a = dict(stream=None, H=2, M=4, K=64, nnz=8, ptrs=ONE, cols=ONE + 4096, q=far(0), qh=4096, ldq=64, k=far(1), kh=4096, ldk=64, D=64, v=far(2),
             vh=4096, ldv=64, Dv=64, scale=0.125, bias=None, bh=0, out=far(3), oh=4096, ldo=64, lse=far(4), g=far(5), gh=4096, ldg=64, dbias=far(6),
             dbh=8)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return getattr(capi_attn_csr_dbias.lib(), name)(*a.values())


@pytest.mark.parametrize("name", sorted(NAMES))
def test_every_kind_of_bad_argument_is_refused_with_its_message_before_any_device_work(name):
    err, short = capi_attn_csr_dbias.last_error, NAMES[name]
    eb = 4 if name.endswith("_f32") else 2
    call = lambda **kw: _call(name, **kw)                                # noqa: E731
    for kw in (dict(D=257, ldq=257, ldk=257), dict(Dv=257, ldv=257, ldo=257, ldg=257), dict(D=0), dict(Dv=0)):
        assert call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert err().startswith(short + ":") and "from 1 to 256" in err()
    for scale in (float("nan"), float("inf"), -float("inf")):
        assert call(scale=scale) == capi.ERR_INVALID_ARG
        assert short + ": scale must be finite" in err()
    for arg in ("ptrs", "cols", "q", "k", "v"):
        assert call(**{arg: None}) == capi.ERR_INVALID_ARG, arg
        assert err() == short + ": rowPtrs, colIdxs, Q, K or V is null"
    for arg in ("out", "lse", "g", "dbias"):
        assert call(**{arg: None}) == capi.ERR_INVALID_ARG, arg
        assert err() == short + ": out, lse, grad_out or dBias is null"
    for kw in (dict(ldq=56), dict(ldk=56), dict(ldv=56), dict(ldo=56), dict(ldg=56)):
        assert call(**kw) == capi.ERR_INVALID_ARG, kw
        assert short + ": leading dimension smaller than the width" in err()
    assert call(dbh=7) == capi.ERR_INVALID_ARG and "dbias_head_stride 7 is smaller than nnz 8" in err()
    assert call(dbh=0) == capi.ERR_INVALID_ARG and "dBias is per head" in err()
    # one head: the stride is not read.  The next check to fail is made to be the overlap: the message shows the call got there
    assert call(H=1, dbh=0, dbias=FAR) == capi.ERR_INVALID_ARG and err() == short + ": dBias overlaps an input"
    # one head of an operand spanning 2 GiB or more IN BYTES of its own element type, as the backward of that type counts
    rows = (1 << 31) // (64 * eb)                                         # rows of 64 elements that reach 2^31 bytes
    small = dict(ldq=8, D=8, ldk=8)
    for kw, who in ((dict(K=rows, ldk=64), 1), (dict(K=rows, ldv=64, **small), 2), (dict(M=rows, ldq=64, ldo=1, ldg=1, Dv=1, ldv=1), 0),
                    (dict(M=rows, ldg=64, ldo=64, **small), 3), (dict(M=1 << 23, ldo=64, **small), 3),
                    (dict(nnz=1 << 29, bias=FAR * 20, dbh=1 << 29), 5)):
        assert call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert short + ": Q, K, V, out, grad_out or bias of one head spans 2 GiB or more" in err()
        spans = [int(s) for s in re.search(r"\(([\d, ]+) bytes\)", err()).group(1).split(",")]
        assert len(spans) == 6 and spans[who] > 0x7FFFFFFF, (kw, spans)
    # ... and just under it the size check lets the shape through: refused for the overlap, which comes after
    for kw in (dict(K=rows - 1, ldk=64), dict(M=(1 << 23) - 1, ldo=64, **small), dict(nnz=(1 << 29) - 1, bias=FAR * 20, dbh=1 << 29)):
        assert call(dbias=FAR, **kw) == capi.ERR_INVALID_ARG, kw
        assert err() == short + ": dBias overlaps an input"
    assert call(M=(1 << 25) + 1, H=1 << 12, ldq=1, ldo=1, ldg=1, D=1, Dv=1, ldk=1, ldv=1) == capi.ERR_UNSUPPORTED and short in err() and "workgroups" in err()
    if eb == 2:
        for kw in (dict(q=FAR + 1), dict(k=2 * FAR + 1), dict(v=3 * FAR + 1), dict(g=6 * FAR + 1)):
            assert call(**kw) == capi.ERR_INVALID_ARG, kw
            assert err() == short + ": Q, K, V and grad_out must be 2-byte aligned"
    # overlaps, on extents in BYTES of each operand's own type: H = 2 heads of Q (4 rows of 64 at head stride 4096) end
    # (4096 + 3 * 64 + 64) * eb bytes past the base; dBias covers (8 + 8) * 4 bytes
    end = (4096 + 3 * 64 + 64) * eb
    for kw in (dict(dbias=FAR), dict(dbias=FAR + end - 4), dict(dbias=FAR - 64 + 4), dict(dbias=4 * FAR + (4096 + 256) * 4 - 4), dict(dbias=5 * FAR + 2 * 4 * 4 - 4),
               dict(dbias=6 * FAR + end - 4), dict(dbias=ONE + 4 * 4), dict(dbias=ONE + 4096 + 7 * 4), dict(bias=FAR * 20, dbias=FAR * 20 + 28),
               dict(bias=FAR * 20, bh=100, dbias=FAR * 20 + 107 * 4)):
        assert call(**kw) == capi.ERR_INVALID_ARG, kw
        assert err() == short + ": dBias overlaps an input"
    # (a dBias right behind an input is not refused: with fake pointers that cannot be shown here, a launch would follow; the
    # GPU test's guard words lie right behind and before real operands)


def test_no_ops_return_before_any_pointer_is_looked_at():
    nothing = dict(ptrs=None, cols=None, q=None, k=None, v=None, out=None, lse=None, g=None, dbias=None)
    for name in NAMES:
        assert _call(name, H=0, **nothing) == capi.OK
        assert _call(name, M=0, **nothing) == capi.OK
        assert _call(name, nnz=0, **nothing) == capi.OK
        assert _call(name, H=0, scale=float("nan")) == capi.ERR_INVALID_ARG          # ... but after the checks that need none
        assert _call(name, nnz=0, D=300, ldq=300, ldk=300) == capi.ERR_UNSUPPORTED


def _symbols(path):
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    return subprocess.run([tool, "-C", path], capture_output=True, text=True, check=True).stdout


def test_the_library_holds_its_nineteen_instances_and_the_tag_table_lists_each():
    out = _symbols(capi_attn_csr_dbias.LIB_PATH)
    stubs = re.findall(r"__device_stub__([A-Za-z0-9_]+)", out)
    assert set(stubs) == {"attn_csr_dbias_kernel"} and len(stubs) == sum(INSTANCES.values()) == 19, stubs
    tags, per_elem = set(), {"f32": 0, "bf16": 0}
    for args in set(re.findall(r"__device_stub__attn_csr_dbias_kernel<([^>]*)>", out)):
        elem, *consts = (s.strip() for s in args.split(","))              # the element policy, then G, VEC, NCH
        kind = {"ElemF32": "f32", "ElemBf16": "bf16"}[elem.split("::")[-1]]
        g, vec, nch = (int(s) for s in consts)
        tags.add(f"attn_csr_dbias<{kind},G{g},V{vec},C{nch}>")
        per_elem[kind] += 1
    assert per_elem == INSTANCES
    assert tags == set(db.TAGS), (sorted(tags - set(db.TAGS)), sorted(set(db.TAGS) - tags))
    for tag, (elem, (d, dv, aligned)) in db.TAGS.items():
        assert db.tag_of(elem, d, dv, aligned) == tag
        # the same (G, V, C) as the backward's row pass on the same operands
        row = bref.tags_of(d, dv, aligned, (True, False, False))[0] if elem == "f32" else None
        if row is not None:
            assert row.split("<f32,")[1] == tag.split("<f32,")[1]
    # the widths of the cases reach every lane width and chunk count the aligned layout can
    reached = {db.tag_of(e, d, dv, True) for e in db.ELEMS for d, dv in ref.WIDTHS}
    assert {t.split(",", 1)[1] for t in reached} >= {"G8,V1,C1>", "G64,V4,C1>", "G32,V8,C1>", "G16,V4,C1>"}
    # the other libraries are untouched by the new kernel: no such symbol there
    for path in (capi.LIB_PATH, capi_attn_csr_bwd.LIB_PATH, capi_attn_csr_bf16_bwd.LIB_PATH):
        assert "attn_csr_dbias" not in _symbols(path), path


def test_the_cases_are_what_the_issue_lists():
    assert len(db.CASES) == 2 * 7 * 3 * 2 and len({c.id for c in db.CASES}) == len(db.CASES) and set(db.CASES) <= set(bref.CASES)
    assert {c.name for c in db.CASES} == {"edges", "ragged"}
    assert {(c.d, c.dv) for c in db.CASES} == {(8, 64), (64, 8), (40, 72), (3, 5), (1, 1), (128, 128), (256, 256)}
    assert {c.bias for c in db.CASES} == {"none", "finite", "masked"} and {c.heads for c in db.CASES} == {1, 3}
    lens = np.diff(db.matrix("edges").row_ptrs.astype(np.int64))
    assert {0, 1, 7, 8, 9, 255, 256, 257, 300, 1025} <= set(lens.tolist()) and lens.size == 32
    import _attn_csr_bf16_ref as fref
    for case in db.CASES:
        op, raw = db.operands(case, "bf16"), db.operands(case)
        for n in ("q", "k", "v", "g"):
            assert fref.is_bf16(op[n]) and np.all(np.abs(op[n] - raw[n]) <= 2.0 ** -8 * np.abs(raw[n])), (case.id, n)
        assert np.array_equal(op["q"], raw["q"]) and np.array_equal(op["k"], raw["k"]), "q and k are bf16 values already"


@pytest.mark.parametrize("case", [c for c in db.CASES if c.d <= 40 and c.name == "edges"], ids=lambda c: c.id)
def test_the_float64_reference_is_torch_autograd_of_the_bias_through_dense_masked_attention(case):
    torch = pytest.importorskip("torch")
    op, csr = db.operands(case), db.matrix(case.name)
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    assert len(set(zip(rows.tolist(), cols.tolist()))) == csr.nnz, "a dense matrix holds a pair once"
    want = db.dbias_f64(csr, op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"])
    nonempty = torch.from_numpy(np.flatnonzero(np.diff(csr.row_ptrs.astype(np.int64)) > 0))
    r, c = torch.from_numpy(rows), torch.from_numpy(cols)
    for h in range(case.heads):
        q, k, v, g = (torch.from_numpy(ref._head(op[n], h).astype(np.float64)) for n in ("q", "k", "v", "g"))
        bias = torch.from_numpy(ref._bias_of(op["bias"], h, csr.nnz).astype(np.float64)).requires_grad_(True)
        s = (q * op["scale"]) @ k.T
        z = torch.full((csr.num_rows, csr.num_cols), -float("inf"), dtype=torch.float64).index_put((r, c), s[r, c] + bias)
        out = torch.softmax(z[nonempty], dim=1) @ v
        (out * g[nonempty]).sum().backward()
        got = bias.grad.numpy()
        assert np.all(np.abs(got - want[h]) <= 1e-11 * (1.0 + np.abs(want[h]))), (case.id, h, float(np.abs(got - want[h]).max()))


@pytest.mark.parametrize("elem", db.ELEMS)
@pytest.mark.parametrize("case", db.CASES, ids=lambda c: c.id)
def test_the_restatement_lies_inside_the_tolerance_and_p_has_a_floor(case, elem):
    got = db.restated(case, elem, with_p=True)
    csr = db.matrix(case.name)
    results = {what: check(got, case, elem) for what, check in db.CHECKS.items()}
    print(f"restated {elem} {case.id}: " + ", ".join(f"{what} {w:.3g}" for what, (_, w) in results.items()))
    for what, (ok, worst) in results.items():
        assert ok, (what, worst)
    # every row with entries has a finite lse: the exact check of the GPU suite leaves no row out on that account ...
    lens = np.diff(csr.row_ptrs.astype(np.int64))
    assert np.isfinite(got["lse"][:, lens > 0]).all()
    # ... and none on account of small numbers: every live P is exactly 0 (a masked entry) or at least 2^-60, and no
    # scale * dBias is subnormal, so fl(dBias * scale) is exact and v_exp_f32 flushes nothing
    p = got["p"]
    assert np.all((p == 0) | (p >= 2.0 ** -60)), float(p[p > 0].min())
    ds = np.abs(got["dbias"].astype(np.float64) * db.operands(case, elem)["scale"])
    assert np.all((ds == 0) | (ds >= 2.0 ** -126))
    masked = np.zeros_like(p, dtype=bool) if case.bias != "masked" else np.isneginf(np.broadcast_to(db.operands(case, elem)["bias"], p.shape))
    assert np.array_equal(p == 0, masked), "P is zero on the masked entries and nowhere else"


# a fault and cases on which it must be noticed
_H3 = (db.Case("edges", 8, 64, "finite", 3), db.Case("ragged", 40, 72, "finite", 3))
_ANY = (db.Case("edges", 8, 64, "finite", 3), db.Case("edges", 3, 5, "masked", 1), db.Case("ragged", 128, 128, "none", 1))
FAULT_CASES = {"scale_multiplied_in": _ANY, "delta_omitted": _ANY, "delta_from_the_wrong_row": _ANY, "head0_lse_for_every_head": _H3,
               "head0_bias_for_every_head": _H3, "last_slot_of_full_batch_not_stored": _ANY, "dead_slot_stored": _ANY,
               "stored_at_previous_batch_offset": _ANY}


def _caught(case, elem, fault):
    got = db.restated(case, elem, fault)
    return [what for what, check in db.CHECKS.items() if not check(got, case, elem)[0]]


@pytest.mark.parametrize("elem", db.ELEMS)
@pytest.mark.parametrize("fault", db.FAULTS)
def test_the_checks_notice_every_fault(fault, elem):
    assert set(FAULT_CASES) == set(db.FAULTS)
    for case in FAULT_CASES[fault]:
        assert case in db.CASES
        caught = _caught(case, elem, fault)
        print(f"{fault} on {elem} {case.id}: rejected by {caught}")
        assert caught, f"{fault} passes every check on {case.id}"
        assert not _caught(case, elem, None), "the honest restatement of the same case passes them all"
    if fault == "scale_multiplied_in":          # a scale of 2^-2 is far outside the bound, and dS comes out scaled twice
        assert {"inside_tolerance", "rebuilds_dq"} <= set(_caught(FAULT_CASES[fault][0], elem, fault))
    if fault in ("last_slot_of_full_batch_not_stored", "stored_at_previous_batch_offset"):
        assert "all_written" in _caught(FAULT_CASES[fault][0], elem, fault)


@pytest.mark.parametrize("variant", db.HONEST)
def test_honest_variants_pass_the_tolerance_check(variant):
    for case in (db.Case("edges", 8, 64, "finite", 3), db.Case("edges", 256, 256, "masked", 1), db.Case("ragged", 128, 128, "none", 1)):
        for elem in db.ELEMS:
            got = db.restated(case, elem, variant)
            ok, worst = db.inside_tolerance(got, case, elem)
            assert ok and db.all_written(got, case, elem)[0], (variant, elem, case.id, worst)


def test_a_guard_between_the_heads_keeps_its_sentinel_and_the_checks_read_it():
    case = db.Case("edges", 8, 64, "finite", 3)
    op, csr = db.operands(case), db.matrix("edges")
    out, lse = db.forward_restated(case)
    args = (csr, op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"], out, lse)
    wide = db.dbias_f32(*args, head_stride=csr.nnz + 5)
    assert db.all_written(dict(dbias=wide), case)[0] and np.array_equal(wide[:, :csr.nnz].view(np.uint32), db.dbias_f32(*args).view(np.uint32))
    assert not db.all_written(dict(dbias=db.dbias_f32(*args, head_stride=csr.nnz + 5, fault="dead_slot_stored")), case)[0], "the last row's dead slots land in the guard"


def test_python_layer_refuses_every_defect_on_cpu_tensors_and_cpu_tensors_as_such():
    torch = pytest.importorskip("torch")
    from mispmm import autograd, ops
    from mispmm.attn_csr_dbias import attention_csr_dbias, attention_csr_dbias_bf16
    csr = matrix("long")
    a = ops.DeviceCSR.from_host(csr, device="cpu")
    m, kk, nnz = csr.num_rows, csr.num_cols, csr.nnz
    for fn, dtype, words in ((attention_csr_dbias, torch.float32, "a float32 tensor"), (attention_csr_dbias_bf16, torch.int16, "an int16 tensor of bf16 bits")):
        other = torch.int16 if dtype == torch.float32 else torch.float32
        t = lambda *shape: torch.zeros(shape, dtype=dtype)                  # noqa: E731
        good = dict(q=t(m, 8), k=t(kk, 8), v=t(kk, 16), out=torch.zeros((m, 16)), lse=torch.zeros(m), grad_out=t(m, 16))

        def refused(match, **kw):
            args = dict(good)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                fn(a, *(args.pop(n) for n in ("q", "k", "v", "out", "lse", "grad_out")), **args)

        # wrong dtype
        refused(f"q must be {words}", q=torch.zeros((m, 8), dtype=other))
        refused(f"k must be {words}", k=torch.zeros((kk, 8), dtype=torch.bfloat16))
        refused(f"v must be {words}", v=torch.zeros((kk, 16), dtype=torch.float64))
        refused(f"grad_out must be {words}", grad_out=torch.zeros((m, 16), dtype=other))
        refused("out must be a float32 tensor", out=torch.zeros((m, 16), dtype=torch.int16))
        refused("bias must be a float32", bias=torch.zeros(nnz, dtype=torch.float64))
        refused("lse must be a contiguous float32", lse=torch.zeros(m, dtype=torch.float64))
        refused("dbias must be a float32 tensor", dbias=torch.zeros(nnz, dtype=torch.float64))
        # wrong rank and shape
        refused("q must be", q=t(m * 8))
        refused("must all be 2-D or all", k=t(1, kk, 8))
        refused("must all be 2-D or all", grad_out=t(1, m, 16))
        refused("q must be", q=t(m + 1, 8))
        refused("k must be", k=t(kk - 1, 8))
        refused("same number of columns", k=t(kk, 16))
        refused("widths from 1 to 256: v", v=t(kk, 264))
        refused("out must have shape", out=torch.zeros((m, 8)))
        refused("grad_out must have shape", grad_out=t(m + 1, 16))
        refused("bias must have shape", bias=torch.zeros(nnz + 1))
        refused("lse must be a contiguous float32", lse=torch.zeros(m + 1))
        refused("dbias must have shape", dbias=torch.zeros(nnz + 1))
        refused("dbias must have shape", dbias=torch.zeros((1, nnz)))
        # strides
        refused("q must have unit column stride", q=t(m, 16)[:, ::2])
        refused("grad_out must have unit column stride", grad_out=t(m, 32)[:, ::2])
        refused("out must have unit column stride", out=torch.zeros((m, 32))[:, ::2])
        refused("bias must have unit stride", bias=torch.zeros(2 * nnz)[::2])
        refused("dbias must have unit stride", dbias=torch.zeros(2 * nnz)[::2])
        refused("k must not overlap its own rows", k=t(1, 8).expand(kk, 8))
        refused("grad_out must not overlap its own rows", grad_out=t(1, 16).expand(m, 16))
        refused("lse must be a contiguous float32", lse=torch.zeros((m, 2))[:, 0])
        heads3 = dict(q=t(2, m, 8), k=t(1, kk, 8).expand(2, kk, 8), v=t(2, kk, 16), out=torch.zeros((2, m, 16)), lse=torch.zeros((2, m)), grad_out=t(2, m, 16))
        refused("dbias must not overlap its own heads", dbias=torch.zeros((1, nnz)).expand(2, nnz), **heads3)
        # a float64 matrix
        with pytest.raises(ValueError, match="float32 DeviceCSR"):
            fn(ops.DeviceCSR.from_host(csr, device="cpu", dtype=torch.float64), *good.values())
        # CPU tensors as such: well-formed operands
        refused("no CPU path")
        refused("no CPU path", bias=torch.zeros(nnz), dbias=torch.zeros(nnz), scale=0.5)
        refused("no CPU path", bias=torch.zeros((2, nnz)), dbias=torch.zeros((2, nnz + 3))[:, :nnz], **heads3)
    # autograd takes the keyword on every path (the device check comes first there, as it always did: the refusal of a bias that
    # requires a gradient without the keyword is held on the GPU)
    tr = autograd.TrainableCSR.from_host(csr, device="cpu")
    q, k, v = torch.zeros((m, 8)), torch.zeros((kk, 8)), torch.zeros((kk, 16))
    bias = torch.zeros(nnz, requires_grad=True)
    for kw in (dict(), dict(fused=True), dict(fused=True, fused_backward=True)):
        with pytest.raises(ValueError, match="no CPU path"):
            autograd.sparse_attention(tr, q, k, v, bias=bias, bias_grad=True, **kw)
    qb, kb, vb = (x.to(torch.bfloat16) for x in (q, k, v))
    for kw in (dict(), dict(fused_backward=True)):
        with pytest.raises(ValueError, match="no CPU path"):
            autograd.sparse_attention_bf16(tr, qb, kb, vb, bias=bias, bias_grad=True, **kw)
