"""The fused CSR attention backward on a machine WITHOUT a GPU: the sixth library and its binding, the entry point's argument
validation (which precedes any device work), the census of both kernels' instances and tags, and both passes as built,
restated in numpy float32 (tests/_attn_csr_bwd_ref.py::backward_f32) on the restated forward's out and lse, inside the derived
tolerances and the derived tight check on every case the GPU suite runs."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_attn_csr, capi_attn_csr_bwd

import _attn_csr_bwd_mutants as mut
import _attn_csr_bwd_ref as bref
import _attn_csr_bwd_tight as btight
import _attn_csr_ref as ref
from _softmax_ref import matrix
from test_census_cpu import _symbol_tool

INSTANCES = {"attn_csr_bwd_row_kernel": 10, "attn_csr_bwd_col_kernel": 10}     # __device_stub__ symbols per kernel template
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mispmm_attn_csr_bwd_f32"


def test_the_library_has_one_export_and_header_and_binding_agree():
    assert os.path.exists(capi_attn_csr_bwd.LIB_PATH), f"{capi_attn_csr_bwd.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_attn_csr_bwd.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_attn_csr_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_attn_csr_bwd.SIGNATURES) == {NAME}
    params = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    kinds = {"mispmm_stream_t": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
    assert want == capi_attn_csr_bwd.SIGNATURES[NAME][1]
    tool = _symbol_tool()
    if tool is not None:
        dyn = subprocess.run([tool, "-D", "--defined-only", capi_attn_csr_bwd.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in dyn.splitlines() if " T " in line and "mispmm_" in line}
        assert exported == {NAME}, exported
    lib = capi_attn_csr_bwd.lib()
    assert lib.mispmm_attn_csr_bwd_f32.argtypes == capi_attn_csr_bwd.SIGNATURES[NAME][1]
    assert capi_attn_csr_bwd.last_kernel() == lib.mispmm_last_kernel().decode()
    # no existing library, header or binding gained a name
    for header in ("mispmm.h", "mispmm_attn_csr.h"):
        with open(os.path.join(ROOT, "include", header), encoding="utf-8") as f:
            assert "attn_csr_bwd" not in f.read()
    assert not any("attn_csr" in n for n in capi.SIGNATURES) and set(capi_attn_csr.SIGNATURES) == {"mispmm_attn_csr_f32"}
    if tool is not None:
        for path in (capi.LIB_PATH, capi_attn_csr.LIB_PATH):
            assert "attn_csr_bwd" not in subprocess.run([tool, "-C", path], capture_output=True, text=True, check=True).stdout


ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced
FAR = [ONE + (i << 32) for i in range(16)]  # fake pointers far apart: no two operands overlap


def _call(**kw):
    """Every call made through here is refused or a no-op: the pointers are fake."""
    a = dict(stream=None, H=2, M=4, K=64, nnz=8, ptrs=FAR[0], cols=FAR[1], tptrs=FAR[2], tcols=FAR[3], perm=None, q=FAR[4], qh=4096, ldq=64,
             k=FAR[5], kh=4096, ldk=64, D=64, v=FAR[6], vh=4096, ldv=64, Dv=64, scale=0.125, bias=None, bh=0, out=FAR[7], oh=4096, ldo=64,
             lse=FAR[8], g=FAR[9], gh=4096, ldg=64, delta=FAR[10], dq=FAR[11], dqh=4096, lddq=64, dk=FAR[12], dkh=4096, lddk=64, dv=FAR[13],
             dvh=4096, lddv=64)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_attn_csr_bwd.lib().mispmm_attn_csr_bwd_f32(*a.values())


def test_every_kind_of_bad_argument_is_refused_with_its_message_before_any_device_work():
    err = capi_attn_csr_bwd.last_error
    # the forward's list
    for name in ("ptrs", "cols", "q", "k", "v"):
        assert _call(**{name: None}) == capi.ERR_INVALID_ARG, name
        assert "attn_csr_bwd_f32" in err() and "null" in err()
    for kw in (dict(D=257, ldq=257, ldk=257), dict(Dv=257, ldv=257, ldo=257), dict(D=0), dict(Dv=0)):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "from 1 to 256" in err()
    for scale in (float("nan"), float("inf"), -float("inf")):
        assert _call(scale=scale) == capi.ERR_INVALID_ARG
        assert "scale must be finite" in err()
    for kw in (dict(ldq=56), dict(ldk=56), dict(ldv=56), dict(ldo=56), dict(ldg=56), dict(lddq=56), dict(lddk=56), dict(lddv=56)):
        assert _call(**kw) == capi.ERR_INVALID_ARG, kw
        assert "leading dimension smaller than the width" in err()
    for kw in (dict(K=1 << 24, ldk=64), dict(M=1 << 21, ldq=1024), dict(M=1 << 24, ldo=64), dict(M=1 << 24, ldg=64), dict(nnz=1 << 30, bias=FAR[14], perm=FAR[15])):
        assert _call(**kw) == capi.ERR_UNSUPPORTED, kw
        assert "2 GiB" in err()
    assert _call(M=(1 << 25) + 1, H=1 << 12, ldq=1, ldo=1, ldg=1, D=1, Dv=1, ldk=1, ldv=1, lddq=1, lddk=1, lddv=1, qh=0, oh=0, gh=0, dqh=0) \
        == capi.ERR_UNSUPPORTED and "workgroups" in err()
    # the backward's own
    for name in ("out", "lse", "g", "delta"):
        assert _call(**{name: None}) == capi.ERR_INVALID_ARG, name
        assert "out, lse, grad_out or delta is null" in err()
    for name in ("tptrs", "tcols"):
        assert _call(**{name: None}) == capi.ERR_INVALID_ARG and "A^T" in err(), name
        assert _call(**{name: None}, dq=None, dk=None) == capi.ERR_INVALID_ARG and "A^T" in err()      # dV alone needs it too
    assert _call(bias=FAR[14], perm=None) == capi.ERR_INVALID_ARG and "perm" in err()
    for kw in (dict(dq=FAR[4]), dict(dk=FAR[5] + 4096), dict(dv=FAR[9]), dict(delta=FAR[8]), dict(dq=FAR[7] + (4096 + 3 * 64 + 64) * 4 - 16)):       # ... the last 16 bytes of out's second head
        assert _call(**kw) == capi.ERR_INVALID_ARG and "overlaps an input" in err(), kw
    assert _call(dk=FAR[11]) == capi.ERR_INVALID_ARG and "overlap one another" in err()


def test_what_a_skipped_pass_would_need_is_not_asked_for():
    """Each of these goes past every refusal into the launch -- on a machine without a GPU the launch fails, with one the fake
    pointers must not be run -- so only the refusals BEFORE them are held: the same calls with one more thing wrong."""
    err = capi_attn_csr_bwd.last_error
    # dQ alone: no pattern of A^T, no perm
    assert _call(dk=None, dv=None, tptrs=None, tcols=None, bias=FAR[14], ldq=56) == capi.ERR_INVALID_ARG and "leading dimension" in err()
    # dV alone: no delta
    assert _call(dq=None, dk=None, delta=None, ldv=56) == capi.ERR_INVALID_ARG and "leading dimension" in err()
    # a null output's leading dimension is not read
    assert _call(dq=None, lddq=0, ldv=56) == capi.ERR_INVALID_ARG and "lddq=0" in err()


def test_no_ops_return_before_any_pointer_is_looked_at():
    nothing = dict(ptrs=None, cols=None, tptrs=None, tcols=None, q=None, k=None, v=None, out=None, lse=None, g=None, delta=None)
    assert _call(H=0, **nothing) == capi.OK
    assert _call(M=0, **nothing) == capi.OK
    assert _call(dq=None, dk=None, dv=None, **nothing) == capi.OK
    assert _call(H=0, scale=float("nan")) == capi.ERR_INVALID_ARG          # ... but after the checks that need none
    assert _call(M=0, D=300, ldq=300, ldk=300) == capi.ERR_UNSUPPORTED


def test_the_library_holds_the_recorded_instances_and_the_tag_table_lists_each():
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    out = subprocess.run([tool, "-C", capi_attn_csr_bwd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found == INSTANCES, f"kernel template: instances in the library {found}, recorded here {INSTANCES}"
    tags = set()
    for kind, args in set(re.findall(r"__device_stub__attn_csr_bwd_(row|col)_kernel<([^>]*)>", out)):
        elem, *consts = (s.strip() for s in args.split(","))          # the element policy, then G, VEC, NCH
        assert elem.endswith("::ElemF32"), args
        g, vec, nch = (int(s) for s in consts)
        tags.add(f"attn_csr_bwd_{kind}<f32,G{g},V{vec},C{nch}>")
    assert tags == set(bref.TAGS), (sorted(tags - set(bref.TAGS)), sorted(set(bref.TAGS) - tags))
    assert len(bref.TAGS) == sum(INSTANCES.values()) == 20
    for tag, (d, dv, aligned) in bref.TAGS.items():
        kind = tag[len("attn_csr_bwd_"):][:3]
        assert tag in bref.tags_of(d, dv, aligned) and tag.startswith(f"attn_csr_bwd_{kind}<")
        step = 4 if "V4" in tag else 1
        for dd, ddv in ((d - step, dv), (d, dv - step)):         # the smallest shape: one step less lands on another tag
            assert dd == 0 or ddv == 0 or tag not in bref.tags_of(dd, ddv, aligned)
    assert bref.tags_of(256, 256, True) == ["attn_csr_bwd_row<f32,G64,V4,C1>", "attn_csr_bwd_col<f32,G64,V4,C1>"]
    assert bref.tags_of(8, 8, True, (True, False, False)) == ["attn_csr_bwd_row<f32,G8,V4,C1>"]
    assert bref.tags_of(8, 8, True, (False, False, True)) == ["attn_csr_bwd_col<f32,G8,V4,C1>"]
    assert len(bref.tags_of(8, 8, True, (False, True, False))) == 2 and bref.tags_of(8, 8, True, (False, False, False)) == []


def test_the_cases_are_what_the_issue_lists_and_the_column_lengths_cover_the_batch_edges():
    assert len(bref.CASES) == 3 * 7 * 3 * 2 and len({c.id for c in bref.CASES}) == len(bref.CASES)
    edges, edges_t = matrix("edges"), bref.matrix("edgesT")
    # edgesT is the transpose: its columns are edges' rows, so the COLUMN pass on it walks edges' row lengths
    t_back, perm = bref.transpose(edges_t)
    assert (t_back.num_rows, t_back.num_cols) == (edges.num_rows, edges.num_cols) and np.array_equal(t_back.row_ptrs, edges.row_ptrs)
    assert all(np.array_equal(np.sort(t_back.col_idxs[lo:hi]), np.sort(edges.col_idxs[lo:hi])) for lo, hi in zip(edges.row_ptrs[:-1], edges.row_ptrs[1:]))
    assert np.array_equal(np.sort(perm), np.arange(edges.nnz))
    col_lens = np.bincount(edges_t.col_idxs.astype(np.int64), minlength=edges_t.num_cols)
    assert np.array_equal(col_lens, np.diff(edges.row_ptrs.astype(np.int64)))
    assert {0, 1, 7, 8, 9, 257, 300, 1025} <= set(col_lens.tolist()) and col_lens[0] == 0 and col_lens[-1] == 0
    assert any(0 < n < 8 for n in col_lens) and 8 in col_lens and 9 in col_lens and col_lens.max() > 16 * 8   # partial, one batch, one more, > 16 batches
    for name in bref.PATTERNS:                                   # ... and every pattern has empty columns and empty rows or none to lose
        csr = bref.matrix(name)
        t, perm = bref.transposed(name)
        rows = np.repeat(np.arange(csr.num_rows), np.diff(csr.row_ptrs.astype(np.int64)))
        assert np.array_equal(t.col_idxs, rows[perm]) and np.array_equal(np.sort(csr.col_idxs[perm], kind="stable"), csr.col_idxs[perm])
    for case in bref.CASES:
        op, csr = bref.operands(case), bref.matrix(case.name)
        assert op["k"].shape[0] == 1 and op["v"].shape[0] == 1 and op["g"].shape == (case.heads, csr.num_rows, case.dv)
        if case.bias == "masked":                                # every non-empty row keeps a finite last entry: its lse is finite
            ptrs = csr.row_ptrs.astype(np.int64)
            assert op["bias"].ndim == 1 and all(np.isfinite(op["bias"][ptrs[r + 1] - 1]) for r in range(csr.num_rows) if ptrs[r + 1] > ptrs[r])
            assert np.isneginf(op["bias"]).any()


@pytest.mark.parametrize("case", bref.CASES, ids=lambda c: c.id)
def test_both_passes_as_built_lie_inside_the_tolerances_and_the_tight_check(case):
    got = mut.restated(case)
    assert not any(np.isnan(got[n]).any() for n in ("dq", "dk", "dv"))
    results = {what: check(got, case) for what, check in mut.CHECKS.items()}
    print(f"restated bwd {case.id}: worst |err| / tolerance (dq, dk, dv): " + "; ".join(f"{what} " + ", ".join(f"{w:.3g}" for w in worst) for what, (_, worst) in results.items()))
    for what, (ok, worst) in results.items():
        assert ok and max(worst) <= 1.0, (what, worst)
    # the tight reference alone covers every element: none is flagged or left out
    assert btight.coverage(case, got["out"], got["lse"]) == 1.0
    csr = bref.matrix(case.name)
    empty_rows = np.diff(csr.row_ptrs.astype(np.int64)) == 0
    empty_cols = np.bincount(csr.col_idxs.astype(np.int64), minlength=csr.num_cols) == 0
    assert not got["dq"][:, empty_rows].view(np.uint32).any() and not got["dk"][:, empty_cols].view(np.uint32).any() \
        and not got["dv"][:, empty_cols].view(np.uint32).any()


def test_the_analytic_reference_is_autograd_through_dense_masked_attention():
    torch = pytest.importorskip("torch")
    from _sddmm_ref import dense_of
    from mispmm import formats
    for case in (bref.Case("edgesT", 3, 5, "masked", 3), bref.Case("ragged", 8, 64, "finite", 1)):
        op, csr = bref.operands(case), bref.matrix(case.name)
        want = bref.backward_f64(csr, op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"])
        pat = formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, np.ones(csr.nnz))
        mask = torch.from_numpy(dense_of(pat) > 0)
        for h in range(case.heads):
            add = torch.from_numpy(dense_of(formats.CSR(csr.num_rows, csr.num_cols, csr.row_ptrs, csr.col_idxs, ref._bias_of(op["bias"], h, csr.nnz).astype(np.float64))))
            qt, kt, vt = (torch.from_numpy(ref._head(op[n], h).astype(np.float64)).requires_grad_(True) for n in ("q", "k", "v"))
            sc = ((qt * op["scale"]) @ kt.t() + add).masked_fill(~mask, float("-inf"))
            p = torch.softmax(sc, dim=1).masked_fill(~mask.any(dim=1, keepdim=True), 0.0)
            (p @ vt).backward(torch.from_numpy(op["g"][h].astype(np.float64)))
            for w, t in zip(want, (qt, kt, vt)):
                assert np.allclose(w[h], t.grad.numpy(), rtol=1e-11, atol=1e-13), case.id


CHAIN_FACTOR = 32.0           # no element's tolerance may exceed the chain's by more
CHAIN_MEDIAN = 4.0            # ... and half of them stay within this


@pytest.mark.parametrize("name", ["long", "ragged"])
def test_the_tolerances_stay_within_a_stated_factor_of_the_chains(name):
    """bwd_tolerances against the composed gradient tolerance of the four-launch chain on one head without a bias.  The two
    are different derivations (this one charges the forward's whole out tolerance to delta through sum |g| E_out and the
    stored lse's bound to every P; the chain's carries its own P error through <P, dP>), so they are not equal; a tolerance
    that were merely generous would show as a large ratio here.  dv has no delta and stays below the chain's."""
    pytest.importorskip("torch")
    from test_gpu_softmax import _attention_tolerances
    from _softmax_ref import full_mantissa
    csr = matrix(name)
    rng = np.random.default_rng(46)
    for d in (8, 64):
        q, k, v, g = (full_mantissa(rng, (n, d), np.float32) for n in (csr.num_rows, csr.num_cols, csr.num_cols, csr.num_rows))
        chain = _attention_tolerances(csr, q, k, v, g, d ** -0.5, "fast")[1:]
        mine = bref.bwd_tolerances(csr, q[None], k[None], v[None], g[None], d ** -0.5)
        for what, a, b in zip(("dq", "dk", "dv"), mine, chain):
            ratio = a[0] / b
            print(f"bwd_tolerances / chain tolerance, {name} D={d} {what}: median {np.median(ratio):.3g} max {ratio.max():.3g}")
            assert ratio.max() <= (1.0 if what == "dv" else CHAIN_FACTOR) and np.median(ratio) <= CHAIN_MEDIAN, (what, ratio.max())


def test_special_values_in_the_restatement():
    case = bref.Case("edges", 8, 8, "finite", 1)
    op, csr = dict(bref.operands(case)), bref.matrix("edges")
    ptrs = csr.row_ptrs.astype(np.int64)
    r = int(np.argwhere(np.diff(ptrs) == 33)[0, 0])
    args = lambda b: (csr, op["q"], op["k"], op["v"], op["g"], op["scale"], b)       # noqa: E731
    out, lse = ref.fused_f32(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"])
    clean = bref.backward_f32(*args(op["bias"]), out, lse)
    for what in ("nan", "+inf", "all -inf"):
        b = op["bias"].copy()
        if what == "nan":
            b[ptrs[r] + 20] = np.nan
        if what == "+inf":
            b[ptrs[r] + 3] = np.inf
        if what == "all -inf":
            b[ptrs[r]:ptrs[r + 1]] = -np.inf
        with np.errstate(all="ignore"):
            out, lse = ref.fused_f32(csr, op["q"], op["k"], op["v"], op["scale"], b)
            dq, dk, dv = bref.backward_f32(*args(b), out, lse)
        assert not np.isfinite(lse[0, r])
        hit = np.zeros(csr.num_rows, bool)
        hit[r] = True
        keys = np.zeros(csr.num_cols, bool)
        keys[csr.col_idxs[ptrs[r]:ptrs[r + 1]]] = True
        assert np.array_equal(np.isnan(dq[0]), np.broadcast_to(hit[:, None], dq[0].shape)), what
        assert np.array_equal(np.isnan(dk[0]), np.broadcast_to(keys[:, None], dk[0].shape)), what
        assert np.array_equal(np.isnan(dv[0]), np.broadcast_to(keys[:, None], dv[0].shape)), what
        assert np.array_equal(dq[0][~hit], clean[0][0][~hit]) and np.array_equal(dv[0][~keys], clean[2][0][~keys])


def test_python_layer_refuses_without_a_gpu():
    torch = pytest.importorskip("torch")
    from mispmm import autograd, ops
    csr = matrix("long")
    t = autograd.TrainableCSR.from_host(csr, device="cpu")
    assert t.perm32().dtype == torch.int32 and t.perm32() is t.perm32() and torch.equal(t.perm32().long(), t.perm)
    q, k = torch.zeros((csr.num_rows, 8)), torch.zeros((csr.num_cols, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.attention_csr_bwd(t.fwd, t.tpattern, t.perm32(), q, k, k, q, torch.zeros(csr.num_rows), q)
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.sparse_attention(t, q, k, k, fused=True, fused_backward=True)
    with pytest.raises(ValueError, match="needs fused=True"):
        autograd.sparse_attention(t, q, k, k, fused_backward=True)
