"""The row-list product with B in bf16 (libmispmm_bf16.so, include/mispmm_bf16.h) on a machine WITHOUT a GPU: the fourth library
and its binding, the census of its kernel instances and their tags, the entry point's refusals (which precede any device work),
the ValueErrors of the Python layer, the sharpness of the data the GPU tests judge the arithmetic on, and the numpy restatement
of the three contracts (tests/_spmm_bf16_ref.py) against the chain in exact rational arithmetic."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_bf16

import _fma_chain as fc
import _spmm_bf16_ref as ref
from test_census_cpu import _symbol_tool

INSTANCES = {"rows_bf16_kernel": 36}       # __device_stub__ symbols of libmispmm_bf16.so per kernel template: 4 G x 3 V x 3 arithmetics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INV, UNS = capi.OK, capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED


def test_the_fourth_library_exports_what_its_header_declares_and_the_binding_binds_it():
    assert os.path.exists(capi_bf16.LIB_PATH), f"{capi_bf16.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_bf16.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_bf16.SIGNATURES) == {"mispmm_rows_bf16"}
    tool = _symbol_tool()
    if tool is not None:
        out = subprocess.run([tool, "-D", "--defined-only", capi_bf16.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("mispmm_")}
        assert exported == declared, exported
    handle = ctypes.CDLL(capi_bf16.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in mispmm_bf16.h but not exported"
    lib = capi_bf16.lib()
    for name, (_, argtypes) in capi_bf16.SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes
    # the tag and the error text are read through the handle of the library loaded here
    assert capi_bf16.last_kernel() == lib.mispmm_last_kernel().decode()
    # the first library, its header and its binding gain nothing
    with open(os.path.join(ROOT, "include", "mispmm.h"), encoding="utf-8") as f:
        assert "rows_bf16" not in f.read()
    assert not any("rows_bf16" in n for n in capi.SIGNATURES)
    assert not hasattr(ctypes.CDLL(capi.LIB_PATH), "mispmm_rows_bf16")


ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced


def _call(**kw):
    a = dict(stream=None, M=4, K=4, nnz=3, rowPtrs=ONE, rowNnz=0, colIdxs=ONE, vals=ONE, B=ONE, N=8, ldb=8, C=ONE, ldc=8, out_bf16=0, acc=0, sum_f32=0)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_bf16.lib().mispmm_rows_bf16(*a.values())


def test_every_refusal_returns_its_status_and_its_message_before_any_device_work():
    err = capi_bf16.last_error
    for acc in (2, -1, 7):
        assert _call(acc=acc) == INV and "rows_bf16" in err() and f"unknown accumulate mode {acc}" in err()
    for name in ("colIdxs", "vals"):
        assert _call(**{name: None}) == INV, name
        assert "rows_bf16: colIdxs or vals is null" in err()
    for name in ("B", "C"):
        assert _call(**{name: None}) == INV, name
        assert "rows_bf16: B or C is null" in err()
    for kw in (dict(ldb=7), dict(ldc=7), dict(N=9)):
        assert _call(**kw) == INV, kw
        assert "leading dimension smaller than N" in err()
    # alignment: B to 2 bytes, C to 4 (fp32) or 2 (bf16)
    for kw in (dict(B=ONE + 1), dict(C=ONE + 2), dict(C=ONE + 1), dict(C=ONE + 1, out_bf16=1), dict(B=ONE + 3, out_bf16=1)):
        assert _call(**kw) == INV, kw
        assert "aligned" in err()
    # the uniform list: M * rowNnz must be nnz
    for kw in (dict(rowPtrs=None, rowNnz=2, nnz=7), dict(rowPtrs=None, rowNnz=0, nnz=3), dict(rowPtrs=None, rowNnz=1 << 31, nnz=0)):
        assert _call(**kw) == INV, kw
        assert "M * rowNnz != nnz" in err()
    # a B or a C that spans 2 GiB or more: there is no wide body
    assert _call(K=1 << 20, ldb=1 << 10) == UNS and "2 GiB" in err()                  # 2 GiB of bf16
    assert _call(M=1 << 19, ldc=1 << 10) == UNS and "2 GiB" in err()                  # 2 GiB of fp32 C
    assert _call(M=1 << 20, ldc=1 << 10, out_bf16=1) == UNS and "2 GiB" in err()      # 2 GiB of bf16 C
    # the order: an unknown mode before everything, a null pointer before the size
    assert _call(acc=5, B=None, ldb=1) == INV and "unknown accumulate mode" in err()
    assert _call(B=None, K=1 << 20, ldb=1 << 10) == INV and "null" in err()


def test_no_ops_return_after_the_checks_that_look_at_no_pointer():
    nulls = dict(rowPtrs=None, colIdxs=None, vals=None, B=None, C=None)
    assert _call(M=0, nnz=0, **nulls) == OK
    assert _call(N=0, rowNnz=2, nnz=8, **nulls) == OK
    assert _call(M=0, acc=3) == INV
    assert _call(N=0, ldb=0, ldc=0, nnz=5, rowPtrs=None, rowNnz=1) == INV and "M * rowNnz != nnz" in capi_bf16.last_error()
    assert _call(M=0, ldb=4) == INV


def _symbols():
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    return subprocess.run([tool, "-C", capi_bf16.LIB_PATH], capture_output=True, text=True, check=True).stdout


def test_the_new_library_holds_the_recorded_instances_and_the_tag_table_lists_each():
    out = _symbols()
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found == INSTANCES, f"kernel template: instances in the library {found}, recorded here {INSTANCES}"
    word = {"AccFast": "fast", "AccRefWide": "ref64", "AccRefF32": "ref32"}
    tags = set()
    for args in set(re.findall(r"__device_stub__rows_bf16_kernel<([^>]*)>", out)):
        g, v, acc = (s.strip() for s in args.split(","))
        tags.add(f"rows_bf16<G{g},V{v},{word[acc.split('::')[-1]]}>")
    assert tags == set(ref.TAGS), (sorted(tags - set(ref.TAGS)), sorted(set(ref.TAGS) - tags))
    assert len(ref.TAGS) == INSTANCES["rows_bf16_kernel"]
    for tag, n in ref.TAGS.items():
        mode = tag[:-1].split(",")[-1]
        v = int(re.search(r",V(\d)", tag).group(1))
        for out_bf16 in (False, True):
            assert ref.tag_of(mode, n, out_bf16=out_bf16) == tag
            # the smallest: one lane's columns less is another tag (or no launch)
            assert n == v or ref.tag_of(mode, n - v, out_bf16=out_bf16) != tag
    assert set(ref.SMALLEST_N.values()) <= set(ref.WIDTHS)
    # nothing leaked into the other three libraries
    from mispmm import capi_attn, capi_attn_bwd
    for path in (capi.LIB_PATH, capi_attn.LIB_PATH, capi_attn_bwd.LIB_PATH):
        other = subprocess.run([_symbol_tool(), "-C", path], capture_output=True, text=True, check=True).stdout
        assert "rows_bf16" not in other, path


def test_the_lane_width_rule_of_the_restatement():
    assert ref.pick(128, 128, 128) == (16, 8)
    assert ref.pick(128, 128, 132) == (16, 8) and ref.pick(128, 128, 132, out_bf16=True) == (32, 4)      # ldc % 8 for a bf16 C
    assert ref.pick(128, 128, 130) == (32, 4) and ref.pick(128, 128, 130, out_bf16=True) == (64, 1)
    assert ref.pick(128, 128, 128, b_off=8) == (16, 8)            # 16 bytes further: still 16-byte lanes
    assert ref.pick(128, 128, 128, b_off=4) == (32, 4)
    assert ref.pick(128, 128, 128, b_off=1) == (64, 1)
    assert ref.pick(128, 128, 128, c_off=2) == (32, 4) and ref.pick(128, 128, 128, c_off=1) == (64, 1)
    assert ref.pick(128, 132, 128) == (32, 4) and ref.pick(128, 129, 128) == (64, 1)
    assert ref.pick(520, 520, 520) == (64, 8) and ref.pick(65, 65, 65) == (64, 1)


def test_bf16_helpers_round_to_nearest_even_and_widen_exactly():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    x = fc.sharp_values(rng, 4096, np.float32)
    x[:8] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 3.3895314e38, 1e-40, -1e-45]       # the last finite one rounds to Inf
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = ref.bf16_bits(x)
    assert ref.same_bits(got, want)
    assert np.array_equal(ref.widen(got)[1:], torch.from_numpy(want.view(np.int16)).view(torch.bfloat16).to(torch.float32).numpy()[1:])
    every = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)                    # all 65536 bf16 values: widen then round is the identity
    assert ref.same_bits(ref.bf16_bits(ref.widen(every)), every)
    assert np.array_equal(ref.widen(every).view(np.uint32), every.astype(np.uint32) << 16)


@pytest.mark.parametrize("name", ["n3c5-b6", "ragged"])
def test_the_data_is_sharp_and_the_three_contracts_differ(name):
    """References alone: on these operands (fp32 values with full mantissas, B the same kind rounded to bf16) an unfused and a
    reversed chain differ from the fma chain in well over SHARP_SHARE of the elements, the three contracts differ pairwise,
    and almost none of it survives a rounding of C to bf16 -- which is why the arithmetic is judged on the fp32 C."""
    c = ref.case(name)
    for n in (1, 8, 19):
        unfused, backwards, count = c.sharpness(n)
        print(f"{name} N={n}: unfused differs in {unfused:.2f}, reversed in {backwards:.2f} of {count} elements")
        assert c.is_sharp(n)
    multi = np.diff(c.row_ptrs.astype(np.int64)) >= 2
    outs = {m: c.expected(m)[multi][:, :19] for m in ref.MODES}
    for x, y in (("fast", "ref64"), ("fast", "ref32"), ("ref64", "ref32")):
        share = float(np.mean(outs[x].view(np.uint32) != outs[y].view(np.uint32)))
        after = float(np.mean(ref.bf16_bits(outs[x]) != ref.bf16_bits(outs[y])))
        print(f"{name}: {x} and {y} differ in {share:.2f} of the elements, in {after:.4f} after rounding to bf16")
        assert share >= fc.SHARP_SHARE
        assert after <= 0.01
    # bf16-representable values of A would make every product exact (8 x 8 bits of mantissa), and then the fused and the
    # unfused chain are the same chain: such data discriminates nothing, hence fp32 values with full mantissas
    exactv = ref.widen(ref.bf16_bits(c.vals))
    b = ref.widen(c.b_bits[:, :19])
    assert np.array_equal(fc._oracle().rows_fma(c.row_ptrs, c.col_idxs, exactv, b).view(np.uint32),
                          fc.chain_unfused(c.row_ptrs, c.col_idxs, exactv, b).view(np.uint32))


def test_the_restatement_agrees_with_the_chain_in_exact_arithmetic():
    """A few dozen elements of the FAST contract through fractions.Fraction, padding slots as dead slots included; the two
    REFERENCE rules against their definitions written out in numpy scalars."""
    rng = np.random.default_rng(5)
    lens = np.array([0, 1, 2, 5, 9, 17, 3, 0])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cols = rng.integers(0, 12, int(rp[-1])).astype(np.uint32)
    vals = fc.sharp_values(rng, int(rp[-1]), np.float32)
    bits = ref.bf16_bits(fc.sharp_values(rng, (12, 6), np.float32))
    b = ref.widen(bits)
    assert np.array_equal(ref.expected("fast", rp, cols, vals, bits).view(np.uint32), fc.chain_exact(rp, cols, vals, b).view(np.uint32))
    want64, want32 = np.zeros((8, 6), np.float32), np.zeros((8, 6), np.float32)
    for r in range(8):
        for j in range(6):
            s64, s32 = np.float64(0.0), np.float32(0.0)
            for e in range(rp[r], rp[r + 1]):
                p = np.float32(vals[e] * b[cols[e], j])
                s64, s32 = s64 + np.float64(p), np.float32(s32 + p)
            want64[r, j], want32[r, j] = np.float32(s64), s32
    assert np.array_equal(ref.expected("ref64", rp, cols, vals, bits).view(np.uint32), want64.view(np.uint32))
    assert np.array_equal(ref.expected("ref32", rp, cols, vals, bits).view(np.uint32), want32.view(np.uint32))
    # a padded uniform list: the padding slots hold a NaN and an Inf and contribute +0
    width = 4
    pc = np.full((5, width), ref.PAD, np.uint32)
    pv = np.full((5, width), np.nan, np.float32)
    pv[3] = np.inf
    for r, n in enumerate((4, 2, 0, 1, 3)):
        pc[r, :n] = rng.integers(0, 12, n)
        pv[r, :n] = fc.sharp_values(rng, n, np.float32)
    live = pc != ref.PAD
    crp = np.concatenate([[0], np.cumsum(live.sum(axis=1))]).astype(np.uint32)
    for mode in ref.MODES:
        got = ref.expected(mode, None, pc, pv, bits, row_nnz=width)
        assert not np.isnan(got).any()
        assert np.array_equal(got.view(np.uint32), ref.expected(mode, crp, pc[live], pv[live], bits).view(np.uint32)), mode
    assert np.array_equal(ref.expected("fast", None, pc, pv, bits, row_nnz=width).view(np.uint32),
                          fc.chain_exact(crp, pc[live], pv[live], b).view(np.uint32))


def test_python_layer_refuses_wrong_operands_with_value_errors():
    torch = pytest.importorskip("torch")
    from mispmm import autograd, formats, ops
    from test_softmax_bsr_cpu import _OnDevice
    c = ref.case("edges")
    csr = c.csr()
    m, k = csr.num_rows, csr.num_cols
    a = ops.DeviceCSR.from_host(csr, device="cpu")
    coo = ops.DeviceCOO.from_host(formats.csr_to_coo(csr), device="cpu")
    ell = ops.DeviceELL.from_host(formats.csr_to_ell_rowmajor(csr), device="cpu", compact=False)
    bits = torch.zeros((k, 8), dtype=torch.int16)
    for f, x in ((ops.spmm_csr_bf16, a), (ops.spmm_coo_bf16, coo), (ops.spmm_ell_bf16, ell)):
        with pytest.raises(ValueError, match="no CPU path"):
            f(x, bits)
    t = autograd.TrainableCSR.from_host(csr, device="cpu")
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.spmm_bf16(t, t.values, bits.view(torch.bfloat16))

    dev = lambda *shape, dtype=torch.int16: _OnDevice(torch.zeros(*shape, dtype=dtype))   # noqa: E731
    on = lambda x, *names: [setattr(x, n, _OnDevice(getattr(x, n))) for n in names]      # noqa: E731
    on(a, "row_ptrs", "col_idxs", "data")
    on(coo, "row_idxs", "col_idxs", "data")
    coo.row_bounds = _OnDevice(torch.zeros(m + 1, dtype=torch.int32))
    on(ell, "col_idxs", "data")
    a64 = ops.DeviceCSR.from_host(csr, device="cpu", dtype=torch.float64)
    on(a64, "row_ptrs", "col_idxs", "data")
    for f, x in ((ops.spmm_csr_bf16, a), (ops.spmm_coo_bf16, coo), (ops.spmm_ell_bf16, ell)):
        bad = [lambda: f(x, dev(k, 8, dtype=torch.bfloat16)),                        # bits are int16
               lambda: f(x, dev(k, 8, dtype=torch.float32)),
               lambda: f(x, dev(k + 1, 8)),                                          # rows of B
               lambda: f(x, dev(k * 8)),                                             # 2-D
               lambda: f(x, _OnDevice(torch.zeros((8, k), dtype=torch.int16).t())),  # unit column stride
               lambda: f(x, dev(k, 8), out=dev(m, 8)),                               # fp32 asked for
               lambda: f(x, dev(k, 8), out_bf16=True, out=dev(m, 8, dtype=torch.float32)),
               lambda: f(x, dev(k, 8), out=dev(m + 1, 8, dtype=torch.float32)),
               lambda: f(x, dev(k, 8), out=_OnDevice(torch.zeros((8, m), dtype=torch.float32).t())),
               lambda: f(x, dev(k, 8), acc="exact")]
        for i, g in enumerate(bad):
            with pytest.raises(ValueError):
                g()
                pytest.fail(f"{f.__name__}: case {i} was not refused")
    with pytest.raises(ValueError, match="float32 matrix"):
        ops.spmm_csr_bf16(a64, dev(k, 8))
    with pytest.raises(ValueError, match="ref_sum"):
        ops.spmm_csr_bf16(a, dev(k, 8), ref_sum="f16")

    on(t.fwd, "row_ptrs")
    vals = _OnDevice(t.values)
    bf = lambda *shape: dev(*shape, dtype=torch.bfloat16)                                 # noqa: E731
    bad = [lambda: autograd.spmm_bf16(t, vals, dev(k, 8, dtype=torch.float32)),
           lambda: autograd.spmm_bf16(t, vals, dev(k, 8)),                           # int16 bits are the ops layer's
           lambda: autograd.spmm_bf16(t, _OnDevice(t.values.to(torch.bfloat16)), bf(k, 8)),
           lambda: autograd.spmm_bf16(t, _OnDevice(t.values[:-1]), bf(k, 8)),
           lambda: autograd.spmm_bf16(t, vals, bf(k + 1, 8)),
           lambda: autograd.spmm_bf16(t, vals, bf(2, k, 8)),
           lambda: autograd.spmm_bf16(t, vals, _OnDevice(torch.zeros((8, k), dtype=torch.bfloat16).t())),
           lambda: autograd.spmm_bf16(t, vals, bf(k, 8), out_dtype=torch.float16),
           lambda: autograd.spmm_bf16(t, vals, bf(k, 8), acc="exact")]
    for i, g in enumerate(bad):
        with pytest.raises(ValueError):
            g()
            pytest.fail(f"autograd.spmm_bf16: case {i} was not refused")
    t64 = autograd.TrainableCSR.from_host(csr, device="cpu", dtype=torch.float64)
    on(t64.fwd, "row_ptrs")
    with pytest.raises(ValueError, match="float32 matrix"):
        autograd.spmm_bf16(t64, _OnDevice(t64.values), bf(k, 8))
