"""SDDMM on a CSR pattern with X and Y in bf16 (libmispmm_sddmm_bf16.so, include/mispmm_sddmm_bf16.h) on a machine WITHOUT a
GPU: the ninth library and its binding, the census of its kernel instances and their tags, the entry point's refusals (which
precede any device work), the ValueErrors of the Python layer, the sharpness of the operands the GPU tests judge the arithmetic
on, and the numpy restatement of ALGORITHM (tests/_sddmm_bf16_ref.py) against exact sums and against its own named breaches."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mispmm import capi, capi_sddmm_bf16

import _sddmm_bf16_ref as ref
from _sddmm_ref import bound, small_ints
from test_census_cpu import _symbol_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INV, UNS = capi.OK, capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
FLOOR = 0.05                               # least share of entries on which two orders, or an order and the exact sum, must differ


def test_the_ninth_library_exports_what_its_header_declares_and_the_binding_binds_it():
    assert os.path.exists(capi_sddmm_bf16.LIB_PATH), f"{capi_sddmm_bf16.LIB_PATH} is not built"
    with open(os.path.join(ROOT, "include", "mispmm_sddmm_bf16.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(mispmm_[a-z0-9_]+)\s*\(", text))
    assert declared == set(capi_sddmm_bf16.SIGNATURES) == {"mispmm_sddmm_csr_bf16"}
    tool = _symbol_tool()
    if tool is not None:
        out = subprocess.run([tool, "-D", "--defined-only", capi_sddmm_bf16.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("mispmm_")}
        assert exported == declared, exported
    handle = ctypes.CDLL(capi_sddmm_bf16.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in mispmm_sddmm_bf16.h but not exported"
    lib = capi_sddmm_bf16.lib()
    for name, (_, argtypes) in capi_sddmm_bf16.SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes
    # the tag and the error text are read through the handle of the library loaded here
    assert capi_sddmm_bf16.last_kernel() == lib.mispmm_last_kernel().decode()
    # the first library, its header and its binding gain nothing
    with open(os.path.join(ROOT, "include", "mispmm.h"), encoding="utf-8") as f:
        assert "sddmm_csr_bf16" not in f.read()
    assert not any("sddmm_csr_bf16" in n for n in capi.SIGNATURES)
    assert not hasattr(ctypes.CDLL(capi.LIB_PATH), "mispmm_sddmm_csr_bf16")


ONE = 64                                   # a fake pointer, 16-byte aligned, never dereferenced


def _call(**kw):
    a = dict(stream=None, M=4, K=4, nnz=3, rowPtrs=ONE, colIdxs=ONE, X=ONE, ldx=8, Y=ONE, ldy=8, N=8, out=ONE, out_bf16=0, acc=0)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return capi_sddmm_bf16.lib().mispmm_sddmm_csr_bf16(*a.values())


def test_every_refusal_returns_its_status_and_its_message_before_any_device_work():
    err = capi_sddmm_bf16.last_error
    for acc in (2, -1, 7):
        assert _call(acc=acc) == INV and "sddmm_csr_bf16" in err() and f"unknown accumulate mode {acc}" in err()
    for kw in (dict(ldx=7), dict(ldy=7), dict(N=9)):
        assert _call(**kw) == INV, kw
        assert "leading dimension smaller than N" in err()
    for name in ("rowPtrs", "colIdxs", "out"):
        assert _call(**{name: None}) == INV, name
        assert "sddmm_csr_bf16: rowPtrs, colIdxs or out is null" in err()
    for name in ("X", "Y"):
        assert _call(**{name: None}) == INV, name
        assert "sddmm_csr_bf16: X or Y is null" in err()
    # alignment: X and Y to 2 bytes, out to 4 (fp32) or 2 (bf16)
    for kw in (dict(X=ONE + 1), dict(Y=ONE + 3), dict(X=ONE + 1, out_bf16=1)):
        assert _call(**kw) == INV, kw
        assert "X and Y must be 2-byte aligned" in err()
    for kw, word in ((dict(out=ONE + 2), "4-byte"), (dict(out=ONE + 1), "4-byte"), (dict(out=ONE + 1, out_bf16=1), "2-byte")):
        assert _call(**kw) == INV, kw
        assert f"out must be {word} aligned" in err()
    # an X or a Y that spans 2 GiB or more: there is no wide body
    assert _call(M=1 << 20, ldx=1 << 10) == UNS and "2 GiB" in err()
    assert _call(K=1 << 20, ldy=1 << 10) == UNS and "2 GiB" in err()
    assert _call(K=(1 << 20) - 1, ldy=1 << 10, Y=None) == INV              # just below: not the size
    # the order: an unknown mode before everything, the leading dimensions before the pointers, a null pointer before the size
    assert _call(acc=5, X=None, ldx=1) == INV and "unknown accumulate mode" in err()
    assert _call(ldx=1, X=None) == INV and "leading dimension" in err()
    assert _call(X=None, M=1 << 20, ldx=1 << 10) == INV and "null" in err()


def test_no_ops_return_after_the_checks_that_look_at_no_pointer():
    nulls = dict(rowPtrs=None, colIdxs=None, X=None, Y=None, out=None)
    assert _call(M=0, nnz=0, **nulls) == OK
    assert _call(nnz=0, **nulls) == OK
    assert _call(M=0, **nulls) == OK
    assert _call(M=0, acc=3) == INV
    assert _call(nnz=0, ldx=4) == INV and "leading dimension" in capi_sddmm_bf16.last_error()
    # N == 0 with work to do still needs its index arrays and its out (the memset's target)
    assert _call(N=0, ldx=0, ldy=0, out=None) == INV and "null" in capi_sddmm_bf16.last_error()
    assert _call(N=0, ldx=0, ldy=0, out=ONE + 2) == INV and "aligned" in capi_sddmm_bf16.last_error()


def _symbols():
    tool = _symbol_tool()
    if tool is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    return subprocess.run([tool, "-C", capi_sddmm_bf16.LIB_PATH], capture_output=True, text=True, check=True).stdout


def test_the_new_library_holds_the_recorded_instances_and_the_tag_table_lists_each():
    out = _symbols()
    found = {}
    for name in re.findall(r"__device_stub__([A-Za-z0-9_]+)", out):
        found[name] = found.get(name, 0) + 1
    assert found == ref.INSTANCES, f"kernel template: instances in the library {found}, recorded here {ref.INSTANCES}"
    word = {"SdRef": "ref64", "SdFast": "fast"}
    tags = set()
    for args in set(re.findall(r"__device_stub__sddmm_csr_bf16_kernel<(.*?)>\(", out)):
        p, g, v, c = (s.strip() for s in args.rsplit(",", 3))
        tags.add(f"sddmm_csr_bf16<{word[p.split('::')[-1]]},G{g},V{v},C{c}>")
    assert tags == set(ref.TAGS), (sorted(tags - set(ref.TAGS)), sorted(set(ref.TAGS) - tags))
    assert len(ref.TAGS) == ref.INSTANCES["sddmm_csr_bf16_kernel"]
    for tag, n in ref.TAGS.items():
        acc = "fast" if "<fast," in tag else "reference"
        v = int(re.search(r",V(\d)", tag).group(1))
        for out_bf16 in (False, True):
            assert ref.head(ref.tag_of(acc, n, out_bf16=out_bf16)) == tag
        # the smallest: one lane's columns less is another tag.  G8 is reached from one lane's columns on; its V1 width is 3, an
        # odd width of more than one column
        g = int(re.search(r",G(\d+)", tag).group(1))
        assert n == (8 if v == 8 else 3) if g == 8 else ref.head(ref.tag_of(acc, n - v)) != tag
    assert sorted(ref.V8_WIDTHS) == [8, 72, 136, 264, 520, 1032, 2056] and sorted(ref.V1_WIDTHS) == [3, 9, 17, 33, 65, 129, 257]
    # nothing leaked into the libraries whose instances other tests hold to their records
    from mispmm import capi_bf16
    for path in (capi.LIB_PATH, capi_bf16.LIB_PATH):
        other = subprocess.run([_symbol_tool(), "-C", path], capture_output=True, text=True, check=True).stdout
        assert "sddmm_csr_bf16" not in other, path


def test_the_lane_width_rule_of_the_restatement():
    assert ref.pick(128) == (16, 8, 1) and ref.pick(40) == (8, 8, 1) and ref.pick(33) == (64, 1, 1)
    assert ref.pick(128, 136, 128) == (16, 8, 1) and ref.pick(128, 132, 128) == (64, 1, 2) and ref.pick(128, 128, 131) == (64, 1, 2)
    assert ref.pick(128, x_off=8) == (16, 8, 1) and ref.pick(128, x_off=1) == (64, 1, 2) and ref.pick(128, y_off=4) == (64, 1, 2)
    assert ref.pick(4) == (8, 1, 1) and ref.pick(12) == (16, 1, 1)            # there is no V4
    assert ref.pick(512) == (64, 8, 1) and ref.pick(2048) == (64, 8, 4) and ref.pick(4096) == (64, 8, 0)
    assert ref.tag_of("reference", 40, out_bf16=True) == "sddmm_csr_bf16<ref64,G8,V8,C1> bf16"
    assert ref.tag_of("fast", 33, 36, 36, x_off=1) == "sddmm_csr_bf16<fast,G64,V1,C1> f32"


def test_the_operands_have_eight_significant_bits_and_their_exact_sums_fit_a_double():
    c = ref.case("census")
    for bits, spread in ((c.x_bits, 4), (c.y_bits, 4), (c._x_far, 40), (c._y_far, 40)):
        v = ref.widen(bits)
        m, e = np.frexp(v.astype(np.float64))
        assert np.all(m * 256 == np.round(m * 256)) and (np.abs(m) * 256 % 2 == 1).mean() > 0.4      # 8 bits, the last one used
        assert e.min() - 1 == -spread and e.max() - 1 == spread and 0.45 < (v < 0).mean() < 0.55
    # 16 product bits + 17 of exponent spread + ceil(log2 2056) = 45 <= 53
    assert 16 + (2 * 4 + 2 * 4 + 1) + int(np.ceil(np.log2(ref.MAX_N))) <= 53


def _share(a, b):
    return float(np.mean(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)))


@pytest.mark.parametrize("name, widths", [("census", sorted(ref.V8_WIDTHS + [n for n in ref.V1_WIDTHS if n >= 8])), ("ragged", [40, 33])])
def test_the_operands_are_sharp_order_and_rounding_show_in_the_bits(name, widths):
    """References alone.  On these operands FAST's result depends on the order of its additions -- the V8 and the V1 order
    differ -- and differs from the correctly rounded sum, each on more than FLOOR of the entries at every width >= 8 the GPU
    tests use; REFERENCE is the correctly rounded sum in either order, and on the operands of exponents -40 .. 40 it is not."""
    c = ref.case(name)
    for n in widths:
        want, exact, scale = c.exact(n)
        f8, f1 = c.expected("fast", n, 8 if n % 8 == 0 else None), c.expected("fast", n, 1)
        order, rounding = _share(f8, f1), min(_share(f8, want), _share(f1, want))
        print(f"{name} N={n}: FAST V8 and V1 order differ on {order:.2f} of {want.size} entries, FAST and the rounded exact sum on {rounding:.2f}")
        if n % 8 == 0:
            assert order >= FLOOR
        assert rounding >= FLOOR
        for v in ((8, 1) if n % 8 == 0 else (1,)):
            assert ref.same_bits(c.expected("reference", n, v), want), (n, v)
            lim = bound(np.float32, "fast", n, exact, scale)
            assert np.all(np.abs(c.expected("fast", n, v).astype(np.float64) - exact) <= lim)
    n = 264 if name == "census" else 40
    r8, r1 = c.expected("reference", n, 8, far=True), c.expected("reference", n, 1, far=True)
    want = ref.rounded_exact(c.row_ptrs, c.col_idxs, *c.far(n))[0]
    print(f"{name} N={n}, exponents -40..40: REFERENCE V8 and V1 order differ on {_share(r8, r1):.2f} of the entries, V8 and the rounded exact "
          f"sum on {_share(r8, want):.2f}")
    assert _share(r8, r1) >= FLOOR and _share(r8, want) >= FLOOR and _share(r1, want) >= FLOOR


def test_the_restatement_equals_the_exact_sum_on_small_integers_in_both_modes_and_widths():
    c = ref.case("census")
    rng = np.random.default_rng(8)
    for n in (8, 40, 33, 72, 520, 257):
        x = small_ints(rng, (c.csr.num_rows, n), np.float32)
        y = small_ints(rng, (c.csr.num_cols, n), np.float32)
        xb, yb = ref.bf16_bits(x), ref.bf16_bits(y)
        assert np.array_equal(ref.widen(xb), x) and np.array_equal(ref.widen(yb), y)
        rows = np.repeat(np.arange(c.csr.num_rows), np.diff(c.row_ptrs.astype(np.int64)))
        want = (x.astype(np.int64)[rows] * y.astype(np.int64)[c.col_idxs.astype(np.int64)]).sum(axis=1).astype(np.float32)
        for acc in ("fast", "reference"):
            for v in ((8, 1) if n % 8 == 0 else (1,)):
                assert np.array_equal(ref.restate(acc, c.row_ptrs, c.col_idxs, xb, yb, v=v), want), (n, acc, v)
    assert ref.restate("fast", c.row_ptrs, c.col_idxs, xb[:, :0], yb[:, :0]).tolist() == [0.0] * c.col_idxs.shape[0]


# fault -> (acc, N, lane width, strided by) of a case whose bits it must change
FAULT_CASES = {"swap_halves": ("fast", 40, 8, 0), "drop_last_chunk": ("reference", 520, 8, 0), "drop_eighth_slot": ("reference", 40, 8, 0),
               "tree_high_first": ("fast", 72, 8, 0), "ref_in_f32": ("reference", 72, 8, 0), "x_next_row": ("reference", 33, 1, 0),
               "read_gap": ("reference", 40, 8, 8)}


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_every_named_breach_changes_the_bits_of_its_case(fault):
    assert set(FAULT_CASES) == set(ref.FAULTS)
    acc, n, v, gap = FAULT_CASES[fault]
    c = ref.case("census")
    x, y = c.x_bits[:, :n + gap], c.y_bits[:, :n + gap]          # the gap columns hold further operands: finite, non-zero
    good = ref.restate(acc, c.row_ptrs, c.col_idxs, x, y, n=n, v=v)
    assert ref.same_bits(good, c.expected(acc, n, v))
    bad = ref.restate(acc, c.row_ptrs, c.col_idxs, x, y, n=n, v=v, fault=fault)
    share = _share(good, bad)
    print(f"{fault}: {acc} N={n} V{v}: {share:.2f} of the entries change")
    assert share > 0 and not ref.same_bits(good, bad)
    if fault == "drop_eighth_slot":
        assert share < 0.2                                            # only the rows with a full batch
    if fault in ("swap_halves", "tree_high_first", "ref_in_f32", "x_next_row", "read_gap", "drop_last_chunk"):
        assert share >= FLOOR


class _OnDeviceCSR:
    """What sddmm_csr_bf16 reads of a DeviceCSR, with index arrays that say they live on the device."""
    def __init__(self, csr, on):
        import torch
        self.num_rows, self.num_cols, self.nnz = csr.num_rows, csr.num_cols, int(csr.col_idxs.shape[0])
        self.row_ptrs = on(torch.zeros(csr.num_rows + 1, dtype=torch.int32))
        self.col_idxs = on(torch.zeros(self.nnz, dtype=torch.int32))


def test_python_layer_refuses_wrong_operands_with_value_errors():
    torch = pytest.importorskip("torch")
    from mispmm import autograd, ops, sddmm_bf16
    from test_softmax_bsr_cpu import _OnDevice
    c = ref.case("census")
    csr = c.csr
    m, k, nnz = csr.num_rows, csr.num_cols, int(csr.col_idxs.shape[0])
    f = sddmm_bf16.sddmm_csr_bf16
    # tensors of the host: every defect is named first, and sound operands meet "no CPU path"
    a_cpu = ops.DeviceCSR.from_host(csr, device="cpu")
    host = lambda *shape, dtype=torch.int16: torch.zeros(*shape, dtype=dtype)          # noqa: E731
    with pytest.raises(ValueError, match="no CPU path"):
        f(a_cpu, host(m, 8), host(k, 8))
    with pytest.raises(ValueError, match="x_bf16 must be an int16 tensor"):
        f(a_cpu, host(m, 8, dtype=torch.bfloat16), host(k, 8))
    a = _OnDeviceCSR(csr, _OnDevice)
    dev = lambda *shape, dtype=torch.int16: _OnDevice(torch.zeros(*shape, dtype=dtype))   # noqa: E731
    bad = [(lambda: f(a, dev(m, 8, dtype=torch.bfloat16), dev(k, 8)), "x_bf16 must be an int16"),     # bits are int16
           (lambda: f(a, dev(m, 8), dev(k, 8, dtype=torch.float32)), "y_bf16 must be an int16"),
           (lambda: f(a, dev(m + 1, 8), dev(k, 8)), "x_bf16 must be"),                                # rows against a
           (lambda: f(a, dev(m, 8), dev(k - 1, 8)), "y_bf16 must be"),
           (lambda: f(a, dev(m * 8), dev(k, 8)), "x_bf16 must be"),                                   # rank
           (lambda: f(a, dev(m, 8), dev(2, k, 8)), "y_bf16 must be"),
           (lambda: f(a, _OnDevice(torch.zeros((8, m), dtype=torch.int16).t()), dev(k, 8)), "x_bf16 must have unit column stride"),
           (lambda: f(a, dev(m, 8), _OnDevice(torch.zeros((k, 16), dtype=torch.int16)[:, ::2])), "y_bf16 must have unit column stride"),
           (lambda: f(a, _OnDevice(torch.zeros(8, dtype=torch.int16).expand(m, 8)), dev(k, 8)), "x_bf16 must not overlap its own rows"),
           (lambda: f(a, dev(m, 8), _OnDevice(torch.zeros((k + 1, 4), dtype=torch.int16).as_strided((k, 8), (4, 1)))), "y_bf16 must not overlap"),
           (lambda: f(a, dev(m, 8), dev(k, 16)), "same number of columns"),
           (lambda: f(a, dev(m, 8), dev(k, 8), out=dev(nnz)), "out must be a float32 tensor"),        # fp32 asked for
           (lambda: f(a, dev(m, 8), dev(k, 8), out_bf16=True, out=dev(nnz, dtype=torch.float32)), "out must be an int16 tensor"),
           (lambda: f(a, dev(m, 8), dev(k, 8), out=dev(nnz + 1, dtype=torch.float32)), "out must be a contiguous 1-D tensor"),
           (lambda: f(a, dev(m, 8), dev(k, 8), out=dev(nnz, 1, dtype=torch.float32)), "out must be a contiguous 1-D tensor"),
           (lambda: f(a, dev(m, 8), dev(k, 8), out=_OnDevice(torch.zeros(2 * nnz, dtype=torch.float32)[::2])), "out must be a contiguous"),
           (lambda: f(a, dev(m, 8), dev(k, 8), acc="exact"), "acc must be one of")]
    for i, (g, words) in enumerate(bad):
        with pytest.raises(ValueError, match=words):
            g()
            pytest.fail(f"sddmm_csr_bf16: case {i} was not refused")

    class _Negative(_OnDevice):                                       # torch itself makes no negative stride: a stand-in that reports one
        def stride(self, *dim):
            s = (-8, 1)
            return s[dim[0]] if dim else s
    with pytest.raises(ValueError, match="x_bf16 must not have a negative stride"):
        f(a, _Negative(torch.zeros((m, 8), dtype=torch.int16)), dev(k, 8))

    # autograd.spmm_bf16: the new keyword
    t = autograd.TrainableCSR.from_host(csr, device="cpu")
    t.fwd.row_ptrs = _OnDevice(t.fwd.row_ptrs)
    b = dev(k, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="sddmm must be 'f32' or 'bf16', not 'bf17'"):
        autograd.spmm_bf16(t, _OnDevice(t.values), b, sddmm="bf17")
    with pytest.raises(ValueError, match="no CPU path"):
        autograd.spmm_bf16(autograd.TrainableCSR.from_host(csr, device="cpu"), t.values, torch.zeros((k, 8), dtype=torch.bfloat16), sddmm="bf16")
