"""The operand contract of mispmm.ops (tests/_ops_contract.py) on the GPU.

Defects run behind a guard: every library is wrapped in a proxy that lets the host helpers and the two status readers
through and raises AssertionError the moment a compute entry point is looked up.  A missing check therefore shows as a
failed assertion and never as a launch on a bad operand.  Held: ValueError, the kernel tag unchanged, every tensor the call
would have written still full of the sentinel.

Accepted views run for real: the result through a padded or strided view is, bit for bit, that of the same call on
contiguous operands (spmm_csr_batch and _csr_plan: of one spmm_csr per operand), and the gap and the tail of every padded
buffer the call writes keep their sentinel."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from mispmm import capi, capi_attn, capi_attn_bwd, capi_attn_csr, capi_attn_csr_bwd, capi_bf16  # noqa: E402

import _ops_contract as oc  # noqa: E402
from test_gpu_census import _SENTINEL, assert_sentinel, sentinel_out  # noqa: E402

pytestmark = pytest.mark.gpu

SIDE = (capi_attn, capi_attn_bwd, capi_attn_csr, capi_attn_csr_bwd, capi_bf16)
PASSED_ON = {"mispmm_last_kernel", "mispmm_last_error", "mispmm_status_string", "mispmm_version", "mispmm_csr_panel_rows"}
FILL = {**_SENTINEL, torch.int32: (torch.int32, 0x7FC0DEAD)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs a GPU"
    capi.lib()


class Guard:
    """A library of which only the host helpers and the status readers can be reached."""
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name.endswith("_host") or name in PASSED_ON:
            return getattr(self._real, name)
        raise AssertionError(f"{name} was looked up: a defective operand got as far as a compute entry point")


@pytest.fixture
def guard(monkeypatch):
    """install(): from here on no compute entry point of any library can be reached."""
    def install():
        for module in (capi,) + SIDE:
            monkeypatch.setattr(module, "lib", lambda real=Guard(module.lib()): real)
    return install


def _written(entry, call):
    """The tensors a call would write: every operand the table marks as written, list members one by one."""
    found = [call.get(op.path) for op in entry.operands if op.out]
    for lo in entry.lists:
        if lo.out:
            found += list(call.get(lo.path))
    return found


def _fill(t):
    as_int, bits = FILL[t.dtype]
    t.view(as_int).fill_(bits)


def _is_full(t):
    as_int, bits = FILL[t.dtype]
    return bool((t.view(as_int) == bits).all())


def _bits(t):
    """A tensor's elements as integers on the host, NaN payloads included."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()]).cpu().numpy()


DEFECTS = [(fn, ident) for fn, e in oc.TABLE.items() for ident in oc.defect_ids(e)]
VARIANTS = [(fn, ident) for fn, e in oc.TABLE.items() for ident in oc.variant_ids(e)]


@pytest.mark.parametrize("fn,ident", DEFECTS, ids=[f"{fn}-{i}" for fn, i in DEFECTS])
def test_defect_is_refused_and_nothing_is_launched(fn, ident, guard):
    entry = oc.TABLE[fn]
    base = entry.make("cuda")
    for t in _written(entry, base):
        _fill(t)
    call, operand = oc.defective(entry, base, ident)
    before = [(t, _bits(t)) for t in _written(entry, call) if isinstance(t, torch.Tensor)]
    tag = capi.last_kernel()
    guard()
    with pytest.raises(ValueError) as err:
        call.run()
    assert oc.names(str(err.value), operand), f"the refusal does not name {operand!r}: {err.value}"
    assert capi.last_kernel() == tag
    torch.cuda.synchronize()
    for t in _written(entry, base):
        assert _is_full(t), "a tensor the refused call was given has been written"
    for t, was in before:
        assert np.array_equal(_bits(t), was), "a tensor the refused call was given has been written"


def _outputs(entry, call, value):
    got = oc.results(value)
    if got:
        return got
    assert value is True, f"{entry.fn} answered {value!r}"          # _csr_plan: True = the shape was taken
    return [t for lo in entry.lists if lo.out for t in call.get(lo.path)]


@pytest.mark.parametrize("fn,ident", VARIANTS, ids=[f"{fn}-{i}" for fn, i in VARIANTS])
def test_legal_view_gives_the_bits_of_the_contiguous_call(fn, ident):
    entry = oc.TABLE[fn]
    if ident.startswith("1row:"):
        call, twin = entry.single_row[ident[5:]]("cuda")
        want = [t.clone() for t in _outputs(entry, twin, twin.run())]
        twin.kwargs["out"].zero_()                   # the two calls may share it
        written = {}
    else:
        twin = entry.make("cuda")
        want = entry.twin(twin) if entry.twin else [t.clone() for t in _outputs(entry, twin, twin.run())]
        call, written = oc.variant(entry, entry.make("cuda"), ident, factory=sentinel_out)
    got = _outputs(entry, call, call.run())
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (i, g.shape, w.shape, g.dtype, w.dtype)
        differ = int((_bits(g) != _bits(w)).sum())
        assert differ == 0, f"{fn} {ident}: result {i} differs from the contiguous call in {differ} of {w.numel()} elements"
    for path, (buf, rows, cols) in written.items():
        assert_sentinel(buf, rows, cols, f"{fn} {ident} {path}")
