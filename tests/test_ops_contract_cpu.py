"""The operand contract of mispmm.ops (tests/_ops_contract.py), proven without a GPU: the libraries are replaced by a recorder
whose every function logs (name, arguments) and returns 0, the device check by a no-op.  A defective operand must raise a
ValueError that names it BEFORE the recorder sees a call; a legal call must reach the library with the width, the leading
dimensions, the batch count and the pointers the table computes from the tensors."""
import dataclasses
import inspect

import pytest

torch = pytest.importorskip("torch")
from mispmm import capi, capi_attn, capi_attn_bwd, capi_attn_csr, capi_attn_csr_bwd, capi_bf16, ops  # noqa: E402

import _ops_contract as oc  # noqa: E402

SIDE = (capi_attn, capi_attn_bwd, capi_attn_csr, capi_attn_csr_bwd, capi_bf16)


class Recorder:
    """Stands in for every library: any attribute is a function that logs its call and answers 0 (OK)."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


class Stream:
    cuda_stream = 0


class OnDevice:
    """A CPU tensor that says it lives on the device, so that ONE operand can be the CPU tensor among device tensors."""
    is_cuda = True

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return getattr(self._t, name)


@pytest.fixture(scope="module", autouse=True)
def _library():
    capi.lib()                                   # the host helpers the builders use are the real ones: raises if not built


@pytest.fixture
def recorder(monkeypatch):
    """A recorder whose install() puts it in place of every library -- after the operands are built, which takes the real
    library's host helpers."""
    rec = Recorder()

    def install():
        monkeypatch.setattr(ops, "PLAN_MIN_N", None)         # the measurement aids of the environment do not decide the call count
        monkeypatch.setattr(ops, "AUTOTUNE", True)
        monkeypatch.setattr(capi, "lib", lambda: rec)
        monkeypatch.setattr(capi, "check", lambda status: None)
        for side in SIDE:
            monkeypatch.setattr(side, "lib", lambda: rec)
            monkeypatch.setattr(side, "check", lambda status: None)
    rec.install = install
    return rec


@pytest.fixture
def no_device_check(monkeypatch):
    monkeypatch.setattr(ops, "_require_gpu", lambda *tensors: None)


def _with_stream(call):
    if call.fn == "_csr_plan":
        call.args[4] = Stream()
    else:
        call.kwargs["stream"] = Stream()
    return call


def _baseline(entry):
    """The entry's smallest valid call on CPU tensors -- built with the real library's host helpers, before the recorder."""
    return _with_stream(entry.make("cpu"))


DEFECTS = [(fn, ident) for fn, e in oc.TABLE.items() for ident in oc.defect_ids(e)]
VARIANTS = [(fn, ident) for fn, e in oc.TABLE.items() for ident in ["baseline"] + oc.variant_ids(e)]


def test_every_public_callable_has_a_row_or_a_reason():
    missing = oc.uncovered()
    assert not missing, f"no row in tests/_ops_contract.py and no reason in its EXCLUDED: {missing}"
    stale = [name for name in list(oc.TABLE) + list(oc.EXCLUDED) if not hasattr(ops, name)]
    assert not stale, f"rows or exclusions for names ops no longer has: {stale}"
    both = sorted(set(oc.TABLE) & set(oc.EXCLUDED))
    assert not both, f"in the table and excluded: {both}"


def test_a_missing_row_is_noticed():
    """The completeness check bites: without its row a function is named."""
    for gone in ("spmm_bsr_bf16", "_csr_plan"):
        assert oc.uncovered({k: v for k, v in oc.TABLE.items() if k != gone}) == [gone]


def test_every_entry_has_the_rows_the_contract_asks_for():
    for fn, e in oc.TABLE.items():
        ids = oc.defect_ids(e)
        for op in e.operands:
            assert f"{op.name}:dtype" in ids, (fn, op.name)
            if op.kind == "dense":
                assert {f"{op.name}:{d}" for d in ("rank", "rows", "colstride", "overlap")} <= set(ids), (fn, op.name)
        if "acc" in inspect.signature(getattr(ops, fn)).parameters:
            assert e.acc and "acc:unknown" in ids, fn
        for lo in e.lists:
            assert {f"{lo.name}:{d}" for d in ("member-shape", "member-dtype", "member-rowstride")} <= set(ids), (fn, lo.name)


@pytest.mark.parametrize("fn,ident", DEFECTS, ids=[f"{fn}-{i}" for fn, i in DEFECTS])
def test_defect_is_refused_before_any_call(fn, ident, recorder, no_device_check):
    entry = oc.TABLE[fn]
    call, operand = oc.defective(entry, _baseline(entry), ident)
    recorder.install()
    with pytest.raises(ValueError) as err:
        call.run()
    assert oc.names(str(err.value), operand), f"the refusal does not name {operand!r}: {err.value}"
    assert recorder.calls == [], f"{[c[0] for c in recorder.calls]} reached before the refusal"


@pytest.mark.parametrize("fn,ident", VARIANTS, ids=[f"{fn}-{i}" for fn, i in VARIANTS])
def test_legal_call_reaches_the_library_as_the_table_says(fn, ident, recorder, no_device_check):
    entry = oc.TABLE[fn]
    if ident.startswith("1row:"):
        call = _with_stream(entry.single_row[ident[5:]]("cpu")[0])
    else:
        call = _baseline(entry)
        if ident != "baseline":
            call = oc.variant(entry, call, ident)[0]
    recorder.install()
    result = call.run()
    assert len(recorder.calls) == entry.calls, [c[0] for c in recorder.calls]
    if entry.abi is None:
        return
    name, args = recorder.calls[-1]
    for seq in entry.abi(call, result):
        assert oc.holds(args, seq), f"{name} was not handed {seq} side by side: {[oc.plain(a) for a in args]}"


def _on_device(call):
    """The call with every tensor, the containers' own included, saying it is on the device."""
    for i, a in enumerate(call.args):
        fields = oc.container_tensors(a)
        if fields:
            call.args[i] = dataclasses.replace(a, **{f: OnDevice(getattr(a, f)) for f in fields})
    for path, t in oc.tensors(call).items():
        call = call.with_(path, OnDevice(t))
    return call


POSITIONS = [(fn, path) for fn, e in oc.TABLE.items() for path in oc.tensors(e.make("cpu"))]


@pytest.mark.parametrize("fn,path", POSITIONS, ids=[f"{fn}-{'.'.join(map(str, p))}" for fn, p in POSITIONS])
def test_cpu_tensor_is_refused_in_every_position(fn, path, recorder):
    entry = oc.TABLE[fn]
    plain = _baseline(entry)
    call = _on_device(plain).with_(path, plain.get(path))
    recorder.install()
    with pytest.raises(ValueError, match="no CPU path"):
        call.run()
    assert recorder.calls == []
