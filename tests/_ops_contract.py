"""The operand contract of mispmm.ops as a table ("The operand contract of the ops entry points").

The C ABI takes raw pointers, a width and a leading dimension; it cannot see a dtype, the extent of an allocation or the
length of a Python list.  What ops.py does not check, nothing checks.  So every public function of mispmm.ops that takes a
device tensor refuses, in Python and before any call into a library, with a ValueError that names the operand:

  * a wrong dtype (bf16 operands are int16 bit patterns);
  * a wrong rank or a wrong shape against the container (rows of B against A's columns, out against [M, N], ...);
  * a column stride other than 1;
  * rows that overlap themselves (an expanded tensor: row stride < N);
  * an `out` whose dtype does not fit the out_bf16 flag;
  * an unknown `acc`;
  * lists whose members differ from one another in shape, dtype or row stride -- EVERY member is looked at, not the first;
  * lists of unequal length;
  * a workspace of the wrong dtype, too few elements, or not contiguous.

Legal and kept legal: the [:rows, :N] corner of a larger buffer (row stride > N), a [1, N] operand with any row stride,
out=None, and non-contiguous input to the conversion helpers, which copy.

One Entry per function: `make(device)` builds the smallest valid call ("cpu" and "cuda" alike), `operands` says which
arguments are tensors of which kind -- the defects and the accepted views are derived from the kind, one change at a time
-- and `abi` says which values the library must be handed for a call that reaches it.  tests/test_ops_contract_cpu.py holds
the table against a recording stand-in of the libraries, tests/test_gpu_ops_contract.py against the kernels.  EXCLUDED lists
what has no row and why; a public callable of ops in neither fails the completeness test."""
import ctypes
import dataclasses
import inspect
import re
from dataclasses import dataclass, field

import numpy as np
import torch

from mispmm import formats, ops

N = 24          # columns of every dense operand: 8 <= N <= 64, no multiple of 16 ...
N_GROUPS = 64   # ... but for the two kernels that take whole 64-column (LDS tiles) or 32-column (plan order) groups only
PAD = 8         # columns a padded view's buffer has beyond N (one more row as well)


# ---------------------------------------------------------------------------------------------------------------- calls
@dataclass
class Call:
    """ops.<fn>(*args, **kwargs).  A path names one argument: (1,) = args[1], ("out",) = kwargs["out"], (1, 2) = args[1][2]."""
    fn: str
    args: list
    kwargs: dict = field(default_factory=dict)

    def run(self):
        return getattr(ops, self.fn)(*self.args, **self.kwargs)

    def _root(self, key):
        return self.args if isinstance(key, int) else self.kwargs

    def get(self, path):
        v = self._root(path[0])[path[0]]
        return v if len(path) == 1 else v[path[1]]

    def with_(self, path, value):
        """A copy of the call with one argument replaced (a list argument is copied, its other members shared)."""
        c = Call(self.fn, list(self.args), dict(self.kwargs))
        root = c._root(path[0])
        if len(path) == 1:
            root[path[0]] = value
        else:
            members = list(root[path[0]])
            members[path[1]] = value
            root[path[0]] = members
        return c

    def without(self, key):
        c = Call(self.fn, list(self.args), dict(self.kwargs))
        del c.kwargs[key]
        return c


@dataclass(frozen=True)
class Op:
    """One tensor argument.  kind: "dense" = 2-D, unit column stride, any row stride >= columns; "flat" = contiguous, of a
    fixed shape; "buffer" = contiguous, of a fixed number of elements in any shape; "perm" = an index list of a fixed number
    of elements (copied where it must be); "convert" = input of a conversion helper (any strides: it is copied);
    "convert2d" = the same, 2-D."""
    name: str                 # what the refusal must name
    path: tuple
    kind: str = "dense"
    out: bool = False         # written by the call
    flag: bool = False        # an out whose dtype the out_bf16 flag decides


@dataclass(frozen=True)
class ListOp:
    name: str
    path: tuple
    out: bool = False


@dataclass
class Entry:
    fn: str
    make: callable                       # device -> Call, deterministic
    operands: tuple = ()
    lists: tuple = ()
    acc: bool = False                    # takes acc=
    calls: int = 1                       # library calls the baseline and every accepted variant make
    abi: callable = None                 # (call, result) -> sequences of values that must stand side by side in one recorded call
    twin: callable = None                # call -> the results the call must reproduce bit for bit by OTHER entry points
    single_row: dict = field(default_factory=dict)   # name -> device -> (Call with a [1, N] operand of odd row stride, contiguous twin)


# -------------------------------------------------------------------------------------------------------- expected values
def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else 0


def ld(t):
    """The leading dimension the library must be told for a 2-D view (one row: whatever covers it)."""
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


def plain(arg):
    """A recorded ctypes argument as a Python value: pointers as integers, arrays as tuples."""
    if isinstance(arg, ctypes.Array):
        return tuple(int(v or 0) for v in arg)
    if isinstance(arg, ctypes.c_void_p):
        return int(arg.value or 0)
    if isinstance(arg, (ctypes.c_float, ctypes.c_int, ctypes.c_uint32)):
        return arg.value
    return arg


def holds(recorded_args, seq):
    """seq stands side by side somewhere in the arguments of one recorded call."""
    args = [plain(a) for a in recorded_args]
    seq = list(seq)
    return any(args[i:i + len(seq)] == seq for i in range(len(args) - len(seq) + 1))


# ---------------------------------------------------------------------------------------------------------------- defects
_OTHER = {torch.float32: torch.float64, torch.float64: torch.float32, torch.int16: torch.float32, torch.int32: torch.int16,
          torch.int64: torch.int16}
_FLAG = {torch.float32: torch.int16, torch.int16: torch.float32}


def _strided_copy(t):
    """t's shape and values with a last stride of 2."""
    return torch.stack([t, t], dim=-1)[..., 0]


DEFECTS = {
    # name -> (kinds it applies to, tensor -> defective tensor)
    "dtype": (("dense", "flat", "buffer", "perm", "convert", "convert2d"), lambda t: t.to(_OTHER[t.dtype])),
    "rank": (("dense", "flat", "convert2d"), lambda t: t[0] if t.dim() > 1 else t.unsqueeze(0)),
    "rows": (("dense",), lambda t: t[:-1]),
    "cols": (("dense-out",), lambda t: t[:, :-1]),
    "colstride": (("dense",), lambda t: t.t().contiguous().t()),
    "overlap": (("dense",), lambda t: t[:1].expand(t.shape[0], t.shape[1])),
    "flag": (("flag",), lambda t: t.to(_FLAG[t.dtype])),
    "size": (("flat", "buffer", "perm"), lambda t: t[:-1]),
    "strided": (("flat", "buffer"), _strided_copy),
}


def _kinds(op):
    return (op.kind,) + (("dense-out",) if op.out and op.kind == "dense" else ()) + (("flag",) if op.flag else ())


def defect_ids(entry):
    """Every defect of an entry as "<operand>:<defect>", known without building a tensor."""
    ids = [f"{op.name}:{d}" for op in entry.operands for d, (kinds, _) in DEFECTS.items() if set(kinds) & set(_kinds(op))]
    for lo in entry.lists:
        ids += [f"{lo.name}:{d}" for d in ("member-shape", "member-dtype", "member-rowstride")]
        if lo.out:
            ids += [f"{lo.name}:{d}" for d in ("shorter", "longer")]
    if entry.lists and not any(lo.out for lo in entry.lists):
        raise AssertionError(f"{entry.fn}: a list entry needs its list of results")
    return ids + (["acc:unknown"] if entry.acc else [])


def padded(t, factory=None):
    """(buffer, its [:rows, :N] corner holding t's values): a legal view with a row stride above N."""
    if factory is not None:
        buf, view = factory(t.shape[0], t.shape[1], PAD, t.dtype)
    else:
        buf = torch.zeros((t.shape[0] + 1, t.shape[1] + PAD), dtype=t.dtype, device=t.device)
        view = buf[:t.shape[0], :t.shape[1]]
    view.copy_(t)
    return buf, view


def defective(entry, call, ident):
    """(the call with the one defect `ident`, the operand name its refusal must hold)."""
    name, what = ident.split(":")
    if ident == "acc:unknown":
        c = Call(call.fn, list(call.args), dict(call.kwargs))
        if "acc" in c.kwargs:
            c.kwargs["acc"] = "quick"
        else:                                      # positional acc (_csr_plan)
            c.args[next(i for i, v in enumerate(c.args) if isinstance(v, str))] = "quick"
        return c, "acc"
    for lo in entry.lists:
        if lo.name != name:
            continue
        members = call.get(lo.path)
        second = members[1]
        if what == "shorter":
            return call.with_(lo.path, members[:-1]), name
        if what == "longer":
            return call.with_(lo.path, members + [members[-1].clone()]), name
        bad = {"member-shape": lambda t: t[:-1], "member-dtype": lambda t: t.to(torch.float64),
               "member-rowstride": lambda t: padded(t)[1]}[what](second)
        return call.with_(lo.path + (1,), bad), name      # the SECOND member: the first is what the old code looked at
    op = next(o for o in entry.operands if o.name == name)
    return call.with_(op.path, DEFECTS[what][1](call.get(op.path))), name


def names(message, operand):
    """The refusal speaks of the operand by its name (as a word: `b` is not named by "bits")."""
    return re.search(rf"(?<![A-Za-z0-9_]){re.escape(operand)}(?![A-Za-z0-9_])", message) is not None


# ------------------------------------------------------------------------------------------------------ accepted variants
def variant_ids(entry):
    ids = []
    for op in entry.operands:
        if op.kind == "dense":
            ids.append(f"{op.name}:padded")
        if op.kind in ("convert", "convert2d"):
            ids.append(f"{op.name}:strided")
        if op.out and op.path[0] == "out":
            ids.append("out:none")
    for lo in entry.lists:
        ids.append(f"{lo.name}:padded")
        if lo.out and isinstance(lo.path[0], str):
            ids.append(f"{lo.name}:none")
    return ids + [f"1row:{k}" for k in entry.single_row]


def variant(entry, call, ident, factory=None):
    """(the call through the legal view `ident`, {path: (buffer, rows, cols)} of the padded buffers the call writes)."""
    name, what = ident.split(":")
    if what == "none":
        return call.without(name), {}
    for lo in entry.lists:
        if lo.name == name:                          # every member the corner of a buffer of its own: one row stride for all
            pads = [padded(t, factory if lo.out else None) for t in call.get(lo.path)]
            written = {lo.path + (i,): (buf, v.shape[0], v.shape[1]) for i, (buf, v) in enumerate(pads)} if lo.out else {}
            return call.with_(lo.path, [v for _, v in pads]), written
    op = next(o for o in entry.operands if o.name == name)
    t = call.get(op.path)
    if what == "strided":
        return call.with_(op.path, _strided_copy(t)), {}
    buf, view = padded(t, factory if op.out else None)
    return call.with_(op.path, view), ({op.path: (buf, t.shape[0], t.shape[1])} if op.out else {})


def results(value):
    """The tensors a call returned, as a list."""
    if isinstance(value, torch.Tensor):
        return [value]
    return [v for v in value if v is not None] if isinstance(value, (list, tuple)) else []


def tensors(call):
    """{path: tensor} of every tensor argument of a call, list members included."""
    found = {}
    for key, v in list(enumerate(call.args)) + list(call.kwargs.items()):
        if isinstance(v, torch.Tensor):
            found[(key,)] = v
        elif isinstance(v, (list, tuple)) and v and all(isinstance(m, torch.Tensor) for m in v):
            found.update({(key, i): m for i, m in enumerate(v)})
    return found


def container_tensors(obj):
    """Names of the dataclass fields of a device container that hold a tensor."""
    return [f.name for f in dataclasses.fields(obj) if isinstance(getattr(obj, f.name), torch.Tensor)] if dataclasses.is_dataclass(obj) else []


# ------------------------------------------------------------------------------------------------------------- operands
def _rng(seed=7):
    return np.random.default_rng(seed)


def _ints(shape, seed, device, dtype=torch.float32):
    """Small integers: every product and sum of them is exact in fp32 and in bf16."""
    t = torch.from_numpy(_rng(seed).integers(-3, 4, shape).astype(np.float32))
    return (t.to(torch.bfloat16).view(torch.int16) if dtype == torch.int16 else t).to(device)


def _reals(shape, seed, device):
    return torch.from_numpy(_rng(seed).uniform(-1, 1, shape).astype(np.float32)).to(device)


def csr_host(m=37, k=29, uniform=0):
    rng = _rng(11)
    lens = np.full(m, uniform) if uniform else np.minimum(rng.integers(0, 7, m), k)
    if not uniform:
        lens[min(5, m - 1)] = 0                                       # an empty row
        lens[0] = min(3, k)
    ptrs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cols = np.concatenate([np.sort(rng.choice(k, size=int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.uint32)
    vals = rng.integers(1, 4, int(ptrs[-1])).astype(np.float32)
    return formats.CSR(m, k, ptrs, cols, vals)


def bsr_host():
    """48 x 32 in 16 x 16 blocks: block rows of 2, 0 and 1 blocks."""
    data = _rng(13).integers(-3, 4, (3, 16, 16)).astype(np.float32)
    return formats.BSR(48, 32, 3 * 256, 16, 16, np.array([0, 2, 2, 3], np.uint32), np.array([0, 1, 1], np.uint32), data)


def _product(fn, a, b_dtype=torch.float32, out_dtype=torch.float32, acc=True, n=N, **more):
    """make() of C = A @ B entry points: (container builder, ...) -> device -> Call(fn, [a, b], out=..., acc=...)."""
    def make(device):
        cont = a(device)
        b = _ints((cont.num_cols, n), 21, device, b_dtype)
        out = torch.zeros((cont.num_rows, n), dtype=out_dtype, device=device)
        kw = {"out": out, **more}
        if acc:
            kw["acc"] = "reference"
        return Call(fn, [cont, b], kw)
    return make


def _product_abi(call, result):
    b = call.args[-1] if call.fn != "spmm_bsr_bf16" else call.args[2]
    return [[ptr(b), b.shape[1], ld(b), ptr(result), ld(result)]]


B = Op("b", (1,))
B16 = Op("b_bf16", (1,))
OUT = Op("out", ("out",), out=True)
OUT_FLAG = Op("out", ("out",), out=True, flag=True)


def _one_row(fn, b_dtype, what):
    """The [1, N] operand with a row stride below N, as b (K = 1) or as out (M = 1), beside its contiguous twin."""
    def make(device):
        csr = csr_host(1, 29) if what == "out" else csr_host(37, 1)
        a = ops.DeviceCSR.from_host(csr, device=device)
        b = _ints((csr.num_cols, N), 21, device, b_dtype)
        out = torch.zeros((csr.num_rows, N), dtype=torch.float32, device=device)
        twin = Call(fn, [a, b], {"out": out, "acc": "reference"})
        t = twin.get(("out",) if what == "out" else (1,))
        odd = torch.as_strided(torch.zeros(N + 8, dtype=t.dtype, device=device), (1, N), (5, 1))
        odd.copy_(t)
        return twin.with_(("out",) if what == "out" else (1,), odd), twin
    return make


def _batch(device, plan=False, n=N):
    csr = csr_host()
    a = ops.DeviceCSR.from_host(csr, device=device, plan=plan)
    bs = [_ints((csr.num_cols, n), 30 + i, device) for i in range(3)]
    outs = [torch.zeros((csr.num_rows, n), dtype=torch.float32, device=device) for _ in bs]
    return a, bs, outs


def _make_batch(device):
    a, bs, outs = _batch(device)
    return Call("spmm_csr_batch", [a, bs], {"outs": outs, "acc": "reference"})


def _make_plan(device):
    a, bs, outs = _batch(device, plan=True, n=N_GROUPS)
    return Call("_csr_plan", [a, bs, outs, "reference", None])


def _batch_abi(call, result):
    bs = call.args[1]
    cs = call.args[2] if call.fn == "_csr_plan" else result
    return [[len(bs), tuple(ptr(b) for b in bs), bs[0].shape[1], ld(bs[0]), tuple(ptr(c) for c in cs), ld(cs[0])]]


def _batch_twin(call):
    """One spmm_csr per operand, without hints: the general entry point."""
    return [ops.spmm_csr(call.args[0], b, use_hint=False) for b in call.args[1]]


def _make_sddmm(device):
    csr = csr_host()
    a = ops.DeviceCSR.from_host(csr, device=device)
    return Call("sddmm_csr", [a, _ints((csr.num_rows, N), 40, device), _ints((csr.num_cols, N), 41, device)],
                {"out": torch.zeros(csr.nnz, dtype=torch.float32, device=device), "acc": "reference"})


def _make_softmax(device):
    csr = csr_host()
    a = ops.DeviceCSR.from_host(csr, device=device)
    return Call("softmax_csr", [a, _reals(csr.nnz, 42, device)], {"out": torch.zeros(csr.nnz, dtype=torch.float32, device=device), "acc": "reference"})


def _make_softmax_bwd(device):
    csr = csr_host()
    a = ops.DeviceCSR.from_host(csr, device=device)
    return Call("softmax_csr_bwd", [a, _reals(csr.nnz, 43, device).abs(), _reals(csr.nnz, 44, device)],
                {"out": torch.zeros(csr.nnz, dtype=torch.float32, device=device), "acc": "reference"})


D, DV = 8, 16


def _make_attn_csr(device):
    csr = csr_host()
    a = ops.DeviceCSR.from_host(csr, device=device)
    m, k = csr.num_rows, csr.num_cols
    return Call("attention_csr", [a, _reals((m, D), 50, device), _reals((k, D), 51, device), _reals((k, DV), 52, device)],
                {"bias": _reals(csr.nnz, 53, device), "return_lse": True, "out": torch.zeros((m, DV), dtype=torch.float32, device=device),
                 "lse": torch.zeros(m, dtype=torch.float32, device=device)})


def _make_attn_csr_bwd(device):
    csr = csr_host()
    t, perm = ops.csr_transpose(csr)
    a, at = ops.DeviceCSR.from_host(csr, device=device), ops.DeviceCSR.from_host(t, device=device)
    m, k = csr.num_rows, csr.num_cols
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)   # noqa: E731
    return Call("attention_csr_bwd", [a, at, torch.from_numpy(perm.astype(np.int32)).to(device), _reals((m, D), 50, device), _reals((k, D), 51, device),
                                      _reals((k, DV), 52, device), _reals((m, DV), 54, device), _reals(m, 55, device), _reals((m, DV), 56, device)],
                {"bias": _reals(csr.nnz, 53, device), "dq": z(m, D), "dk": z(k, D), "dv": z(k, DV), "delta": z(m)})


def _attn_csr_abi(call, result):
    q, k, v = call.args[1:4] if call.fn == "attention_csr" else call.args[3:6]
    seqs = [[ptr(q), 0, ld(q)], [ptr(k), 0, ld(k), D], [ptr(v), 0, ld(v), DV]]
    if call.fn == "attention_csr":
        out = call.kwargs.get("out", result[0])
        return seqs + [[ptr(out), 0, ld(out), ptr(call.kwargs["lse"])]]
    out, lse, g = call.args[6:9]
    dq, dk, dv = (call.kwargs[n] for n in ("dq", "dk", "dv"))
    return seqs + [[ptr(out), 0, ld(out), ptr(lse), ptr(g), 0, ld(g), ptr(call.kwargs["delta"]), ptr(dq), 0, ld(dq), ptr(dk), 0, ld(dk), ptr(dv), 0, ld(dv)]]


def _bsr_dev(device):
    return ops.DeviceBSR.from_host(bsr_host(), device=device)


def _blocks_bits(device):
    return torch.from_numpy(bsr_host().data).to(torch.bfloat16).view(torch.int16).to(device)


def _make_bsr_bf16(device):
    a = _bsr_dev(device)
    return Call("spmm_bsr_bf16", [a, _blocks_bits(device), _ints((a.num_cols, N), 21, device, torch.int16)],
                {"out_bf16": False, "out": torch.zeros((a.num_rows, N), dtype=torch.float32, device=device)})


def _make_sddmm_bsr(device):
    a = _bsr_dev(device)
    return Call("sddmm_bsr_bf16", [a, _ints((a.num_rows, N), 60, device, torch.int16), _ints((a.num_cols, N), 61, device, torch.int16)],
                {"out_bf16": False, "out": torch.zeros((a.num_blocks, 16, 16), dtype=torch.float32, device=device)})


def _make_softmax_bsr(device):
    a = _bsr_dev(device)
    return Call("softmax_bsr", [a, _reals((a.num_blocks, 16, 16), 62, device)],
                {"mask": _reals((a.num_blocks, 16, 16), 63, device), "out_bf16": False, "out": torch.zeros((a.num_blocks, 16, 16), dtype=torch.float32, device=device)})


def _make_softmax_bsr_bwd(device):
    a = _bsr_dev(device)
    return Call("softmax_bsr_bwd", [a, _reals((a.num_blocks, 16, 16), 64, device).abs(), _reals((a.num_blocks, 16, 16), 65, device)],
                {"out_bf16": False, "out": torch.zeros((a.num_blocks, 16, 16), dtype=torch.float32, device=device)})


def _bits(shape, seed, device):
    return _reals(shape, seed, device).to(torch.bfloat16).view(torch.int16)


def _make_attn_bsr(device):
    a = _bsr_dev(device)
    m, k = a.num_rows, a.num_cols
    return Call("attention_bsr_bf16", [a, _bits((m, D), 70, device), _bits((k, D), 71, device), _bits((k, DV), 72, device)],
                {"mask": _reals((a.num_blocks, 16, 16), 73, device), "out_bf16": False, "return_lse": True,
                 "out": torch.zeros((m, DV), dtype=torch.float32, device=device), "lse": torch.zeros(m, dtype=torch.float32, device=device)})


def _make_attn_bsr_bwd(device):
    host = bsr_host()
    t, perm = ops.bsr_transpose(host)
    a, at = ops.DeviceBSR.from_host(host, device=device), ops.DeviceBSR.from_host(t, device=device)
    m, k = a.num_rows, a.num_cols
    z = lambda *shape: torch.zeros(shape, dtype=torch.int16, device=device)   # noqa: E731
    return Call("attention_bsr_bwd_bf16", [a, at, torch.from_numpy(perm.astype(np.int32)).to(device), _bits((m, D), 70, device), _bits((k, D), 71, device),
                                           _bits((k, DV), 72, device), _reals((m, DV), 74, device), _reals(m, 75, device), _bits((m, DV), 76, device)],
                {"mask": _reals((a.num_blocks, 16, 16), 73, device), "dq": z(m, D), "dk": z(k, D), "dv": z(k, DV),
                 "delta": torch.zeros(m, dtype=torch.float32, device=device)})


def _attn_bsr_abi(call, result):
    if call.fn == "attention_bsr_bf16":
        q, k, v = call.args[1:4]
        out = call.kwargs.get("out", result[0])
        return [[ptr(q), ld(q), 0, ptr(k), ld(k), 0, ptr(v), ld(v), 0, D, DV, ptr(call.kwargs["mask"])], [ptr(out), ld(out), 0, 0, ptr(call.kwargs["lse"])]]
    q, k, v, out, lse, g = call.args[3:9]
    dq, dk, dv = (call.kwargs[n] for n in ("dq", "dk", "dv"))
    return [[ptr(q), ld(q), 0, ptr(k), ld(k), 0, ptr(v), ld(v), 0, ptr(g), ld(g), 0, ptr(out), ld(out), 0, 0, ptr(lse), ptr(call.kwargs["delta"]), D, DV],
            [ptr(dq), ld(dq), 0, ptr(dk), ld(dk), 0, ptr(dv), ld(dv), 0, 1]]


def _make_coo(device):
    csr = csr_host()
    a = ops.DeviceCOO.from_host(formats.csr_to_coo(csr), device=device)
    call = _product("spmm_coo", lambda d: a)(device)
    call.kwargs["workspace"] = torch.zeros(csr.num_rows + 1, dtype=torch.int32, device=device)
    return call


def _make_bounds(device):
    return Call("coo_row_bounds", [ops.DeviceCOO.from_host(formats.csr_to_coo(csr_host()), device=device)])


def _make_use_plan(device):
    return Call("use_plan", [ops.DeviceCSR.from_host(csr_host(), device=device, plan=True), N], {"acc": "reference"})


def _convert(fn, dtype):
    return lambda device: Call(fn, [_ints((19, N), 80, device, dtype)])


_csr = lambda **kw: (lambda device: ops.DeviceCSR.from_host(csr_host(), device=device, **kw))                       # noqa: E731
_ell = lambda device: ops.DeviceELL.from_host(formats.csr_to_ell_colmajor(csr_host()), device=device)              # noqa: E731
_coo = lambda device: ops.DeviceCOO.from_host(formats.csr_to_coo(csr_host()), device=device)                       # noqa: E731
_flat = lambda name, path, out=False, flag=False, kind="flat": Op(name, path, kind, out, flag)                     # noqa: E731
_QKV = (Op("q", (1,)), Op("k", (2,)), Op("v", (3,)))
_QKV_BWD = (Op("q", (3,)), Op("k", (4,)), Op("v", (5,)), Op("out", (6,)), _flat("lse", (7,)), Op("grad_out", (8,)),
            Op("dq", ("dq",), out=True), Op("dk", ("dk",), out=True), Op("dv", ("dv",), out=True), _flat("delta", ("delta",), out=True))

TABLE = {e.fn: e for e in (
    Entry("spmm_csr", _product("spmm_csr", _csr()), (B, OUT), acc=True, abi=_product_abi,
          single_row={"b": _one_row("spmm_csr", torch.float32, "b"), "out": _one_row("spmm_csr", torch.float32, "out")}),
    Entry("spmm_csr_batch", _make_batch, lists=(ListOp("bs", (1,)), ListOp("outs", ("outs",), out=True)), acc=True, abi=_batch_abi, twin=_batch_twin),
    Entry("_csr_plan", _make_plan, lists=(ListOp("bs", (1,)), ListOp("cs", (2,), out=True)), acc=True, abi=_batch_abi, twin=_batch_twin),
    Entry("use_plan", _make_use_plan, acc=True),
    Entry("spmm_csr_tiles", _product("spmm_csr_tiles", lambda d: ops.DeviceCSRTiles.from_host(csr_host(uniform=3), device=d), n=N_GROUPS), (B, OUT), acc=True, abi=_product_abi),
    Entry("spmm_csr_panels", _product("spmm_csr_panels", lambda d: ops.DeviceCSRPanels.from_host(csr_host(), device=d)), (B, OUT), acc=True, abi=_product_abi),
    Entry("spmm_ell", _product("spmm_ell", _ell), (B, OUT), acc=True, abi=_product_abi),
    Entry("spmm_bsr", _product("spmm_bsr", _bsr_dev), (B, OUT), acc=True, abi=_product_abi),
    Entry("spmm_bsr_nonzeros", _product("spmm_bsr_nonzeros", lambda d: ops.bsr_nonzeros(bsr_host(), device=d)), (B, OUT), acc=True, abi=_product_abi),
    Entry("spmm_coo", _make_coo, (B, OUT, _flat("workspace", ("workspace",), out=True, kind="buffer")), acc=True, abi=_product_abi),
    Entry("coo_row_bounds", _make_bounds),
    Entry("sddmm_csr", _make_sddmm, (Op("x", (1,)), Op("y", (2,)), _flat("out", ("out",), out=True)), acc=True,
          abi=lambda c, r: [[ptr(c.args[1]), ld(c.args[1]), ptr(c.args[2]), ld(c.args[2]), N, ptr(r)]]),
    Entry("softmax_csr", _make_softmax, (_flat("scores", (1,)), _flat("out", ("out",), out=True)), acc=True, abi=lambda c, r: [[ptr(c.args[1]), ptr(r)]]),
    Entry("softmax_csr_bwd", _make_softmax_bwd, (_flat("p", (1,)), _flat("dp", (2,)), _flat("out", ("out",), out=True)), acc=True,
          abi=lambda c, r: [[ptr(c.args[1]), ptr(c.args[2]), ptr(r)]]),
    Entry("attention_csr", _make_attn_csr, _QKV + (_flat("bias", ("bias",), kind="buffer"), Op("out", ("out",), out=True), _flat("lse", ("lse",), out=True)), abi=_attn_csr_abi),
    Entry("attention_csr_bwd", _make_attn_csr_bwd, (_flat("perm", (2,), kind="perm"),) + _QKV_BWD + (_flat("bias", ("bias",), kind="buffer"),), abi=_attn_csr_abi),
    Entry("f32_to_bf16", _convert("f32_to_bf16", torch.float32), (Op("x", (0,), "convert"),), abi=lambda c, r: [[c.args[0].numel()], [ptr(r)]]),
    Entry("bf16_to_f32", _convert("bf16_to_f32", torch.int16), (Op("x", (0,), "convert"),), abi=lambda c, r: [[c.args[0].numel()], [ptr(r)]]),
    Entry("dense_transpose", _convert("dense_transpose", torch.float32), (Op("x", (0,), "convert2d"),), abi=lambda c, r: [[19, N], [ptr(r)]]),
    Entry("spmm_bsr_bf16", _make_bsr_bf16, (_flat("blocks_bf16", (1,), kind="buffer"), Op("b_bf16", (2,)), OUT_FLAG), abi=_product_abi),
    Entry("spmm_bsrc_bf16", _product("spmm_bsrc_bf16", lambda d: ops.DeviceBSRC.from_host(bsr_host(), device=d), torch.int16, acc=False, out_bf16=False),
          (B16, OUT_FLAG), abi=_product_abi),
    Entry("spmm_bsrc_slots_bf16", _product("spmm_bsrc_slots_bf16", lambda d: ops.DeviceBSRCSlots.from_host(bsr_host(), device=d), torch.int16, acc=False,
                                            out_bf16=False), (B16, OUT_FLAG), abi=_product_abi),
    Entry("sddmm_bsr_bf16", _make_sddmm_bsr, (Op("x_bf16", (1,)), Op("y_bf16", (2,)), _flat("out", ("out",), out=True, flag=True)),
          abi=lambda c, r: [[ptr(c.args[1]), ld(c.args[1]), ptr(c.args[2]), ld(c.args[2]), N, ptr(r), 0]]),
    Entry("softmax_bsr", _make_softmax_bsr, (_flat("scores", (1,)), _flat("mask", ("mask",)), _flat("out", ("out",), out=True, flag=True)),
          abi=lambda c, r: [[ptr(c.args[1]), ptr(c.kwargs["mask"]), 1.0, ptr(r), 0]]),
    Entry("softmax_bsr_bwd", _make_softmax_bsr_bwd, (_flat("p", (1,)), _flat("dp", (2,)), _flat("out", ("out",), out=True, flag=True)),
          abi=lambda c, r: [[ptr(c.args[1]), 0, ptr(c.args[2]), 1.0, ptr(r), 0]]),
    Entry("attention_bsr_bf16", _make_attn_bsr, _QKV + (_flat("mask", ("mask",)), Op("out", ("out",), out=True, flag=True), _flat("lse", ("lse",), out=True)),
          abi=_attn_bsr_abi),
    Entry("attention_bsr_bwd_bf16", _make_attn_bsr_bwd, (_flat("perm", (2,), kind="perm"),) + _QKV_BWD + (_flat("mask", ("mask",)),), abi=_attn_bsr_abi),
    Entry("spmm_csr_bf16", _product("spmm_csr_bf16", _csr(), torch.int16, out_bf16=False), (B16, OUT_FLAG), acc=True, abi=_product_abi,
          single_row={"b_bf16": _one_row("spmm_csr_bf16", torch.int16, "b"), "out": _one_row("spmm_csr_bf16", torch.int16, "out")}),
    Entry("spmm_coo_bf16", _product("spmm_coo_bf16", _coo, torch.int16, out_bf16=False), (B16, OUT_FLAG), acc=True, calls=2, abi=_product_abi),
    Entry("spmm_ell_bf16", _product("spmm_ell_bf16", _ell, torch.int16, out_bf16=False), (B16, OUT_FLAG), acc=True, abi=_product_abi),
)}

# What has no row, and why.  A public callable of mispmm.ops that is in neither TABLE nor EXCLUDED fails the completeness test.
_HOST = "host-only helper: numpy arrays and host containers in, no device tensor"
_CONTAINER = "container class: holds the tensors its from_host uploads, takes none from a caller"
EXCLUDED = {
    **{name: _HOST for name in ("check_host", "uniform_row_nnz", "csr_spans_by_length", "wants_spans", "spans_long_count", "cluster_rows", "permute_rows",
                                "plan_pays", "autotune_pick", "csr_transpose", "bsr_transpose", "colmajor_ell_to_rowmajor", "ell_rows_f64",
                                "bsr_nonzeros_f64_host", "shard_rows_by_nnz")},
    "bsr_nonzeros": "upload step: a host BSR in, a DeviceCSR out, no device tensor taken",
    **{name: _CONTAINER for name in ("CsrPlan", "DeviceCSR", "DeviceELL", "DeviceBSR", "RowSpans", "DeviceCOO", "DeviceCSRTiles", "DeviceCSRPanels",
                                     "DeviceBSRC", "DeviceBSRCSlots")},
}
# Private helpers have no rows of their own, except _csr_plan, which tests and tools call directly: they are reached through the
# public entry points above, whose rows cover them.


def public_callables():
    """Names of the functions and classes mispmm.ops defines itself and exports (no leading underscore)."""
    return sorted(name for name, obj in vars(ops).items()
                  if not name.startswith("_") and (inspect.isfunction(obj) or inspect.isclass(obj)) and obj.__module__ == ops.__name__)


def uncovered(table=None):
    """Public callables of ops that are neither in the table nor excluded -- plus _csr_plan if its row is gone."""
    table = TABLE if table is None else table
    return [name for name in public_callables() + ["_csr_plan"] if name not in table and name not in EXCLUDED]

