"""Every numerical check the GPU suite applies to an output of the two fused attention kernels, as a function of (got, case): the
GPU tests (tests/test_gpu_attn_fused.py, tests/test_gpu_attn_fused_bwd.py, tests/test_gpu_attn_tight.py) hand them what the
kernels wrote, the CPU harness (tests/test_attn_mutants_cpu.py) what the numpy restatements give, with and without a deliberate
fault -- the very same code holds both.

case: a Case -- pattern, widths, mask kind, where the operands come from, the types of out and of the gradients.
got:  a dict of host arrays, bf16 outputs widened to float32: `out`, `lse` (forward); `out`, `lse` as the backward read them and
      `dq`, `dk`, `dv` (backward); `subsets`: {need: (dq, dk, dv)} for the subset check.
A check returns None where it does not apply to the case, else (ok, worst) with ok exactly what the assertion it restates
asserts and worst the figure that assertion's test prints (worst |err| / tolerance)."""
import dataclasses
import functools

import numpy as np

import _attn_fused_bwd_ref as bwd_ref
import _attn_fused_ref as fwd_ref


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    d: int
    dv: int
    kind: str = "none"             # none | causal | leading | blankcols (backward: -Inf over every block of every second block column)
    src: str = "fwd"               # whose operands: tests/_attn_fused_ref.py (four patterns) or tests/_attn_fused_bwd_ref.py (six)
    out_bf16: bool = False
    grads_bf16: bool = False
    g32: bool = False              # grad_out with all 24 significant bits, rounded to bf16 by the Python layer
    const_v: float = 0.0           # != 0: V holds this value everywhere
    wide: int = 1                  # Q times this power of two: scores spread past the overflow of exp; S is no longer exact
    scale: float = 0.0             # 0: d ** -0.5

    @property
    def id(self):
        extra = "".join(f",{n}" for n, on in (("obf16", self.out_bf16), ("gbf16", self.grads_bf16), ("g32", self.g32),
                                                (f"v={self.const_v}", self.const_v), (f"wide{self.wide}", self.wide != 1),
                                                (f"scale={self.scale}", self.scale)) if on)
        return f"{self.src}:{self.name},D{self.d},Dv{self.dv},{self.kind}{extra}"

    @property
    def bsr(self):
        return bwd_ref.bwd_pattern(self.name)[0]

    @property
    def scale_value(self):
        return self.scale or self.d ** -0.5

    @property
    def mask(self):
        return _mask(self.name, self.kind)

    @property
    def arrays(self):
        """(q, k, v, g) float32 host arrays of one head; q, k, v hold bf16 numbers, g too unless g32.  Read-only."""
        return _arrays(self.src, self.name, self.d, self.dv, self.g32, self.const_v, self.wide)

    @property
    def g_bf16(self):
        """grad_out as the kernel gets it."""
        return bwd_ref.bf16_round(self.arrays[3])


@functools.lru_cache(maxsize=None)
def _mask(name, kind):
    if kind != "blankcols":
        return bwd_ref.mask_of(name, kind)
    bsr, tbsr, _ = bwd_ref.bwd_pattern(name)
    return blank_columns_mask(bsr, tbsr)[0]


def blank_columns_mask(bsr, tbsr):
    """(mask, blank): -Inf over every block of every second non-empty block column; every block row keeps one block.  blank: per
    block column."""
    bs = bsr.block_row_size
    counts = np.diff(np.asarray(tbsr.block_row_ptrs, dtype=np.int64))
    cols_of = np.asarray(bsr.block_col_idxs, dtype=np.int64)
    ptrs = np.asarray(bsr.block_row_ptrs, dtype=np.int64)
    blank = np.zeros(counts.shape[0], bool)
    blank[np.argwhere(counts > 0).ravel()[::2]] = True
    for lo, hi in zip(ptrs[:-1], ptrs[1:]):                        # a block row must keep one block: unblank its last column if need be
        if hi > lo and blank[cols_of[lo:hi]].all():
            blank[cols_of[hi - 1]] = False
    assert blank.any()
    m = np.zeros((bsr.num_blocks, bs, bs), np.float32)
    m[blank[cols_of]] = -np.inf
    return m, blank


@functools.lru_cache(maxsize=None)
def _arrays(src, name, d, dv, g32, const_v, wide):
    if src == "fwd":
        q, k, v = (x[0] for x in fwd_ref.operands(name, d, dv))
        g = np.zeros((q.shape[0], dv), np.float32)
    else:
        q, k, v, g = (x[0] for x in bwd_ref.operands(name, d, dv))
    if g32:
        rng = np.random.default_rng(91)
        g = (np.where(rng.random(g.shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, g.shape)).astype(np.float32)
        assert (g.view(np.uint32) & 0xFFFF).any()
    if const_v:
        v = np.full(v.shape, const_v, np.float32)
    if wide != 1:
        q = q * np.float32(wide)
    for x in (q, k, v, g):
        x.setflags(write=False)
    return q, k, v, g


def empty_block_rows(bsr):
    return np.repeat(np.diff(np.asarray(bsr.block_row_ptrs, dtype=np.int64)) == 0, bsr.block_row_size)


def _worst(err, tol):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(err / tol, initial=0.0))


# ---- the forward's checks
@functools.lru_cache(maxsize=None)
def forward_reference(case):
    """(float64 out, {out_bf16: tolerance}, exact lse, its tolerance): float64 dense masked attention, the `out` component of
    tests/test_gpu_softmax_bsr.py::_attention_tolerances, tests/_attn_fused_ref.py::lse_reference.  Keyed on the case without its
    out type; read-only."""
    from test_gpu_softmax_bsr import _attention_tolerances, _dense_attention
    assert not case.out_bf16 and case.src == "fwd"
    q, k, v, _ = case.arrays
    g = np.zeros((q.shape[0], case.dv), np.float32)
    want = _dense_attention(case.bsr, q, k, v, g, case.scale_value, case.mask)[0]
    tols = {ob: _attention_tolerances(case.name, q, k, v, g, case.scale_value, case.mask, ob)[0] for ob in (False, True)}
    return (want, tols) + fwd_ref.lse_reference(case.name, q, k, case.mask, case.scale_value)


def out_composed(got, case):
    """out against float64 dense masked attention inside the composed tolerance of the three-launch chain."""
    if case.src != "fwd" or case.const_v:
        return None
    want, tols, _, _ = forward_reference(dataclasses.replace(case, out_bf16=False))
    err = np.abs(got["out"].astype(np.float64) - want)
    return bool(np.all(err <= tols[case.out_bf16])), _worst(err, tols[case.out_bf16])


def lse_bound(got, case):
    """lse = -Inf exactly on the empty block rows, elsewhere inside the bound of tests/_attn_fused_ref.py against float64 logsumexp."""
    if case.src != "fwd" or case.const_v:
        return None
    _, _, exact, tol = forward_reference(dataclasses.replace(case, out_bf16=False))
    empty = empty_block_rows(case.bsr)
    lse = got["lse"]
    err = np.abs(lse[~empty].astype(np.float64) - exact[~empty])
    return bool(np.array_equal(np.isneginf(lse), empty) and np.all(err <= tol[~empty])), _worst(err, tol[~empty])


def forward_zero_rows(got, case):
    """An empty block row: +0 bits in its rows of out (a bf16 out widened to float32 keeps them)."""
    empty = empty_block_rows(case.bsr)
    if not empty.any() or "dq" in got:
        return None
    return bool(not np.ascontiguousarray(got["out"], dtype=np.float32).view(np.uint32)[empty].any()), 0.0


def constant_v(got, case):
    """l is summed from the bf16 weights the product multiplies by: with V constant, out = value to within (L + 16) 2^-24 relative."""
    if not case.const_v or case.out_bf16:
        return None
    bsr = case.bsr
    length = np.repeat(np.diff(np.asarray(bsr.block_row_ptrs, dtype=np.int64)) * bsr.block_row_size, bsr.block_row_size).astype(np.float64)
    rows = length > 0
    rel = np.abs(got["out"][rows].astype(np.float64) / case.const_v - 1.0)
    tol = ((length[rows] + 16) * 2.0 ** -24)[:, None]
    return bool(np.all(rel <= tol)), _worst(rel, tol)


# ---- the backward's checks
@functools.lru_cache(maxsize=None)
def backward_exact(case):
    """float64 (dq, dk, dv) by torch.autograd on dense masked attention; keyed on the case without its types; read-only."""
    from test_gpu_softmax_bsr import _dense_attention
    q, k, v, g = case.arrays
    return _dense_attention(case.bsr, q, k, v, g, case.scale_value, case.mask)[1:]


@functools.lru_cache(maxsize=None)
def backward_tolerances(case):
    q, k, v, g = case.arrays
    return bwd_ref.bwd_tolerances(case.name, q, k, v, g, case.scale_value, case.mask, case.out_bf16, case.grads_bf16, g_rounded=case.g32)


def bwd_composed(got, case):
    """dq, dk, dv against float64 dense masked attention inside tests/_attn_fused_bwd_ref.py::bwd_tolerances.  worst: per gradient."""
    if case.src != "bwd" or case.kind == "blankcols":
        return None
    want = backward_exact(dataclasses.replace(case, out_bf16=False, grads_bf16=False))
    tols = backward_tolerances(case)
    errs = [np.abs(got[n].astype(np.float64) - w) for n, w in zip(("dq", "dk", "dv"), want)]
    return all(bool(np.all(e <= t)) for e, t in zip(errs, tols)), tuple(_worst(e, t) for e, t in zip(errs, tols))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def backward_zero_rows(got, case):
    """+0 bits: dq on the empty block rows of A, dk and dv on the empty block rows of A^T and, under `blankcols`, on the block
    columns whose every block is masked; every other row of dq holds a non-zero; nothing is NaN."""
    if case.src != "bwd" or case.kind not in ("none", "blankcols"):
        return None
    bsr, tbsr, _ = bwd_ref.bwd_pattern(case.name)
    empty_rows, empty_cols = empty_block_rows(bsr), empty_block_rows(tbsr)
    ok = not _bits(got["dq"])[empty_rows].any()
    if case.kind == "none":
        ok = ok and bool((_bits(got["dq"])[~empty_rows] != 0).any(axis=1).all())
        gone = empty_cols
    else:
        gone = empty_cols | np.repeat(blank_columns_mask(bsr, tbsr)[1], bsr.block_row_size)
        ok = ok and not any(np.isnan(got[n]).any() for n in ("dq", "dk", "dv"))
    return bool(ok and not _bits(got["dk"])[gone].any() and not _bits(got["dv"])[gone].any()), 0.0


def subsets_equal(got, case):
    """Every subset of (dq, dk, dv) asked for alone has the bits of the call for all three."""
    if "subsets" not in got:
        return None
    ok = True
    for need, outs in got["subsets"].items():
        for n, wanted, x in zip(("dq", "dk", "dv"), need, outs):
            ok = ok and ((x is None) if not wanted else np.array_equal(_bits(x), _bits(got[n])))
    return bool(ok), 0.0


OLD_FORWARD = {"out_composed": out_composed, "lse_bound": lse_bound, "forward_zero_rows": forward_zero_rows, "constant_v": constant_v}
OLD_BACKWARD = {"bwd_composed": bwd_composed, "backward_zero_rows": backward_zero_rows, "subsets_equal": subsets_equal}
