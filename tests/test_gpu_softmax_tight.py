"""The two row-softmax kernels (mispmm_softmax_csr_f32 / _f64, mispmm_softmax_bsr_f32 and their backward) on the GPU against the
checks that leave no room (tests/_softmax_tight.py, through tests/_softmax_mutants.NEW): the derived tight tolerance, the tie
rows bit for bit, the offset rows, and for the backward -- which has no exponential -- the bits of the lane-order restatement
(tests/_softmax_lanes.py).  Every kernel instance is checked under its own tag: each arithmetic x each G, forward and backward;
bS x held / walk x mask / nomask x out type x p type.  tests/test_softmax_mutants_cpu.py shows on the CPU which faults these
checks catch that the stated bounds of tests/test_gpu_softmax.py and tests/test_gpu_softmax_bsr.py let through.

`To the same bits`.  Which form a row takes is fixed by its length (CSR: registers up to 256 entries, three walks beyond; BSR:
held up to C blocks, walked beyond), so no row has both forms to compare.  What can move is the LAUNCH around it: a row that
the whole wave owns gives the same bits whichever G the host picked for the pattern, and a block row alone (a `held` launch
when it has up to C blocks) gives the bits it gives among the others (a `walk` launch).  Both are held here; that a walked
row's recomputed exponentials are the first walk's is held by the tie rows (exact in walked and held rows alike) and by the
backward's lane bits.

Worst |err| / tight tolerance printed on an MI355X (`-s` prints every one), forward and backward, tight and offset rows together:
f32 REFERENCE 1.00, 1.00 (the half ulp of the one rounding to fp32 is sharp); f32 FAST 0.89, 0.346 (offset rows 0.287, 0.344);
f64 REFERENCE 0.839, 0.396 and f64 FAST 0.839, 0.431 (offset rows 0.246, 0.369); BSR fp32 out 0.976, 0.337 (offset rows 0.247,
0.227), bf16 out 1.00, 1.00 (the half bf16 ulp).  Tie rows and the backward's lane bits: no bit differs, in any instance."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import capi, ops  # noqa: E402

import _softmax_bsr_ref as bref  # noqa: E402
import _softmax_mutants as mut  # noqa: E402
import _softmax_ref as cref  # noqa: E402
import _softmax_tight as tight  # noqa: E402
from _sddmm_bsr_ref import from_bits, to_bits  # noqa: E402
from _softmax_lanes import ARITH, csr_shape  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                     # a copy: the shared operands are read-only


@functools.lru_cache(maxsize=None)
def device_csr(name):
    return ops.DeviceCSR.from_host(cref.matrix(name), plan=False)


def device_bsr_of(bs, ptrs):
    ptrs = np.asarray(ptrs, dtype=np.int64)
    n = int(ptrs[-1])
    return ops.DeviceBSR((ptrs.shape[0] - 1) * bs, max(n, 1) * bs, bs, bs, n, dev(ptrs.astype(np.int32)), dev(np.arange(n, dtype=np.int32)),
                         torch.empty(0, device="cuda"))                                   # columns and values are never read


@functools.lru_cache(maxsize=None)
def device_bsr(name):
    p = bref.pattern(name)
    return device_bsr_of(p.block_row_size, p.block_row_ptrs)


def run_csr(case, operands=None, a=None, group=None):
    """The kernel on a case's operands, its tag asserted: numpy array of the out type."""
    op = operands or tight.csr_operands(case)
    a = a or device_csr(case.name)
    acc = "fast" if case.arith.endswith("fast") else "reference"
    if case.direction == "fwd":
        out = ops.softmax_csr(a, dev(op["s"]), acc=acc)
    else:
        out = ops.softmax_csr_bwd(a, dev(op["p"]), dev(op["dp"]), acc=acc)
    want = f"softmax_csr{'_bwd' if case.direction == 'bwd' else ''}<{case.arith},G{group or op['group']},R{cref.REGS}>"
    assert capi.last_kernel() == want, (capi.last_kernel(), want)
    return out.cpu().numpy()


def run_bsr(case, a=None, rows=slice(None), path=None):
    """The kernel on a case's operands (or on the blocks `rows` of them, as a pattern `a` of their own), its tag asserted:
    float32 values, whichever out type."""
    op = tight.bsr_operands(case)
    bs = op["bs"]
    a = a or device_bsr(case.name)
    path = path or ("held" if a.num_blocks <= bref.HELD[bs] else "walk")
    kind = "bf16" if case.out_bf16 else "f32"
    if case.direction == "fwd":
        mask = None if op["mask"] is None else dev(op["mask"][rows])
        out = ops.softmax_bsr(a, dev(op["s"][rows]), scale=case.scale, mask=mask, out_bf16=case.out_bf16)
        want = f"softmax_bsr<b{bs},{kind},{path},C{bref.HELD[bs]},{'nomask' if mask is None else 'mask'}>"
    else:
        p = dev(to_bits(op["p"][rows])) if case.p_bf16 else dev(op["p"][rows])
        out = ops.softmax_bsr_bwd(a, p, dev(op["dp"][rows]), scale=case.scale, out_bf16=case.out_bf16)
        want = f"softmax_bsr_bwd<b{bs},{kind},{path},C{bref.HELD[bs]},p_{'bf16' if case.p_bf16 else 'f32'}>"
    assert capi.last_kernel() == want, (capi.last_kernel(), want)
    got = out.cpu().numpy()
    return from_bits(got) if case.out_bf16 else got


def hold(run, family, keep):
    """Every NEW check on its cases of `family` that `keep` lets in; prints the worst ratio per check."""
    seen = 0
    for name in mut.NEW:
        worst = 0.0
        cases = [c for c in mut.cases_of(name, family) if keep(c)]
        for case in cases:
            ok, ratio = mut.CHECKS[name](run(case), case)
            assert ok, f"{name} fails on {mut.case_id(case)} {capi.last_kernel()}: {ratio:.3g}"
            worst = max(worst, ratio)
        if cases and name in ("tight", "offset_rows"):
            print(f"{family} {name} {capi.last_kernel()}: worst |err| / tight tolerance over {len(cases)} cases = {worst:.3g}")
        seen += len(cases)
    return seen


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("name", mut.CSR_NAMES)
def test_csr_tight_tolerance_tie_rows_offset_rows_and_lane_bits(name, arith, direction):
    got = functools.lru_cache(maxsize=None)(run_csr)
    seen = hold(got, f"csr_{direction}", lambda c: c.name == name and c.arith == arith)
    assert seen == (3 + 5 + 1 if direction == "fwd" else 2 + 5 + 1 + 2)


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("name", mut.BSR_NAMES)
def test_bsr_forward_tight_tolerance_tie_rows_and_offset_rows(name, out_bf16, mask):
    seen = hold(run_bsr, "bsr_fwd", lambda c: c.name == name and c.out_bf16 == out_bf16 and c.mask == mask)
    assert seen == 6 + mask + 5 + 1                      # narrow and wide at three scales (a mask: the special values too), ties, offset


@pytest.mark.parametrize("p_bf16", [False, True])
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("name", mut.BSR_NAMES)
def test_bsr_backward_tight_tolerance_tie_rows_offset_rows_and_lane_bits(name, out_bf16, p_bf16):
    got = functools.lru_cache(maxsize=None)(run_bsr)
    seen = hold(got, "bsr_bwd", lambda c: c.name == name and c.out_bf16 == out_bf16 and c.p_bf16 == p_bf16)
    assert seen == 4 + 5 + 1 + 3


def same_bits(got, want, what):
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    differ = np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} elements differ, first at {np.argwhere(differ)[:3].tolist()}"


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("arith", ARITH)
def test_csr_a_row_the_wave_owns_has_the_same_bits_whichever_g_the_host_picks(arith, direction):
    """The rows of `edges` among the padding of edges-g4 ... edges-g64, on the same scores: where the whole wave owns a row in
    both launches -- from registers up to 256 entries, in walks beyond -- the bits agree."""
    base = tight.CsrCase(direction, "edges", "offset", arith)
    op = tight.csr_operands(base)
    rp = op["row_ptrs"]
    lens, n = np.diff(rp)[:len(cref.EDGE_LENGTHS)], int(rp[len(cref.EDGE_LENGTHS)])
    whole = run_csr(base)
    forms = set()
    for name in mut.CSR_NAMES[1:]:
        other = tight.CsrCase(direction, name, "offset", arith)
        padded = dict(tight.csr_operands(other))
        for k in ("s", "p", "dp"):
            if k in padded:
                padded[k] = padded[k].copy()
                padded[k][:n] = op[k][:n]
        got = run_csr(other, operands=padded)
        for r, length in enumerate(lens):
            if length and csr_shape(int(length), op["group"])[0] == csr_shape(int(length), padded["group"])[0] == 64:
                same_bits(got[rp[r]:rp[r + 1]], whole[rp[r]:rp[r + 1]], f"{name} against edges, the row of {length} entries")
                forms.add("walk" if length > 256 else "registers")
    assert forms == {"registers", "walk"}


@pytest.mark.parametrize("name", mut.BSR_NAMES)
def test_bsr_a_block_row_alone_has_the_bits_it_has_among_the_others_held_launch_or_walk(name):
    """Block rows of 1, C - 1, C, C + 1 and 2 C + 1 blocks as patterns of their own -- a `held` launch up to C blocks -- on the tie
    rows, the offset rows and the suite's masked scores: the bits of the whole pattern's `walk` launch, and inside the same
    checks."""
    pat = bref.pattern(name)
    bs, c = pat.block_row_size, bref.HELD[pat.block_row_size]
    ptrs = np.asarray(pat.block_row_ptrs, dtype=np.int64)
    cases = [tight.BsrCase("fwd", name, "tie4", 0.125, True, False, True), tight.BsrCase("fwd", name, "tie16", 0.125, False, False, False),
             tight.BsrCase("fwd", name, "offset", 0.3, True, False, False), tight.BsrCase("fwd", name, "narrow", 0.3, True, False, True),
             tight.BsrCase("bwd", name, "tie8", 0.125, False, True, True), tight.BsrCase("bwd", name, "narrow", 0.3, False, False, False),
             tight.BsrCase("bwd", name, "offset", 0.125, False, True, False),
             tight.BsrCase("fwd", name, "tie2", 0.125, False, False, True), tight.BsrCase("bwd", name, "tie1", 0.125, False, False, True)]
    assert {(x.direction, x.mask, x.p_bf16, x.out_bf16) for x in cases} >= {(d, m, p, o) for d, m, p in (("fwd", False, False), ("fwd", True, False),
                                                                                                      ("bwd", False, False), ("bwd", False, True))
                                                                            for o in (False, True)}      # every instance, held too
    for case in cases:
        whole = run_bsr(case)
        exact, tol, dead = tight.reference(case)
        for n in (1, c - 1, c, c + 1, 2 * c + 1):
            r = int(np.argwhere(np.diff(ptrs) == n)[0, 0])
            rows = slice(int(ptrs[r]), int(ptrs[r + 1]))
            alone = run_bsr(case, a=device_bsr_of(bs, [0, n]), rows=rows, path="held" if n <= c else "walk")
            same_bits(alone, whole[rows], f"{mut.case_id(case)}: a block row of {n} blocks alone")
            assert tight.inside(alone, exact[rows], tol[rows], dead[rows])[0]
            if case.kind.startswith("tie"):
                same_bits(alone, tight.tie_expected(case)[rows], f"{mut.case_id(case)}: the tie rows of a block row of {n} blocks alone")
