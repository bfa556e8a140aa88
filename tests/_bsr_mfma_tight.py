"""The checks of the bf16 block-sparse MFMA products (mispmm_bsr_bf16, mispmm_bsrc_bf16, mispmm_bsrc_slots_bf16) as functions of
(got, case), shared by the CPU mutation harness (tests/test_bsr_mfma_mutants_cpu.py, on the numpy restatement) and the GPU tests
(tests/test_gpu_bsr_mfma_tight.py, on the kernels).  `got` is the FLAT C buffer the product wrote into -- rows * ldc elements
and TAIL more behind them, filled with SENTINEL beforehand -- as float32, a bf16 C widened.

THE BOUND (include/mispmm.h, bf16 BSR section).  `exact` is the real-number sum of the element's stored terms, S = sum |a||b|,
u = 2^-23 per addition, g_n = n u / (1 - n u):
    fp32 C   |C - exact| <= g_n S
    bf16 C   C lies between the bf16 roundings (nearest even) of the two ends of [exact - g_n S, exact + g_n S]
THE COUNT n, from the code.  The product of two bf16 numbers has 16 significant bits: exact in fp32.  So only additions round,
and a term's error factor is one (1 + d), |d| <= u, per addition on its way to the stored value; adding an exact zero rounds
nothing.  n bounds the additions on the longest such way, n = P + T + W:
    P   the element's products that are not zero: inside ONE MFMA a term meets at most as many rounding additions as the step
        has non-zero products (the order in there is the hardware's; any order adds k non-zero terms to the addend in k
        additions that can round), and summed over the steps that is at most P;
    T   the MFMA steps the busiest wave runs for that block row, one join with the accumulator each:
          bsr_mfma_bf16      pair p -> wave p % 4:   T = ceil(ceil(blocks / 2) / 4)
          bsr_mfma_bf16_b32  block b -> wave b % 4:  T = ceil(blocks / 4)      (two halves, two accumulators: the same count)
          bsrc_mfma_bf16     one wave, all steps:    T = steps
          bsrc_slots         slot + extra steps:     T = 1 + ceil(extra / 3)   (wave 1 takes extra steps 0, 3, 6, ...)
    W   partial tiles added across waves: 3 for the three 4-wave kernels (wave 0, or the owner of a row quad, adds the other
        three in wave order), 0 for bsrc_mfma_bf16.
No constant here comes from running a kernel.  The reference is numpy in np.longdouble (its own error, at most P 2^-52 S, is
2^-29 of the tolerance and is ignored), never the oracle.

NaN / Inf.  The dense-block kernels (bsr_mfma_bf16, _b32, bsr_bf16_lds) multiply every stored element of a block, an explicit
zero included: 0 * Inf = NaN.  The compacted kernels multiply the 16 rows of every OCCUPIED column of a block row (a column in
which some row holds a value that is non-zero as bf16) and nothing else.  `terms` below is that rule; exact, S and P follow.

THE FOUR CHECKS.  tight (wide-exponent operands, the bound above; for a bf16 C an element whose interval ends round to two
bf16 numbers is `flagged` and allowed either, and a case with more than FLAG_CAP of its live elements flagged is refused);
sharp_exact (bf16 numbers in [0.5, 2) with all 8 bits in use, sum |a||b| < 2^8 on every element, so every partial sum in any
order is a multiple of 2^-16 below 2^8 and exact in fp32 -- the argument of _attn_tight.exact_products: bit for bit, ties of
the bf16 rounding in both parities among them); specials (NaN and +-Inf planted in B rows that are occupied, in B rows that
only a padding slot, a missing pair half or an unoccupied column could touch, and in block values: NaN positions and Inf signs
as the rule above gives them, every other element inside `tight`); untouched (an empty block row is +0, the gap of ldc > N and
the tail keep the sentinel)."""
import collections
import functools

import numpy as np

import _bsr_mfma_lanes as lanes
import _sddmm_bsr_ref as sbr
from mispmm import formats

SENTINEL = np.float32(-7.0)
TAIL = 64
U = 2.0 ** -23
FLAG_CAP = 0.02

# kernel: bsr16 | bsr32 | bsrc | slots (| lds: the child process's arrays, sharp only); pattern: PATTERNS or an old case's name
Case = collections.namedtuple("Case", "kernel pattern kind n ldb ldc out_bf16")

# blocks (dense) or occupied columns (compacted) per block row; an empty row inside and, for the dense ones, at the end
PATTERNS = {
    "p16": dict(bs=16, bc=16, nbc=20, counts=[3, 1, 0, 2, 4, 5, 8, 9, 17, 0]),
    "p32": dict(bs=32, bc=32, nbc=12, counts=[3, 1, 0, 4, 5, 9]),
    "c16": dict(bs=16, bc=16, nbc=16, occupied=[31, 1, 0, 32, 33, 128, 129, 161]),
    "c8": dict(bs=16, bc=8, nbc=32, occupied=[31, 1, 0, 32, 33, 128, 129, 161]),
    "c16s": dict(bs=16, bc=16, nbc=16, occupied=[31, 1, 0, 32, 33, 128]),          # no extra steps: the `share` instance
    "c8s": dict(bs=16, bc=8, nbc=32, occupied=[31, 1, 0, 32, 33, 128]),
}
ROW_CAP = 64          # non-zeros per row: 64 products below 4 keep sum |a||b| < 2^8


def case_id(case):
    return ",".join(str(x) for x in case)


# ------------------------------------------------------------------------------------------------ patterns and operands
@functools.lru_cache(maxsize=None)
def structure(name):
    """(block_row_ptrs, block_col_idxs, mask [nb, bs, bc] of the non-zero positions).  Block columns 0 and nbc - 1 are used by
    no block row (B rows 0 and K - 1 are touched by nobody), block columns are not ascending, a row holds at most ROW_CAP
    non-zeros, the one-block / one-column row holds ONE product per element (the tie row)."""
    p = PATTERNS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    bs, bc, nbc = p["bs"], p["bc"], p["nbc"]
    ptrs, idxs, masks = [0], [], []
    for r, cnt in enumerate(p.get("counts", p.get("occupied"))):
        compacted = "occupied" in p
        nblk = (0 if cnt == 0 else -(-cnt // bc) + 1) if compacted else cnt
        assert nblk <= nbc - 2
        cols = rng.permutation(np.arange(1, nbc - 1))[:nblk]
        if nblk > 1 and np.all(np.diff(cols) > 0):
            cols = cols[::-1]
        m = np.zeros((nblk, bs, bc), bool)
        if compacted and cnt:
            occ = np.sort(rng.choice(nblk * bc, size=cnt, replace=False))
            for q, o in enumerate(occ):
                m[o // bc, :, o % bc] = True if cnt == 1 else rng.random(bs) < 0.5
                m[o // bc, q % bs, o % bc] = True
        elif cnt == 1:
            m[0, np.arange(bs), (5 * np.arange(bs) + 3) % bc] = True
        elif cnt:
            m[:] = rng.random(m.shape) < 0.85
        for i in range(bs):                                         # the cap; an occupied column keeps a non-zero
            for b, j in rng.permutation(np.argwhere(m[:, i, :])):
                if m[:, i, :].sum() <= ROW_CAP:
                    break
                if not compacted or m[b, :, j].sum() > 1:
                    m[b, i, j] = False
            assert m[:, i, :].sum() <= ROW_CAP
        idxs += list(cols)
        masks.append(m)
        ptrs.append(len(idxs))
    return np.array(ptrs, np.uint32), np.array(idxs, np.uint32), np.concatenate(masks)


def _wide(rng, shape):
    """sbr.wide_exponent's magnitudes (8-bit mantissas, exponents uniform in [-6, 6], so the fp32 sums really round) with one
    sign in twenty negative: both signs meet in every sum, but few sums cancel so far that the tolerance reaches the spacing of
    bf16 numbers around them (the flagged elements of a bf16 C; FLAG_CAP)."""
    return (np.abs(sbr.wide_exponent(rng, shape, spread=6)) * np.where(rng.random(shape) < 0.05, -1.0, 1.0)).astype(np.float32)


def _sharp(rng, shape):
    """Random signs, m / 128 and m / 256 with m in [128, 255]: bf16 numbers in [0.5, 2), all 8 significant bits in use."""
    v = rng.integers(128, 256, shape) * 2.0 ** -rng.integers(7, 9, shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def operands(case):
    """{bsr (formats.BSR, float32 values that are bf16 numbers), b [K, N] float32 of bf16 numbers, planted: what specials put
    where}.  Read-only."""
    if case.pattern.startswith("old:"):
        return _old_operands(case)
    p = PATTERNS[case.pattern]
    ptrs, idxs, mask = structure(case.pattern)
    bs, bc, k = p["bs"], p["bc"], p["nbc"] * p["bc"]
    rng = np.random.default_rng(1000 + sum(map(ord, case.pattern)) + case.n)
    make = _sharp if case.kind == "sharp" else _wide
    data = np.where(mask, make(rng, mask.shape), np.float32(0)).astype(np.float32)
    b = make(rng, (k, case.n)).astype(np.float32)
    planted = {}
    if case.kind == "sharp":
        one = p.get("counts", p.get("occupied")).index(1)            # the tie row: one product per element, 1.5 b or 0.75 b
        lo, hi = int(ptrs[one]), int(ptrs[one + 1])
        data[lo:hi] = np.where(mask[lo:hi], np.where(rng.random(mask[lo:hi].shape) < 0.5, 1.5, 0.75), 0).astype(np.float32)
    if case.kind == "specials":
        b, data = b.copy(), data.copy()
        used = np.unique((idxs.astype(np.int64)[:, None] * bc + np.arange(bc)).reshape(-1)[mask.any(axis=1).reshape(-1)])
        for row, col, v in ((used[1], 1, np.nan), (used[len(used) // 2], case.n - 1, np.inf), (used[-2], case.n // 2, -np.inf),
                            (used[0], 0, np.inf), (int(idxs[0]) * bc + 3, 2, np.inf)):
            b[row, col] = v
        stored = np.zeros(k, bool)
        stored[(idxs.astype(np.int64)[:, None] * bc + np.arange(bc)).reshape(-1)] = True
        idle = np.flatnonzero(stored & ~np.isin(np.arange(k), used))           # stored but nobody's non-zero: explicit zeros only
        for row, col, v in [(0, 1, np.inf), (0, case.n - 2, np.nan), (k - 1, 0, -np.inf), (k - 1, 3, np.nan)] + \
                [(int(r), int(r) % case.n, np.inf) for r in idle[:3]] + [(int(r), (int(r) + 1) % case.n, np.nan) for r in idle[3:5]]:
            b[row, col] = v
        nz = np.argwhere(mask)
        data[tuple(nz[len(nz) // 3])] = np.inf
        data[tuple(nz[2 * len(nz) // 3])] = np.nan
        planted = dict(used=used, idle=idle)
    nb = mask.shape[0]
    bsr = formats.BSR((len(ptrs) - 1) * bs, k, nb * bs * bc, bs, bc, ptrs, idxs, data)
    return dict(bsr=bsr, b=b, planted=planted)


def b_flat(case, gap=np.float32(3.0)):
    """B as the kernel sees it: K * ldb elements, the gap behind N filled with a finite number nobody may read into C."""
    b = operands(case)["b"]
    flat = np.full((b.shape[0], case.ldb), gap, np.float32)
    flat[:, :case.n] = b
    return flat.reshape(-1)


# ------------------------------------------------------------------------------------------------ the reference
def terms(case, r):
    """(B rows, coefficients [bs, T]) of block row r under the case's kernel family: every stored element for the dense-block
    kernels, the occupied columns for the compacted ones."""
    bsr = operands(case)["bsr"]
    bs, bc = bsr.block_row_size, bsr.block_col_size
    lo, hi = int(bsr.block_row_ptrs[r]), int(bsr.block_row_ptrs[r + 1])
    data = np.asarray(bsr.data, np.float64).reshape(-1, bs, bc)[lo:hi]
    rows = (np.asarray(bsr.block_col_idxs, np.int64)[lo:hi, None] * bc + np.arange(bc)).reshape(-1)
    coef = data.transpose(1, 0, 2).reshape(bs, -1)
    if case.kernel in ("bsrc", "slots"):
        occ = np.any(coef != 0, axis=0)                             # a NaN or an Inf is not zero
        rows, coef = rows[occ], coef[:, occ]
    return rows, coef


def steps_and_waves(case, r):
    """(T, W) of the count n for block row r."""
    bsr = operands(case)["bsr"]
    cnt = int(bsr.block_row_ptrs[r + 1]) - int(bsr.block_row_ptrs[r])
    if case.kernel in ("bsr16", "lds"):
        return (-(-(-(-cnt // 2)) // 4), 3) if case.kernel == "bsr16" else (-(-cnt // 2), 0)
    if case.kernel == "bsr32":
        return -(-cnt // 4), 3
    steps = -(-terms(case, r)[0].shape[0] // 32)
    return (steps, 0) if case.kernel == "bsrc" else (1 + -(-max(steps - 4, 0) // 3), 3)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(exact, tol, dead, scale) [M, N] float64: dead = NaN or +-Inf by the contract (exact holds which), tol = g_n S elsewhere."""
    ops_ = operands(case)
    bsr, b = ops_["bsr"], np.asarray(ops_["b"], np.longdouble)
    bs = bsr.block_row_size
    m = bsr.num_rows
    exact, tol, scale = np.zeros((m, case.n)), np.zeros((m, case.n)), np.zeros((m, case.n))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(m // bs):
            rows, coef = terms(case, r)
            if rows.shape[0] == 0:
                continue
            br, cf = b[rows], coef.astype(np.longdouble)
            e = (cf[:, :, None] * br[None]).sum(axis=1)
            s = (np.abs(cf)[:, :, None] * np.abs(br)[None]).sum(axis=1)
            p = (cf != 0).astype(np.float64) @ (br != 0).astype(np.float64)
            t, w = steps_and_waves(case, r)
            n = (p + t + w) * U
            sl = slice(r * bs, (r + 1) * bs)
            exact[sl], scale[sl] = e.astype(np.float64), s.astype(np.float64)
            tol[sl] = n / (1.0 - n) * s.astype(np.float64)
    dead = ~np.isfinite(exact)
    tol[dead] = 0.0
    return exact, tol, dead, scale


def c_view(got, case):
    m = operands(case)["bsr"].num_rows
    got = np.asarray(got, np.float32)
    assert got.shape == (m * case.ldc + TAIL,), (got.shape, m, case.ldc)
    return got[:m * case.ldc].reshape(m, case.ldc)


def _ends16(exact, tol):
    """The bf16 roundings of the smallest fp32 number >= exact - tol and the largest <= exact + tol."""
    lo, hi = exact - tol, exact + tol
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32.astype(np.float64) < lo, np.nextafter(lo32, np.float32(np.inf)), lo32)
    hi32 = np.where(hi32.astype(np.float64) > hi, np.nextafter(hi32, np.float32(-np.inf)), hi32)
    return lanes.bf16_rne(lo32).astype(np.float64), lanes.bf16_rne(hi32).astype(np.float64)


def flagged(case):
    """bf16 C: the live elements whose interval ends round to different bf16 numbers."""
    exact, tol, dead, _ = reference(case)
    lo, hi = _ends16(np.where(dead, 0.0, exact), tol)
    return (lo != hi) & ~dead


def within(got, case):
    """(ok [M, N], ratio [M, N]) of the live elements against the derived bound.  ratio = |err| / tol for an fp32 C; for a bf16 C
    the least error an fp32 number rounding to `got` can have, over tol."""
    exact, tol, dead, _ = reference(case)
    c = c_view(got, case)[:, :case.n].astype(np.float64)
    ex = np.where(dead, 0.0, exact)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(c - ex)
        if case.out_bf16:
            lo, hi = _ends16(ex, tol)
            ok = (c >= lo) & (c <= hi)
            half = np.ldexp(1.0, np.frexp(c)[1] - 9)                # half a bf16 ulp of c: what its rounding may have cost
            err = np.maximum(err - half, 0.0)
            err = np.where(ok, np.minimum(err, tol), np.maximum(err, tol * 1.0000001))
        else:
            ok = err <= tol
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    ok = np.where(dead, True, ok & np.isfinite(c))
    return ok, np.where(dead, 0.0, ratio)


# ------------------------------------------------------------------------------------------------ the checks: (ok, worst)
def tight(got, case):
    if case.out_bf16:
        assert flagged(case).sum() <= FLAG_CAP * (~reference(case)[2]).sum(), f"{case_id(case)}: too many flagged elements"
    ok, ratio = within(got, case)
    return bool(ok.all()), float(ratio.max(initial=0.0))


def sharp_premise(case):
    """sum |a||b| < 2^8 on every element, every operand a bf16 number in [0.5, 2)."""
    ops_ = operands(case)
    for v in (np.asarray(ops_["bsr"].data)[np.asarray(ops_["bsr"].data) != 0], ops_["b"]):
        a = np.abs(v)
        if not (np.all(a >= 0.5) and np.all(a < 2.0) and np.array_equal(lanes.bf16_rne(v), v)):
            return False
    return bool(np.all(reference(case)[3] < 2.0 ** 8))


def sharp_want(case):
    exact = reference(case)[0].astype(np.float32)
    assert np.array_equal(exact.astype(np.float64), reference(case)[0])
    return lanes.bf16_rne(exact) if case.out_bf16 else exact


def sharp_ties(case):
    """(ties that round down to an even bf16, ties that round up to one) among the exact answers."""
    u = reference(case)[0].astype(np.float32).view(np.uint32)
    tie = (u & np.uint32(0xFFFF)) == np.uint32(0x8000)
    odd = ((u >> np.uint32(16)) & np.uint32(1)) == 1
    return int((tie & ~odd).sum()), int((tie & odd).sum())


def sharp_exact(got, case):
    c = c_view(got, case)[:, :case.n]
    wrong = c != sharp_want(case)                                   # the sign of a zero is not held
    return not wrong.any(), float(wrong.sum())


def specials(got, case):
    exact, _, dead, _ = reference(case)
    c = c_view(got, case)[:, :case.n].astype(np.float64)
    nan_ok = np.array_equal(np.isnan(c), np.isnan(exact))
    inf = np.isinf(exact)
    inf_ok = np.array_equal(np.isinf(c), inf) and np.array_equal(np.sign(c[inf]), np.sign(exact[inf]))
    ok, ratio = within(got, case)
    return bool(nan_ok and inf_ok and ok.all()), float(ratio.max(initial=0.0))


def untouched(got, case):
    bsr = operands(case)["bsr"]
    c = c_view(got, case)
    bs = bsr.block_row_size
    empty = np.repeat(np.diff(np.asarray(bsr.block_row_ptrs, np.int64)) == 0, bs)
    zero = np.all(c[empty, :case.n].view(np.uint32) == 0)
    gap = np.all(c[:, case.n:] == SENTINEL) and np.all(np.asarray(got)[c.size:] == SENTINEL)
    return bool(zero and gap), 0.0


# ------------------------------------------------------------------------------------------------ the checks as they stood
def _old_operands(case):
    """The operands of today's tests: a census row (`old:<tag>`, kinds full / ints of run_bf16) or the ragged 16 x 8 slots case of
    test_bsrc_slots_bf16_ragged_rows_extra_steps_and_strides (`old:ragged`)."""
    import _census as census
    from mispmm import synth
    if case.pattern == "old:ragged":
        rng = np.random.default_rng(12)
        mb, kb, bc = 10, 60, 8
        ptrs, idxs, blocks = [0], [], []
        for r in range(mb):
            cnt = [0, 1, 12, 3, 0, 7, 25, 2, 44, 60][r]
            idxs += list(np.sort(rng.choice(kb, size=cnt, replace=False)))
            for _ in range(cnt):
                blocks.append(np.where(rng.random((16, bc)) < 0.6, rng.uniform(-2, 2, (16, bc)), 0.0).astype(np.float32))
            ptrs.append(len(idxs))
        data = synth.bf16_round(np.stack(blocks).reshape(-1)).reshape(-1, 16, bc)
        bsr = formats.BSR(mb * 16, kb * bc, int(data.size), 16, bc, np.array(ptrs, np.uint32), np.array(idxs, np.uint32), data)
        b = synth.dense_b(kb * bc, case.n)
        return dict(bsr=bsr, b=synth.bf16_round(b.reshape(-1)).reshape(b.shape), planted={})
    spec = next(row.spec for fam in ("bsr_mfma_bf16", "bsr_mfma_bf16_b32", "bsrc_mfma_bf16", "bsrc_slots_mfma_bf16")
                for row in census.FAMILIES[fam] if row.key == case.pattern[4:])
    host = census.bsr_operands(spec)
    bsr = host["bsr"]
    if case.kind == "full":
        blocks = synth.bf16_round(bsr.data.reshape(-1)).reshape(bsr.data.shape)
        b = synth.bf16_round(host["b"].reshape(-1)).reshape(host["b"].shape)
    else:
        rng = np.random.default_rng(17)
        blocks = np.where(bsr.data != 0, rng.integers(-4, 5, bsr.data.shape), 0).astype(np.float32)
        b = rng.integers(-8, 9, host["b"].shape).astype(np.float32)
    a16 = formats.BSR(bsr.num_rows, bsr.num_cols, bsr.nnz, spec["bs"], spec["bs"], bsr.block_row_ptrs, bsr.block_col_idxs, blocks)
    return dict(bsr=a16, b=b, planted={})


@functools.lru_cache(maxsize=None)
def oracle_like(case):
    """(ref, scale): the oracle's sum restated -- fp32, every stored element of a block row in storage order, ascending column
    inside a block -- and |A| |B| in float64."""
    ops_ = operands(case)
    bsr, b = ops_["bsr"], ops_["b"].astype(np.float32)
    bs, bc = bsr.block_row_size, bsr.block_col_size
    ref, scale = np.zeros((bsr.num_rows, case.n), np.float32), np.zeros((bsr.num_rows, case.n))
    data = np.asarray(bsr.data, np.float32).reshape(-1, bs, bc)
    for r in range(bsr.num_rows // bs):
        sl = slice(r * bs, (r + 1) * bs)
        for blk in range(int(bsr.block_row_ptrs[r]), int(bsr.block_row_ptrs[r + 1])):
            col0 = int(bsr.block_col_idxs[blk]) * bc
            for j in range(bc):
                ref[sl] = ref[sl] + data[blk][:, j, None] * b[col0 + j][None, :]
            scale[sl] += np.abs(data[blk]).astype(np.float64) @ np.abs(b[col0:col0 + bc]).astype(np.float64)
    return ref, scale


def stated_limit(case):
    ref, scale = oracle_like(case)
    return 2e-6 * scale + 1e-30 + (2.0 ** -8 * np.abs(ref.astype(np.float64)) if case.out_bf16 else 0.0)


def old_bound(got, case):
    """|got - oracle| <= 2e-6 * scale (+ 2^-8 |ref| for a bf16 C): every bound assertion of the old tests."""
    c = c_view(got, case)[:, :case.n].astype(np.float64)
    lim = stated_limit(case)
    with np.errstate(invalid="ignore"):
        err = np.abs(c - oracle_like(case)[0])
        ok = err <= lim
    return bool(ok.all()), float(np.nanmax(err / lim, initial=0.0))


def old_ints(got, case):
    """run_bf16's integer kind: bit for bit against the oracle (rounded once for a bf16 C)."""
    ref = oracle_like(case)[0]
    want = lanes.bf16_rne(ref) if case.out_bf16 else ref
    wrong = c_view(got, case)[:, :case.n] != want
    return not wrong.any(), float(wrong.sum())


def old_sentinel(got, case):
    """assert_sentinel, and the ragged case's `an empty block row is overwritten with zeros`."""
    c = c_view(got, case)
    ok = np.all(c[:, case.n:] == SENTINEL) and np.all(np.asarray(got)[c.size:] == SENTINEL)
    if case.pattern == "old:ragged":
        ok = ok and np.all(c[4 * 16:5 * 16, :case.n] == 0)
    return bool(ok), 0.0
