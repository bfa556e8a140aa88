"""Checks of the two row-softmax kernels that leave no room: a tolerance DERIVED from the words of include/mispmm.h (sections
"Row softmax on a CSR pattern", "Row softmax on a BSR pattern") and the lane order of tests/_softmax_lanes.py, rows whose
answers are exact, and rows that ride on a large offset.  Functions of (got, case): the CPU harness
(tests/test_softmax_mutants_cpu.py) and the GPU tests (tests/test_gpu_softmax_tight.py) call the same code, after
tests/_attn_csr_tight.py.  No constant below comes from running a kernel or the restatement.

(a) THE TIGHT TOLERANCE.  The reference is the header's `exact`: the real-number softmax of the given scores (BSR: of the fp32
z = fma(scale, s, mask), which is part of the definition), in the widest float numpy has.  What a kernel that keeps the words
may differ by, u the unit roundoff of its arithmetic (2^-53; f32 FAST and BSR 2^-24), g_n = n u / (1 - n u):
  the exponential of entry e, relative eps_e: the header's count PER ENTRY -- the rounded difference t_e = s_e - m turned by
      the exp into |t_e| u, the exp itself 1 ulp = 2 u: eps_e = (|t_e| + 2) u; FAST: the rounded log2 e and the rounded
      product add 2 |t_e| u: eps_e = (3 |t_e| + 2) u.  The header puts the row's worst T here for every entry.
  the sum: a term passes the additions of ITS OWN PATH only: a lane's chain (the live slots of lane 0: ceil(L / W); BSR: 4
      elements of every block of wave 0), the butterfly's log2 W steps, on BSR 3 more where the waves meet -- and never more
      than the L - 1 of any order; adding +0 is exact.  d = min(chain + steps (+ 3), L - 1), relative g_d.  The header puts L.
  the division: u.
  out_e / exact_e = (1 + de_e)(1 + dq) / sum_e' p_e' (1 + de_e')(1 + ds_e'), so to first order the relative error is
      de_e - sum_e' p_e' de_e' - sum_e' p_e' ds_e' + dq: the entry's own exponential error is common to numerator and
      denominator with weight p_e and cancels that far -- a factor common to a quotient of sums cancels --
      rel_e = 1.01 (eps_e (1 - p_e) + sum_{e' != e} p_e' eps_e' + g_d + u),   1.01 for the second order (rel < 2^-15).
  each kernel keeps its own underflow terms and its own last rounding:
      f64         |out - exact| <= rel exact + 2 tiny
      f32 ref64   |out - exact| <= h32(exact) + rel exact + 2 tiny,  h32(x) = half an fp32 ulp of x: the one rounding to fp32
                  (rounding is monotone and rel exact is far below an ulp, so the rounded value lies within half an ulp OF
                  EXACT'S BINADE of the unrounded one; the header says 2^-24 exact, up to twice as much)
      f32 fast    |out - exact| <= rel exact + 2^-126                BSR fp32 out: the same
      BSR bf16    |out - exact| <= h16(exact) + (the fp32 tolerance) + 2^-126,  h16 half a bf16 ulp: the rounding of the fp32
                  result, exactly (the header says 2^-8 exact: up to four times as much)
  BACKWARD, on the given p and dp, S = sum |p||dp|: the dot's terms pass d' = min(chain + steps (+ 3), L) fmas and additions
  (f64 REFERENCE rounds the product apart: d' + 1), so |dot^ - dot| <= g_d' S; then fl(dp - dot^), fl(p * .) (BSR: and
  fl(scale * .)), k = 2 (3) roundings:  ds^ = p (dp - dot)(1 + th_k) - p (dot^ - dot)(1 + th_k), hence
      |ds - exact| <= g_k |exact| + g_(d' + k) |p| S   (BSR: times scale)   + the kernel's own underflow term,
  and f32 ref64 / bf16 out add h32(|exact|) / h16(|exact|) for the last rounding.  No 1.01: g carries the second order.
  Every element that is finite by contract is covered; where the contract says NaN the result must be NaN.  Element by
  element the tolerance is no looser than the header's bound (asserted on the CPU).

(b) TIE ROWS.  On the `edges` patterns: in every row t entries (1, 2, 4, 8, 16; the largest power of two <= L where the row is
shorter) share the maximum, a finite OFFSET C, and every other entry lies a multiple of `gap` below it.  Per arithmetic
(TIE_OFFSET; asserted on the CPU): exp(C) overflows the accumulator's type (fp64 for f32 ref64: C = 1024; fp32: C = 128),
so a forward that does not subtract the maximum cannot pass, and exp(-gap) is below the subnormals, exactly +0.  Then every
live term is exp(0) = 1, the sum is t in any order and out is exactly 1 / t or +0, bit for bit, in every arithmetic and out
type.  Backward: p = that out, dp = t * (integers in -3 .. 3): every product and partial sum is a small integer, dp - dot is
one, and ds = p (dp - dot) (BSR: times the power-of-two scale) is exact; the sign of a zero follows IEEE.  BSR: scale =
2^-3, the offset carried by the scores or, in the other variant, by a FINITE mask.

(c) OFFSET ROWS.  scores = C + (narrow scores rounded to multiples of 2^-8), C = +-1000 (fp32), +-10^4 (fp64), the sign by row:
exact in the scores' type, s - m exact and |t| < 8, so the tight tolerance is about (3 * 8 + 2 + d + 1) u ~ 50 u relative.
An fp32 value near 1000 has an ulp of 2^-14 = 1024 u: a z that is ONE ulp off moves every quotient of its row by up to
1024 u, twenty times the tolerance.  BSR with a mask: the mask carries C, the scores are the suite's full-mantissa ones and
scale = 0.3, so the product scale * s is inexact and fl(fl(scale * s) + mask) differs from the fma wherever the exact sum
lies within 2^-25 of a rounding tie of spacing 2^-14: about one element in 2^10.  (With a power-of-two scale the product is
exact and the two forms are the same number.)"""
import collections
import functools

import numpy as np

import _softmax_bsr_ref as bref
import _softmax_ref as cref
from _sddmm_ref import entry_rows
from _softmax_lanes import WAVE, WAVES, csr_shape

LD = cref.LD
TIES = (1, 2, 4, 8, 16)
TIE_OFFSET = {"f32,ref64": (1024.0, 1024.0), "f32,fast": (128.0, 128.0), "f64,ref": (1024.0, 1024.0), "f64,fast": (1024.0, 1024.0),
              "bsr": (128.0, 128.0)}                       # arithmetic -> (C, gap)
OFFSET = {np.dtype(np.float32): 1000.0, np.dtype(np.float64): 1.0e4}
TIE_SCALE = 0.125

# direction: "fwd" | "bwd";  kind: narrow | wide | equal | specials | zero_dp | offset | tie<t>
CsrCase = collections.namedtuple("CsrCase", "direction name kind arith")
# mask: the forward reads one (tie rows: the mask carries the offset);  p_bf16: the backward's p is bf16
BsrCase = collections.namedtuple("BsrCase", "direction name kind scale mask p_bf16 out_bf16")


def dtype_of(arith):
    return np.float32 if arith.startswith("f32") else np.float64


def unit(arith):
    return 2.0 ** -24 if arith in ("f32,fast", "bsr") else 2.0 ** -53


def gamma(n, u):
    return n * u / (1.0 - n * u)


def half_ulp(x, bits):
    """Half an ulp of |x| in a format of `bits` significand bits (24: fp32, 8: bf16) as if its exponent range had no end; 0
    at 0.  Below the normal range the format's grid is coarser than this: that is what each tolerance's underflow term
    (2 tiny, 2^-126) is for, as in the header, where the relative terms `hold for results in the normal range only`."""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.where(np.asarray(x, dtype=np.float64) == 0, 0.0, np.ldexp(1.0, e - 1 - bits))


# ---- operands
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _tie_positions(mode, length, n, anchor, step, rng):
    """n distinct positions in a row of `length`: 0 from the start; 1 the row's last; 2 from `anchor` back by `step`, what falls
    off the front made up from the start; 3 anywhere."""
    if mode == 0:
        return np.arange(n)
    if mode == 1:
        return length - n + np.arange(n)
    if mode == 2:
        pos = [p for p in (anchor - step * k for k in range(n)) if p >= 0]
        pos += [p for p in range(length) if p not in set(pos)][:n - len(pos)]
        return np.array(pos)
    return rng.choice(length, n, replace=False)


def _tie_count(t, length):
    return 0 if length == 0 else min(t, 1 << (int(length).bit_length() - 1))


@functools.lru_cache(maxsize=None)
def csr_tie(name, t):
    """(tied [nnz] bool, count of tied entries per entry's row [nnz])."""
    csr = cref.matrix(name)
    group = cref.picked_group(csr.num_rows, csr.nnz)
    rp = np.asarray(csr.row_ptrs, dtype=np.int64)
    rng = np.random.default_rng(5100 + t)
    tied, count = np.zeros(csr.nnz, bool), np.zeros(csr.nnz, np.int64)
    for r, (lo, hi) in enumerate(zip(rp[:-1], rp[1:])):
        length = int(hi - lo)
        n = _tie_count(t, length)
        if n == 0:
            continue
        w, _ = csr_shape(length, group)
        anchor = w * ((length - 1) // w) - 1                 # the last entry of lane W - 1
        tied[lo + _tie_positions((r + TIES.index(t)) % 4, length, n, anchor if anchor >= 0 else length - 1, 1, rng)] = True
        count[lo:hi] = n
    tied.setflags(write=False)
    count.setflags(write=False)
    return tied, count


@functools.lru_cache(maxsize=None)
def bsr_tie(name, t):
    """(tied [num_blocks, bS, bS] bool, count per element)."""
    p = bref.pattern(name)
    bs, c = p.block_row_size, bref.HELD[p.block_row_size]
    ptrs = np.asarray(p.block_row_ptrs, dtype=np.int64)
    rng = np.random.default_rng(5200 + t + bs)
    tied = np.zeros((p.num_blocks, bs, bs), bool)
    for r, (lo, hi) in enumerate(zip(ptrs[:-1], ptrs[1:])):
        n = int(hi - lo)
        for i in range(bs if n else 0):
            anchor = min(c + 1, n - 1) * bs + (3 * i + r) % bs
            pos = _tie_positions((r * bs + i + TIES.index(t)) % 4, n * bs, t, anchor, bs, rng)
            tied[lo + pos // bs, i, pos % bs] = True
    tied.setflags(write=False)
    return tied, np.full(tied.shape, t, np.int64)


def _gaps(shape, seed):
    return 1.0 + np.random.default_rng(seed).integers(0, 4, shape)


def _tie_dp(count, seed):
    return count * np.random.default_rng(seed).integers(-3, 4, count.shape)


def _quantised(v):
    return np.rint(np.asarray(v, dtype=np.float64) * 256.0) / 256.0


@functools.lru_cache(maxsize=None)
def csr_operands(case):
    """fwd: dict(row_ptrs, group, s); bwd: dict(row_ptrs, group, p, dp).  Read-only."""
    csr = cref.matrix(case.name)
    dt = dtype_of(case.arith)
    rp = np.asarray(csr.row_ptrs, dtype=np.int64)
    base = dict(row_ptrs=rp, group=cref.picked_group(csr.num_rows, csr.nnz))
    kind = case.kind
    if kind.startswith("tie"):
        t = int(kind[3:])
        tied, count = csr_tie(case.name, t)
        c, gap = TIE_OFFSET[case.arith]
        if case.direction == "fwd":
            return _frozen(dict(base, s=np.where(tied, c, c - gap * _gaps(csr.nnz, 5300 + t)).astype(dt)))
        return _frozen(dict(base, p=np.where(tied, 1.0 / np.maximum(count, 1), 0.0).astype(dt), dp=_tie_dp(count, 5400 + t).astype(dt)))
    if kind == "specials":                                     # tests/test_gpu_softmax.py::test_masks_and_special_values
        lens = np.diff(rp)
        rng = np.random.default_rng(8)
        s = cref.scores("narrow", csr.nnz, dt).copy()
        s[rng.random(csr.nnz) < 0.25] = -np.inf
        r_inf, r_nan, r_pinf, r_keep = [int(np.argwhere(lens == n)[0, 0]) for n in (17, 65, 300, 1025)]
        s[rp[r_inf]:rp[r_inf + 1]] = -np.inf
        s[rp[r_nan] + 40] = np.nan
        s[rp[r_pinf] + 7] = np.inf
        s[rp[r_keep]] = 0.0
        return _frozen(dict(base, s=s))
    if kind == "offset":
        sign = np.where(entry_rows(rp) % 2 == 0, 1.0, -1.0)
        s = (sign * OFFSET[np.dtype(dt)] + _quantised(cref.scores("narrow", csr.nnz, np.float64))).astype(dt)
    else:
        s = cref.scores("narrow" if kind == "zero_dp" else kind, csr.nnz, dt)
    if case.direction == "fwd":
        return _frozen(dict(base, s=s))
    dp = np.zeros(csr.nnz, dt) if kind == "zero_dp" else cref.full_mantissa(np.random.default_rng(10), csr.nnz, dt)
    return _frozen(dict(base, p=cref.softmax_rows(rp, s).astype(dt), dp=dp))


def _bsr_special_rows(name):
    """[(block row, element row, what)]: a NaN, a +Inf and an all -Inf matrix row, each in another block row (first, last
    non-empty, one of C + 1 blocks)."""
    p = bref.pattern(name)
    counts = np.diff(np.asarray(p.block_row_ptrs, dtype=np.int64))
    filled = np.argwhere(counts > 0).ravel()
    walk = np.argwhere(counts == bref.HELD[p.block_row_size] + 1).ravel()
    return [(int(filled[0]), 3, "nan"), (int(filled[-1]), 8, "+inf"), (int(walk[0]), 13, "all -inf"), (int(walk[0]), 5, "+inf")]


@functools.lru_cache(maxsize=None)
def bsr_operands(case):
    """fwd: dict(ptrs, bs, s, mask, scale); bwd: dict(ptrs, bs, p, dp, scale), p as float32 values.  Read-only."""
    pat = bref.pattern(case.name)
    bs = pat.block_row_size
    ptrs = np.asarray(pat.block_row_ptrs, dtype=np.int64)
    shape = (pat.num_blocks, bs, bs)
    base = dict(ptrs=ptrs, bs=bs, scale=case.scale)
    kind = case.kind
    store = (lambda v: bref.bf16_round(np.asarray(v).astype(np.float32))) if case.p_bf16 else (lambda v: np.asarray(v).astype(np.float32))
    if kind.startswith("tie"):
        t = int(kind[3:])
        assert case.scale == TIE_SCALE
        tied, count = bsr_tie(case.name, t)
        c, gap = TIE_OFFSET["bsr"]
        if case.direction == "bwd":
            return _frozen(dict(base, p=store(np.where(tied, 1.0 / count, 0.0)), dp=_tie_dp(count, 5500 + t).astype(np.float32)))
        below = np.where(tied, 0.0, -gap * _gaps(shape, 5600 + t))
        if case.mask:
            return _frozen(dict(base, s=(below / case.scale).astype(np.float32), mask=np.full(shape, c, np.float32)))
        return _frozen(dict(base, s=((c + below) / case.scale).astype(np.float32), mask=None))
    if kind == "offset":
        c = OFFSET[np.dtype(np.float32)]
        if case.mask:
            s, mask = bref.scores("narrow", case.name), (c + _quantised(bref.random_mask(case.name))).astype(np.float32)
        else:
            assert np.frexp(case.scale)[0] == 0.5, "without a mask the offset rides on the scores: a power-of-two scale keeps z exact"
            s, mask = ((c + _quantised(bref.scores("narrow", case.name))) / case.scale).astype(np.float32), None
    else:
        s = bref.scores("narrow" if kind in ("zero_dp", "specials") else kind, case.name)
        mask = bref.random_mask(case.name) if case.mask else None
    if kind == "specials":
        s = s.copy()
        for r, i, what in _bsr_special_rows(case.name):
            if what == "nan":
                s[ptrs[r] + (ptrs[r + 1] - ptrs[r]) // 2, i, bs - 1] = np.nan
            elif what == "+inf":
                s[ptrs[r + 1] - 1, i, 0] = np.inf
            else:
                s[ptrs[r]:ptrs[r + 1], i, :] = -np.inf
    if case.direction == "fwd":
        return _frozen(dict(base, s=s, mask=mask))
    dp = np.zeros(shape, np.float32) if kind == "zero_dp" else bref.full_mantissa(np.random.default_rng(10), shape)
    return _frozen(dict(base, p=store(bref.forward(case.name, bref.z_values(s, mask, case.scale))[0]), dp=dp))


def bsr_z(case):
    op = bsr_operands(case)
    return bref.z_values(op["s"], op["mask"], case.scale)


# ---- (a) the tight tolerance
def _row_reduce(ufunc, v, rp):
    lens = np.diff(rp)
    starts = rp[:-1][lens > 0]
    return np.repeat(ufunc.reduceat(v, starts), lens[lens > 0]) if v.shape[0] else v


def _forward_rel(rp, values, exact, fast, depth, u):
    """rel per entry (see the docstring) for rows given as a CSR of `values` (the scores, or z)."""
    v = np.asarray(values, dtype=np.float64)
    p = np.asarray(exact, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        top = _row_reduce(np.maximum, np.where(np.isfinite(v), v, -np.inf), rp)
        t = np.where(p > 0, np.abs(v - top), 0.0)              # an entry of weight 0 (masked, or a dead row) costs nothing
    eps = np.where(p > 0, ((3.0 if fast else 1.0) * t + 2.0) * u, 0.0)
    others = _row_reduce(np.add, np.where(p > 0, p * eps, 0.0), rp) - p * eps
    return 1.01 * (eps * (1.0 - p) + np.maximum(others, 0.0) + gamma(depth, u) + u)


def _csr_depth(rp, group, cap_less):
    """d per entry: min(a lane's chain + the butterfly's steps, L - cap_less)."""
    lens = np.diff(rp)
    d = np.zeros(lens.shape[0])
    for r, length in enumerate(lens):
        if length:
            w, _ = csr_shape(int(length), group)
            d[r] = min(-(-int(length) // w) + int(np.log2(w)), int(length) - cap_less)
    return np.repeat(d, lens)


def _bsr_depth(name, cap_less):
    pat = bref.pattern(name)
    bs = pat.block_row_size
    counts = np.diff(np.asarray(pat.block_row_ptrs, dtype=np.int64))
    d = np.minimum(4 * -(-counts // WAVES) + int(np.log2(bs // 4)) + 3, counts * bs - cap_less).astype(np.float64)
    return np.broadcast_to(np.repeat(d, counts)[:, None, None], (pat.num_blocks, bs, bs))


@functools.lru_cache(maxsize=None)
def csr_forward_reference(case):
    """(exact [nnz] in the widest float, tolerance [nnz] float64, NaN by contract [nnz] bool)."""
    op = csr_operands(case)
    rp, s = op["row_ptrs"], op["s"]
    with np.errstate(all="ignore"):
        exact = cref.softmax_rows(rp, s)
    dead = np.isnan(exact)
    p = np.where(dead, 0.0, exact).astype(np.float64)
    u = unit(case.arith)
    rel = _forward_rel(rp, s, p, case.arith == "f32,fast", _csr_depth(rp, op["group"], 1), u)
    if case.arith == "f32,fast":
        tol = rel * p + 2.0 ** -126
    else:
        tol = rel * p + 2.0 * cref.tiny(dtype_of(case.arith)) + (half_ulp(p, 24) if case.arith == "f32,ref64" else 0.0)
    return exact, tol, dead


@functools.lru_cache(maxsize=None)
def csr_backward_reference(case):
    op = csr_operands(case)
    rp, p, dp = op["row_ptrs"], op["p"], op["dp"]
    exact, cap = cref.softmax_bwd_rows(rp, p, dp)
    ex, cap = np.abs(exact).astype(np.float64), cap.astype(np.float64)
    u = unit(case.arith)
    d = _csr_depth(rp, op["group"], 0) + (1.0 if case.arith == "f64,ref" else 0.0)
    length = cref.row_lengths(rp)
    core = gamma(2.0, u) * ex + gamma(d + 2.0, u) * np.abs(p).astype(np.float64) * cap
    if case.arith == "f32,fast":
        tol = core + (length + 2.0) * 2.0 ** -126
    elif case.arith == "f32,ref64":
        tol = half_ulp(ex, 24) + core * (1.0 + 2.0 ** -23) + cref.tiny(np.float32)
    else:
        tol = core + (length + 2.0) * cref.tiny(np.float64)
    return exact, tol, np.zeros(ex.shape, bool)


@functools.lru_cache(maxsize=None)
def bsr_forward_reference(case):
    z = bsr_z(case)
    rp, _ = bref.layout(case.name)
    with np.errstate(all="ignore"):
        exact = bref.forward(case.name, z)[0]
    dead = np.isnan(exact)
    p = np.where(dead, 0.0, exact).astype(np.float64)
    u = unit("bsr")
    rel = bref.from_rows(case.name, _forward_rel(rp, bref.to_rows(case.name, z), bref.to_rows(case.name, p), True,
                                                 bref.to_rows(case.name, _bsr_depth(case.name, 1)), u))
    tol = rel * p + 2.0 ** -126
    if case.out_bf16:
        tol = half_ulp(p, 8) + tol + 2.0 ** -126
    return exact, tol, dead


@functools.lru_cache(maxsize=None)
def bsr_backward_reference(case):
    op = bsr_operands(case)
    exact, cap = bref.backward(case.name, op["p"], op["dp"], case.scale)
    ex, cap = np.abs(exact).astype(np.float64), cap.astype(np.float64)
    u = unit("bsr")
    scale = float(np.float32(case.scale))
    d = _bsr_depth(case.name, 0)
    tol = (gamma(3.0, u) * ex + scale * gamma(d + 3.0, u) * np.abs(op["p"]).astype(np.float64) * cap
           + (bref.lengths(case.name) + 3.0) * 2.0 ** -126 * max(1.0, scale))
    if case.out_bf16:
        tol = half_ulp(ex, 8) + tol + 2.0 ** -126
    return exact, tol, np.zeros(ex.shape, bool)


def reference(case):
    table = {(CsrCase, "fwd"): csr_forward_reference, (CsrCase, "bwd"): csr_backward_reference,
             (BsrCase, "fwd"): bsr_forward_reference, (BsrCase, "bwd"): bsr_backward_reference}
    return table[type(case), case.direction](case)


def stated_bound(case):
    """The header's bound on the same elements, for the comparison `no looser than`."""
    exact, _, dead = reference(case)
    ex = np.where(dead, 0.0, exact).astype(np.float64)
    if isinstance(case, CsrCase):
        op = csr_operands(case)
        rp = op["row_ptrs"]
        if case.direction == "fwd":
            return cref.fwd_bound(dtype_of(case.arith), "fast" if case.arith.endswith("fast") else "reference", cref.row_lengths(rp),
                                  cref.spread(rp, op["s"]), ex)
        cap = cref.softmax_bwd_rows(rp, op["p"], op["dp"])[1].astype(np.float64)
        return cref.bwd_bound(dtype_of(case.arith), "fast" if case.arith.endswith("fast") else "reference", cref.row_lengths(rp), op["p"],
                              op["dp"], cap, ex)
    op = bsr_operands(case)
    if case.direction == "fwd":
        z = bsr_z(case)
        with np.errstate(all="ignore"):
            t = bref.forward(case.name, np.where(np.isnan(z) | np.isposinf(z), np.float32(0), z))[1]
        return bref.fwd_bound(case.out_bf16, bref.lengths(case.name), t, ex)
    cap = bref.backward(case.name, op["p"], op["dp"], case.scale)[1].astype(np.float64)
    return bref.bwd_bound(case.out_bf16, bref.lengths(case.name), op["p"], op["dp"], cap, case.scale, ex)


def inside(got, exact, tol, dead):
    """(ok, worst |err| / tol over the elements finite by contract); NaN exactly where the contract says NaN."""
    got = np.asarray(got)
    live = ~dead
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got.astype(LD)[live] - exact[live]).astype(np.float64)
    err = np.where(np.isnan(err), np.inf, err)
    ratio = np.where(err == 0, 0.0, err / tol[live])
    ok = bool(np.all(err <= tol[live])) and bool(np.isnan(got[dead]).all())
    return ok, float(np.max(ratio, initial=0.0))


def tight(got, case):
    """`got` (the out or ds array; bf16 results as float32 values) against the derived tolerance: (ok, worst ratio)."""
    return inside(got, *reference(case))


# ---- (b) tie rows
def tie_expected(case):
    """The exact answer of a tie case, in the out type's values (float32 / float64 array)."""
    t = int(case.kind[3:])
    if isinstance(case, CsrCase):
        op = csr_operands(case)
        dt = dtype_of(case.arith)
        tied, count = csr_tie(case.name, t)
        out = np.where(tied, 1.0 / np.maximum(count, 1), 0.0)
        if case.direction == "fwd":
            return out.astype(dt)
        dp = op["dp"].astype(np.float64)
        dot = _row_reduce(np.add, out * dp, op["row_ptrs"])
        want = out * (dp - dot)
        assert np.array_equal(want * 16.0, np.rint(want * 16.0))
        return want.astype(dt)
    op = bsr_operands(case)
    tied, count = bsr_tie(case.name, t)
    out = np.where(tied, 1.0 / count, 0.0)
    if case.direction == "bwd":
        rp, _ = bref.layout(case.name)
        dp = op["dp"].astype(np.float64)
        dot = bref.from_rows(case.name, _row_reduce(np.add, bref.to_rows(case.name, out * dp), rp))
        out = case.scale * (out * (dp - dot))
        assert np.array_equal(out * 128.0, np.rint(out * 128.0))
    out = out.astype(np.float32)
    return bref.bf16_round(out) if case.out_bf16 else out


def tie_check(got, case):
    """(ok, elements whose bits differ).  No tolerance."""
    want = tie_expected(case)
    got = np.ascontiguousarray(got, dtype=want.dtype)
    bits = np.uint32 if want.dtype == np.float32 else np.uint64
    wrong = int((got.view(bits) != want.view(bits)).sum())
    return wrong == 0, wrong


def tie_premises(arith):
    """exp(C) overflows the accumulator's type and exp(-gap) is below its subnormals, in the arithmetic's own exponential."""
    c, gap = TIE_OFFSET[arith]
    with np.errstate(over="ignore", under="ignore"):
        if arith in ("f32,fast", "bsr"):
            log2e = np.float32(1.44269504088896340736)
            return bool(np.isposinf(np.exp2(np.float32(c) * log2e))) and float(np.exp2(np.float32(-gap) * log2e)) == 0.0 \
                and c > 128 * np.log(2.0) and gap > 150 * np.log(2.0)
        return bool(np.isposinf(np.exp(np.float64(c)))) and float(np.exp(np.float64(-gap))) == 0.0 and c > 1024 * np.log(2.0) \
            and gap > 1075 * np.log(2.0)


def csr_tie_coverage(name):
    """What the tied entries of all TIES meet on a CSR pattern, asserted: every register slot, lane 0 and lane W - 1 of both
    kinds of owner, the first and the last walk step and a partial last one."""
    csr = cref.matrix(name)
    group = cref.picked_group(csr.num_rows, csr.nnz)
    rp = np.asarray(csr.row_ptrs, dtype=np.int64)
    seen = dict(group=group, slots=set(), lane0=set(), lane_last=set(), owners=set(), first_step=False, last_step=False, partial_last=False)
    for t in TIES:
        tied, _ = csr_tie(name, t)
        for lo, hi in zip(rp[:-1], rp[1:]):
            length = int(hi - lo)
            if not length:
                continue
            w, steps = csr_shape(length, group)
            pos = np.argwhere(tied[lo:hi]).ravel()
            seen["owners"].add(w)
            seen["slots"].update((pos % (cref.REGS * w) // w).tolist())
            if (pos % w == 0).any():
                seen["lane0"].add(w)
            if (pos % w == w - 1).any():
                seen["lane_last"].add(w)
            if steps > 1:
                step = pos // (cref.REGS * w)
                seen["first_step"] |= bool((step == 0).any())
                seen["last_step"] |= bool((step == steps - 1).any())
                seen["partial_last"] |= bool(length % (cref.REGS * w) != 0 and (step == steps - 1).any())
    assert seen["slots"] == set(range(cref.REGS)), seen
    assert seen["owners"] == {group, WAVE} and seen["lane0"] == seen["owners"] and seen["lane_last"] == seen["owners"], seen
    assert seen["first_step"] and seen["last_step"] and seen["partial_last"], seen
    return seen


def bsr_tie_coverage(name):
    """On a block pattern: every wave, the blocks C - 1, C and C + 1 of a walked block row, every step of a lane (element rows
    8 k .. 8 k + 7 at 32 x 32), held and walked block rows."""
    pat = bref.pattern(name)
    bs, c = pat.block_row_size, bref.HELD[pat.block_row_size]
    ptrs = np.asarray(pat.block_row_ptrs, dtype=np.int64)
    seen = dict(waves=set(), around_c=set(), steps=set(), paths=set())
    for t in TIES:
        tied, _ = bsr_tie(name, t)
        for lo, hi in zip(ptrs[:-1], ptrs[1:]):
            e, i, _ = np.nonzero(tied[lo:hi])
            if e.size:
                seen["waves"].update((e % WAVES).tolist())
                seen["steps"].update((i * (bs // 4) // WAVE).tolist())
                seen["paths"].add("walk" if hi - lo > c else "held")
                if hi - lo > c:
                    seen["around_c"].update(set(e.tolist()) & {c - 1, c, c + 1})
    assert seen["waves"] == set(range(WAVES)) and seen["around_c"] == {c - 1, c, c + 1}, seen
    assert seen["steps"] == set(range(bs * bs // 256)) and seen["paths"] == {"held", "walk"}, seen
    return seen
