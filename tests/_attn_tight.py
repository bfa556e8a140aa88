"""A differential check of the two fused attention kernels that is DERIVED from the contract and not measured, and a family of
operands whose answers are exact.  Functions of (got, case) as tests/_attn_checks.py has them: the CPU harness and the GPU tests
call the same code.

WHY IT CAN BE TIGHT.  The composed tolerances (out_composed, lse_bound, bwd_composed) allow for errors the kernels cannot make:
  * S and dP are EXACT.  The operands are bf16 numbers of magnitude in [0.5, 2): multiples of 2^-8, so every product is a multiple
    of 2^-16, and where sum |q||k| < 2^8 (sum |g||v| < 2^8) every partial sum, in any order, is a multiple of 2^-16 below 2^8: 24
    bits, exact in fp32.  `exact_products` asserts the condition on every stored element of a case.
  * z is one fma (or one product) of exact inputs: its bits are determined.  So are the running maxima, mu, and z - mu.
  * delta's order is in the contract (delta_f32): its bits are determined by grad_out and the stored out.
What is left between a kernel that keeps the contract and a float64 evaluation of the contract with its roundings inserted:
  (a) the exponential: v_exp_f32 of fl(t * log2 e) against exp.  The header's count: relative (3 t + 2) u, t = |argument|, u = 2^-24
      (the difference, the product with the rounded log2 e, the instruction), and a flushed subnormal, 2^-126.
  (b) the order of the fp32 sums inside the second products' MFMAs, the rescalings and the running sums: g_n = n 2^-23 / (1 - n 2^-23)
      on sum |terms|, n the number of roundings a term passes -- the g_n and the u of tests/_sddmm_bsr_ref.py::bound.
  (c) roundings to bf16 that FLIP: the kernel rounds a weight w^ (a dS) that lies within (a) of the reference's w.  Rounding is
      monotone, so bf16(w^) lies between bf16(w (1 - e) - 2^-126) and bf16(w (1 + e) + 2^-126).  Where the two ends round alike --
      almost everywhere -- the kernel's bf16 weight is DETERMINED and gets no allowance at all; where they differ the element
      is `flagged` and is allowed the distance to the further end, one bf16 ulp, propagated linearly into out, dq, dk, dv.
The tolerance is (b) + (c) + the first-order effect of (a) where it does not cancel (the chain of rescale factors, lse), times
1.01 for second-order terms, and nothing else.  No constant comes from running a kernel.  A case whose flagged share of live
elements exceeds FLAGGED_CAP is refused: change the operands, never the cap.

FORWARD.  Reference: per 32-key step s with mu_s the running maximum (exact), w = exp(z - mu_s) in float64, w^ = bf16(w),
c_s = prod over the later steps of exp(mu_old - mu_new); effective weight a = w^ c_s; out = sum a v / sum a; lse = mu + log sum w c_s.
The kernel multiplies O and l by the SAME computed factor, but a step's terms take the factors of the later steps only: an error
of a factor shifts weight between earlier and later steps.  Relative allowance of an effective weight:
    E = sum over the later steps that move the maximum of ((3 tau + 2) u),  tau = mu_new - mu_old        (a factor of exactly 1 costs 0)
      + (flagged: |bf16 end - w^| / w^)
    |out - ref| <= sum p E |v - ref| + g_N sum p |v| + g_M |ref|,   p = a / sum a
N = the keys of the padded row + 2 per step + 2 (numerator: the MFMA's sum, a rescale and an addition per step, 1 / l and the last
product), M = 8 per step + 2 per step + 2 (divisor: a lane's 8 additions, rescale and addition per step, the meeting).
    |lse - ref| <= sum P (E_w + E_chain) + g_M + 2^-23 (|log lx| + |ref|),   P = w c / lx,  E_w = (3 t + 2) u
logf to an ulp and the final addition.  A bf16 out: the fp32 interval [ref - tol, ref + tol] rounded at both ends (monotone again).

BACKWARD, on the kernel's OWN stored out and lse (the check isolates the backward): P = exp(z - lse), E_P = (3 t + 2) u;
x = fl32(dP - delta) is determined; dS = P x scale in float64, E_dS = E_P + 2 u (the two fp32 products); P^ = bf16(P), dS^ = bf16(dS),
flags and allowances f as in (c).
    |dQ - ref| <= g_n sum |dS^||K| + sum f_dS |K|,  n = L + L / 32 + 1;  dK the same down the column with |Q|;  dV with P^, f_P, |dO|.
A bf16 gradient: the interval rounded at both ends.

TIE ROWS (tie_operands, tie_expected): operands on a small integer grid, a power-of-two scale, integer V and dO, t in {1, 2, 4, 8, 16}
keys sharing the exact maximum of a matrix row and every other key at least 2^10 below it -- through Q.K itself or through a
FINITE additive mask of -2^12.  The live weights are exactly 1 (2^0 = 1), the others exactly +0 (exp of -2^10 and below is under
the subnormals), the divisor is t and 1 / t is exact, out is the mean of t integer rows of V; lse = the maximum bitwise at t = 1;
P, dS and the three gradients are exact.  Bit for bit, no tolerance."""
import dataclasses
import functools

import numpy as np

import _attn_fused_bwd_ref as bwd_ref
from _attn_checks import empty_block_rows
from _softmax_bsr_ref import fma32

U = 2.0 ** -24
FLAGGED_CAP = 0.01
TINY = 2.0 ** -126


def gamma(n):
    return n * 2.0 ** -23 / (1.0 - n * 2.0 ** -23)


def bf16_of_real(x):
    """The bf16 number nearest to a real (float64) x, ties to even, subnormals of bf16 included; float64."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    quantum = np.ldexp(1.0, np.maximum(e - 8, -133))
    return np.rint(x / quantum) * quantum


def _ends(centre, rel):
    """(bf16 of the centre, allowance): where bf16 of an fp32 number within rel (relative) + 2^-126 of `centre` can land."""
    mid = bf16_of_real(centre)
    spread = np.abs(centre) * rel * 1.01 + TINY
    lo, hi = bf16_of_real(centre - spread), bf16_of_real(centre + spread)
    return mid, np.maximum(np.abs(hi - mid), np.abs(lo - mid))


def _inside(got, ref, tol, as_bf16):
    """(ok, worst): fp32: |got - ref| <= tol, worst = max |got - ref| / tol.  bf16: got between the roundings of ref - tol and of
    ref + tol; worst = 0 where got is the rounded reference itself, 0.5 where it is another bf16 number of the interval (a flip the
    fp32 tolerance allows), and 1 + (the distance past the interval) / tol outside."""
    got = got.astype(np.float64)
    if not as_bf16:
        err = np.abs(got - ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            return bool(np.all(err <= tol)), float(np.max(np.where(err == 0, 0.0, np.where(np.isnan(err), np.inf, err / tol)), initial=0.0))
    lo, hi = bf16_of_real(ref - tol), bf16_of_real(ref + tol)
    out = np.maximum(np.maximum(lo - got, got - hi), 0.0)
    bad = ~((got >= lo) & (got <= hi))
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.max(np.where(bad, 1.0 + out / tol, np.where(got == bf16_of_real(ref), 0.0, 0.5)), initial=0.0))
    return bool(not bad.any()), worst


# ---- exactness of S and dP
def exact_products(case):
    """True where every stored element has sum |q||k| < 2^8 and sum |g||v| < 2^8 on bf16 operands that are multiples of 2^-8."""
    q, k, v, _ = case.arrays
    g = case.g_bf16
    b = bwd_ref._blocks(case.name)
    for x in (q, k, v, g):
        if not np.array_equal(x * 256.0, np.rint(x * 256.0)):
            return False
    f64 = np.float64
    worst = float(np.max(b.sampled(np.abs(q).astype(f64), np.abs(k).astype(f64)), initial=0.0))
    if g.any():
        worst = max(worst, float(np.max(b.sampled(np.abs(g).astype(f64), np.abs(v).astype(f64)), initial=0.0)))
    return worst < 256.0


# ---- the forward
@functools.lru_cache(maxsize=None)
def forward_reference(case):
    """(out [M, Dv], tol_out, lse [M], tol_lse, flagged share) in float64 on the case without its out type; read-only."""
    assert not case.out_bf16
    assert exact_products(case), f"{case.id}: S is not exact in fp32 -- use narrower operands"
    f32, f64 = np.float32, np.float64
    bsr = case.bsr
    bs = bsr.block_row_size
    q, k, v, _ = case.arrays
    mask, scale = case.mask, f32(case.scale_value)
    out, tol = np.zeros((bsr.num_rows, case.dv)), np.zeros((bsr.num_rows, case.dv))
    lse, ltol = np.full(bsr.num_rows, -np.inf), np.zeros(bsr.num_rows)
    flagged = live = 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r, lo, hi, keys in bwd_ref._block_rows(bsr):
            if hi == lo:
                continue
            rows = slice(r * bs, (r + 1) * bs)
            s = (q[rows].astype(f64) @ k[keys].T.astype(f64)).astype(f32)            # exact
            z = scale * s if mask is None else fma32(scale, s, mask[lo:hi].transpose(1, 0, 2).reshape(bs, -1))
            pad = -keys.shape[0] % 32
            z = np.concatenate([z, np.full((bs, pad), -np.inf, f32)], axis=1).astype(f64)
            vk = np.concatenate([v[keys].astype(f64), np.zeros((pad, case.dv))], axis=0)
            steps = z.shape[1] // 32
            zs = z.reshape(bs, steps, 32)
            top = np.maximum.accumulate(np.max(zs, axis=2), axis=1)                  # running maximum after every step
            mu = np.where(np.isinf(top), 0.0, top)
            before = np.concatenate([np.full((bs, 1), -np.inf), top[:, :-1]], axis=1)
            mu_before = np.concatenate([np.zeros((bs, 1)), mu[:, :-1]], axis=1)
            tau = np.where(np.isneginf(before), 0.0, mu - mu_before)                 # the factor is exp(-tau); exactly 1 at tau = 0
            e_factor = np.where(tau > 0, (3.0 * tau + 2.0) * U, 0.0)
            # what the later steps do to a step's terms: chain[s] = prod_{s' > s} exp(-tau[s']) = exp(mu[s] - mu[last]) where both count
            later = lambda x: np.cumsum(x[:, ::-1], axis=1)[:, ::-1] - x             # noqa: E731
            chain = np.exp(-later(tau))
            e_chain = later(e_factor)
            arg = zs - mu[:, :, None]
            w = np.where(np.isneginf(zs), 0.0, np.exp(arg))
            e_w = np.where(np.isneginf(zs), 0.0, (3.0 * np.abs(np.where(np.isneginf(zs), 0.0, arg)) + 2.0) * U)
            wb, slack = _ends(w, e_w)
            slack = np.where(np.isneginf(zs), 0.0, slack)                            # exp2(-Inf) is exactly +0
            live += int(np.isfinite(zs).sum())
            flagged += int((slack > 0).sum())
            a = (wb * chain[:, :, None]).reshape(bs, -1)
            total = a.sum(axis=1, keepdims=True)
            p = a / total
            ref = p @ vk
            with np.errstate(invalid="ignore", divide="ignore"):
                e = (e_chain[:, :, None] + np.where(wb > 0, slack / wb, 0.0)).reshape(bs, -1)
            n_num, n_den = z.shape[1] + 2.0 * steps + 2.0, 10.0 * steps + 2.0
            dev = np.abs(vk[None, :, :] - ref[:, None, :])                           # [row, key, column]
            out[rows] = ref
            tol[rows] = 1.01 * (np.einsum("rk,rkc->rc", p * e, dev) + np.einsum("rk,rkc->rc", slack.reshape(bs, -1) * (wb.reshape(bs, -1) == 0)
                                                                                   * chain.repeat(32, axis=1) / total, np.abs(vk)[None] + np.abs(ref)[:, None])
                                + gamma(n_num) * (p @ np.abs(vk)) + gamma(n_den) * np.abs(ref)) + 1e-30
            wx = (w * chain[:, :, None]).reshape(bs, -1)
            lx = wx.sum(axis=1)
            share = wx / lx[:, None]
            lse[rows] = mu[:, -1] + np.log(lx)
            ltol[rows] = 1.01 * ((share * (e_w.reshape(bs, -1) + e_chain.repeat(32, axis=1))).sum(axis=1) + gamma(n_den)
                                 + 2.0 ** -23 * (np.abs(np.log(lx)) + np.abs(lse[rows]))) + 1e-30
    return out, tol, lse, ltol, (flagged / live if live else 0.0)


def tight_forward(got, case):
    """out and lse against the contract-level reference inside the derived tolerance.  None where the case is not one of exact
    products.  (ok, (worst out, worst lse, flagged share))."""
    if "dq" in got or case.const_v or case.wide != 1:
        return None
    ref, tol, lse, ltol, share = forward_reference(dataclasses.replace(case, out_bf16=False, grads_bf16=False, g32=False))
    assert share <= FLAGGED_CAP, f"{case.id}: {share:.3%} of the live weights flagged -- change the operands, not the cap"
    ok_out, worst_out = _inside(got["out"], ref, tol, case.out_bf16)
    stored = ~empty_block_rows(case.bsr)
    ok_lse, worst_lse = _inside(got["lse"][stored], lse[stored], ltol[stored], False)
    return ok_out and ok_lse and bool(np.array_equal(np.isneginf(got["lse"]), ~stored)), (worst_out, worst_lse, share)


# ---- the backward
def backward_reference(case, out, lse):
    """((dq, dk, dv), (tol_dq, tol_dk, tol_dv), (flagged share of P, of dS)) in float64 from the stored out and lse (float32 arrays)."""
    assert exact_products(case), f"{case.id}: S or dP is not exact in fp32 -- use narrower operands"
    f32, f64 = np.float32, np.float64
    b = bwd_ref._blocks(case.name)
    q, k, v, _ = case.arrays
    g = case.g_bf16
    mask, scale = case.mask, f32(case.scale_value)
    delta = bwd_ref.delta_f32(g, np.ascontiguousarray(out, dtype=f32))                 # the contract fixes its order: bits
    q64, k64, v64, g64 = (x.astype(f64) for x in (q, k, v, g))
    with np.errstate(invalid="ignore", over="ignore"):
        s = b.sampled(q64, k64).astype(f32)                                            # exact
        z = (scale * s if mask is None else fma32(scale, s, mask)).astype(f64)
        live = np.isfinite(z)
        arg = np.where(live, z - b.of_row(lse.astype(f64)), 0.0)
        p = np.where(live, np.exp(arg), 0.0)
        e_p = np.where(live, (3.0 * np.abs(arg) + 2.0) * U, 0.0)
        x = (b.sampled(g64, v64).astype(f32) - b.of_row(delta).astype(f32)).astype(f64)    # fl32(dP - delta): determined
        ds = p * x * f64(scale)
        pb, f_p = _ends(p, e_p)
        dsb, f_ds = _ends(ds, e_p + 2.0 * U)
    f_p, f_ds = np.where(live, f_p, 0.0), np.where(live, f_ds, 0.0)
    pb, dsb = np.where(live, pb, 0.0), np.where(live, dsb, 0.0)
    n_live = max(int(live.sum()), 1)
    shares = (float((f_p > 0).sum()) / n_live, float((f_ds > 0).sum()) / n_live)
    g_row = gamma(b.n_row + b.n_row / 32.0 + 1.0)[:, None]
    g_col = gamma(b.n_col + b.n_col / 32.0 + 1.0)[:, None]
    refs = (b.times(dsb, k64), b.times_t(dsb, q64), b.times_t(pb, g64))
    tols = (g_row * b.times(np.abs(dsb), np.abs(k64)) + b.times(f_ds, np.abs(k64)),
            g_col * b.times_t(np.abs(dsb), np.abs(q64)) + b.times_t(f_ds, np.abs(q64)),
            g_col * b.times_t(pb, np.abs(g64)) + b.times_t(f_p, np.abs(g64)))
    return refs, tuple(1.01 * t + 1e-30 for t in tols), shares


def tight_backward(got, case):
    """dq, dk, dv against the contract-level reference on the stored out and lse in got.  (ok, (worst dq, dk, dv, share P, share dS))."""
    if "dq" not in got or case.wide != 1 or case.kind == "blankcols":
        return None
    refs, tols, shares = backward_reference(case, got["out"], got["lse"])
    assert max(shares) <= FLAGGED_CAP, f"{case.id}: {shares} of the live P / dS flagged -- change the operands, not the cap"
    res = [_inside(got[n], r, t, case.grads_bf16) for n, r, t in zip(("dq", "dk", "dv"), refs, tols)]
    return all(ok for ok, _ in res), tuple(w for _, w in res) + shares




# ---- tie rows
TIES = (1, 2, 4, 8, 16)
TIE_SCALE = 1024.0
TIE_WIDTHS = {16: (16, 72), 32: (72, 16)}          # (D, Dv) per block size: D2 with T8 / V4, D4 with T4 / V2


@functools.lru_cache(maxsize=None)
def tie_operands(name, t, through_mask):
    """dict(q, k, v, g, mask, scale, tied) on pattern `name` (one of the six); integers throughout, read-only.
    tied [num_blocks, bS, bS] (block, query, key): the t keys of a matrix row that share its maximum z = +0; every other stored key
    has z <= -2048.  For the j-th non-empty block row and its query i the tied keys are the aligned group
    (5 i + 3 j) mod (bS / t) of t consecutive keys of ONE block: the row's first, its last or block (7 i + j) mod n, by (i + j) mod 3
    -- so that over a pattern the first and the last step, every one of the 32 positions of a step, the live half of an odd 16 x 16
    row's last step and the first and last query of a column-pass step are met (tie_coverage counts them).
    Through Q.K (scale 2^10, no mask): K's row spells its block column (7 columns) and the high bits of its position in the block
    (log2 bS - log2 t columns) in +-1, Q's row spells the block column and the group it wants, and one more column holds -(the number
    of spelt bits) in Q and 1 in K: s = 0 where every bit agrees and <= -2 elsewhere.  Of the remaining columns one half is +-1 in Q and 0
    in K, the other +-1 in K and 0 in Q: they feed dK and dQ and leave the scores alone.
    Through the mask: Q is +-1 in its first D / 2 columns and K in its last, s = +0 everywhere, and the mask is 0 on the tied keys
    and -2^12 on all others -- FINITE, so the ordinary path runs.
    V: 16 * {-1, 0, 1}: a mean of t <= 16 rows is an integer.  dO: +-1 in 8 columns of a row, 0 elsewhere: dP - delta is an integer of
    magnitude <= 256, so dS = (dP - delta) 2^10 / t is a bf16 number."""
    a, at, perm = bwd_ref.bwd_pattern(name)
    bs = a.block_row_size
    d, dv = TIE_WIDTHS[bs]
    assert t in TIES and t <= bs
    rng = np.random.default_rng(4000 + 10 * t + through_mask)
    ptrs = np.asarray(a.block_row_ptrs, dtype=np.int64)
    cols = np.asarray(a.block_col_idxs, dtype=np.int64)
    groups = bs // t
    pos_bits = int(np.log2(groups))
    sign = lambda value, bits: np.array([1.0 if (value >> b) & 1 else -1.0 for b in range(bits)], np.float32)   # noqa: E731
    tied = np.zeros((a.num_blocks, bs, bs), bool)
    q = rng.choice(np.array([-1.0, 1.0], np.float32), (a.num_rows, d))
    k = np.zeros((a.num_cols, d), np.float32)
    if through_mask:
        q[:, d // 2:] = 0
        k[:, d // 2:] = rng.choice(np.array([-1.0, 1.0], np.float32), (a.num_cols, d - d // 2))
    else:
        used = 7 + pos_bits + 1
        free = used + (d - used) // 2                           # columns used .. free - 1: Q's alone; free .. d - 1: K's alone
        assert a.num_cols // bs <= 128 and free < d
        q[:, free:] = 0
        k[:, free:] = rng.choice(np.array([-1.0, 1.0], np.float32), (a.num_cols, d - free))
        for key in range(a.num_cols):
            k[key, :7] = sign(key // bs, 7)
            k[key, 7:7 + pos_bits] = sign((key % bs) // t, pos_bits)
            k[key, 7 + pos_bits] = 1.0
    j = 0
    for r, (lo, hi) in enumerate(zip(ptrs[:-1], ptrs[1:])):
        n = hi - lo
        if n == 0:
            continue
        for i in range(bs):
            block = lo + (0, n - 1, (7 * i + j) % n)[(i + j) % 3]
            group = (5 * i + 3 * j) % groups
            tied[block, i, group * t:(group + 1) * t] = True
            if not through_mask:
                row = r * bs + i
                q[row, :7] = sign(int(cols[block]), 7)
                q[row, 7:7 + pos_bits] = sign(group, pos_bits)
                q[row, 7 + pos_bits] = -(7.0 + pos_bits)
        j += 1
    v = 16.0 * rng.integers(-1, 2, (a.num_cols, dv)).astype(np.float32)
    g = np.zeros((a.num_rows, dv), np.float32)
    for row in range(a.num_rows):
        g[row, rng.choice(dv, 8, replace=False)] = rng.choice(np.array([-1.0, 1.0], np.float32), 8)
    mask = np.where(tied, 0.0, -4096.0).astype(np.float32) if through_mask else None
    res = dict(q=q, k=k, v=v, g=g, mask=mask, scale=TIE_SCALE, tied=tied)
    for x in res.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def tie_expected(name, t, through_mask):
    """dict(out, lse, dq, dk, dv) in float64, every one a number fp32 holds (asserted), and z_ok: the scores are what the docstring of
    tie_operands says.  lse = log t on the stored rows (+0 at t = 1, the maximum, bitwise), -Inf on the empty ones."""
    op = tie_operands(name, t, through_mask)
    b = bwd_ref._blocks(name)
    f64 = np.float64
    q, k, v, g = (op[n].astype(f64) for n in ("q", "k", "v", "g"))
    tied = op["tied"]
    z = op["scale"] * b.sampled(q, k) + (0.0 if op["mask"] is None else op["mask"].astype(f64))
    assert np.all(z[tied] == 0.0) and np.all(z[~tied] <= -1024.0), "tie rows: the scores are not what they are meant to be"
    p = tied.astype(f64) / t
    out = b.times(p, v)
    stored = ~empty_block_rows(b.a)
    assert np.array_equal(b.row_reduce(tied.astype(f64), np.add, 0.0) == t, stored)
    lse = np.where(stored, np.log(float(t)), -np.inf)
    delta = np.sum(g * out, axis=1)
    ds = op["scale"] * p * (b.sampled(g, v) - b.of_row(delta))
    assert np.array_equal(ds, bf16_of_real(ds)) and np.array_equal(p, bf16_of_real(p)), "tie rows: P or dS is no bf16 number"
    res = dict(out=out, lse=lse, dq=b.times(ds, k), dk=b.times_t(ds, q), dv=b.times_t(p, g))
    # every partial sum of the second products is exact in fp32 in any order: multiples of a common quantum below 2^24 of it
    for terms, other, quantum in ((np.abs(ds), np.abs(k), op["scale"] / 16), (np.abs(p), np.abs(v), 1.0)):
        assert np.max(b.times(terms, other)) / quantum < 2.0 ** 24
    for terms, other, quantum in ((np.abs(ds), np.abs(q), op["scale"] / 16), (np.abs(p), np.abs(g), 1.0 / 16)):
        assert np.max(b.times_t(terms, other)) / quantum < 2.0 ** 24
    for n in ("out", "dq", "dk", "dv"):
        res[n] = res[n] + 0.0                                   # -0 -> +0: every accumulator starts from +0
        assert np.array_equal(res[n], res[n].astype(np.float32).astype(f64)), n
    return res


def tie_coverage(names, t, through_mask):
    """What the tied keys of the patterns `names` meet: positions of a 32-key step, first / last steps, the live half of a half step,
    first / last query of a 32-query step of the column pass."""
    seen = dict(positions=set(), first_step=False, last_step=False, half_step=False, first_query=False, last_query=False)
    for name in names:
        a, at, perm = bwd_ref.bwd_pattern(name)
        bs = a.block_row_size
        tied = tie_operands(name, t, through_mask)["tied"]
        ptrs = np.asarray(a.block_row_ptrs, dtype=np.int64)
        for lo, hi in zip(ptrs[:-1], ptrs[1:]):
            for e in range(lo, hi):
                keys = np.argwhere(tied[e].any(axis=0)).ravel() + (e - lo) * bs
                if keys.size == 0:
                    continue
                seen["positions"].update((keys % 32).tolist())
                steps = -(-(hi - lo) * bs // 32)
                seen["first_step"] |= bool((keys // 32 == 0).any()) and steps > 1
                seen["last_step"] |= bool((keys // 32 == steps - 1).any()) and steps > 1
                seen["half_step"] |= bs == 16 and (hi - lo) % 2 == 1 and hi - lo > 1 and e == hi - 1
        tptrs = np.asarray(at.block_row_ptrs, dtype=np.int64)
        for lo, hi in zip(tptrs[:-1], tptrs[1:]):
            for e in range(lo, hi):
                queries = np.argwhere(tied[perm[e]].any(axis=1)).ravel() + (e - lo) * bs
                seen["first_query"] |= bool((queries % 32 == 0).any())
                seen["last_query"] |= bool((queries % 32 == 31).any())
    return seen


def _same_bits(got, want, as_bf16):
    want = bf16_of_real(want) if as_bf16 else want
    return int((np.ascontiguousarray(got, dtype=np.float32).view(np.uint32) != want.astype(np.float32).view(np.uint32)).sum())


def tie_forward(got, name, t, through_mask, out_bf16=False):
    """(ok, elements that differ): out bit for bit; lse bit for bit at t = 1 (+0, the maximum) and on the empty rows (-Inf), and within
    two fp32 ulps of log t otherwise (logf, which no integer grid makes exact)."""
    want = tie_expected(name, t, through_mask)
    wrong = _same_bits(got["out"], want["out"], out_bf16)
    lse = got["lse"]
    if t == 1:
        wrong += _same_bits(lse, want["lse"], False)
    else:
        stored = np.isfinite(want["lse"])
        wrong += int((~np.isneginf(lse[~stored])).sum()) + int((~(np.abs(lse[stored].astype(np.float64) - want["lse"][stored]) <= 2.0 ** -22 * np.log(t))).sum())
    return wrong == 0, wrong


def tie_backward(got, name, t, through_mask, grads_bf16=False):
    """(ok, elements that differ): dq, dk, dv bit for bit (a bf16 gradient: the exact fp32 sum rounded once)."""
    want = tie_expected(name, t, through_mask)
    wrong = sum(_same_bits(got[n], want[n], grads_bf16) for n in ("dq", "dk", "dv"))
    return wrong == 0, wrong
