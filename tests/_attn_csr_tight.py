"""A check of the fused CSR attention kernel that is DERIVED from the words of include/mispmm_attn_csr.h and not measured, and a
family of rows whose answers are exact.  Functions of (got, case): the CPU harness (tests/test_attn_csr_mutants_cpu.py) and the
GPU tests call the same code, after tests/_attn_tight.py.

WHY IT CAN BE TIGHT.  The composed tolerance (_attn_csr_ref.out_tolerance) allows for errors this kernel cannot make on these
operands: q and k are multiples of 2^-8 with sum |q||k| < 2^8 (`exact_scores` asserts it per case), so every product is a multiple
of 2^-16 and every partial sum, in any order, a multiple of 2^-16 below 2^8: 24 bits, exact in fp32.  With a power-of-two scale
(asserted) scale * s is exact too and z = fma(scale, s, bias) is ONE rounding of an exact number: its bits are determined.  So
are the batch maxima, every running maximum m, mu, t = fl(z - mu) and tau = fl(mu_old - mu_new).
THE REFERENCE is a float64 evaluation of the header's ALGORITHM with those roundings inserted: per batch b of 8 entries,
w = exp(t) with t = fl32(z - mu_b); alpha_b = exp(tau_b), exactly 1 where m_old is -Inf; the effective weight of an entry is
a = w * prod over the LATER batches of alpha; out = sum a v / sum a; lse = mu_last + log sum a.
WHAT A KERNEL THAT KEEPS THE WORDS MAY DIFFER BY, and nothing else (u = 2^-24):
  (a) the exponential: v_exp_f32 of fl(t * fl(log2 e)) against exp(t): relative (3 |t| + 2) u (the product with the rounded
      log2 e, its rounding, the instruction), and a flushed subnormal, 2^-126 absolute.  Per weight, and per rescale factor
      THAT DOES NOT CANCEL: O and l are multiplied by the same bits of alpha, so alpha_b's error is common to everything summed
      before batch b and absent from everything after: it shifts weight between the two groups and costs the entries of the
      earlier batches (3 |tau_b| + 2) u each.  A factor of exactly 1 (tau = 0, or m_old = -Inf) costs nothing: exp2(0) = 1.
  (b) the order of its fp32 sums and one rounding per rescale product and the final division: g_n = n u' / (1 - n u'),
      u' = 2^-23 (the g of tests/_attn_tight.py), on sum |terms|: a term of the numerator passes at most L fma additions, one
      rescale product per batch and the division, N = L + L/8 + 2; a term of the divisor the tree's 3 additions, a rescale and
      an addition per batch, M = 2 L/8 + 4.
There are no bf16 roundings here, so no element is flagged and nothing is left out: the check covers every element.
    E(e) = (3 |t_e| + 2) u + sum over the later batches b that move the maximum of (3 |tau_b| + 2) u
    |out - ref| <= 1.01 (sum_e p_e E_e |v_e - ref| + g_N sum_e p_e |v_e| + g_M |ref| + sum_e 2^-126 c_e (|v_e| + |ref|) / sum a),
    p = a / sum a, c_e the entry's chain of factors.  The first term is the first-order effect of relative weight errors on a
    quotient of sums (a common factor cancels, which is why |v - ref| and not |v| stands there); 1.01 covers the second order.
    |lse - ref| <= 1.01 (sum_e p_e E_e + g_M + 2^-23 (|log sum a| + |ref|))            logf to an ulp and the final addition
No constant comes from running a kernel.  Two honest variants of the restatement (_attn_csr_ref.HONEST: exponentials in float64;
sums in another order) lie inside it, and so does the restatement (tests/test_attn_csr_cpu.py).

TIE ROWS (tie_pattern, tie_operands, tie_expected, tie_check): a pattern of the `edges` row lengths on 2048 columns, unsorted.  In
every row t entries (t in 1, 2, 4, 8, 16; the largest power of two <= L where the row is shorter) share the exact maximum z = +0
and every other entry lies at least 2^10 below it -- through Q.K (scale 2^10: k spells the 6 bits of its column's class c mod 64
in +-1 and holds 1 in a seventh column, q spells the class it wants and holds -6 there, s = -2 * (bits that differ)) or through
a FINITE bias of -2^12 on s = +0 (q and k live in different columns).  The live weights are exactly 1, the others exactly +0
(exp of -2^10 and below is under the subnormals), every rescale factor is exactly 1 or exactly 0, the divisor is t, V holds
16 * {-1, 0, 1}: out is an exact mean, bit for bit, and lse = +0 bitwise at t = 1 (log t within 2 ulps elsewhere).  tie_coverage
asserts that the tied entries meet every slot of a batch, first and last batches of rows of several, and the live part of a
partial last batch."""
import functools

import numpy as np

import _attn_csr_ref as ref
from _sddmm_ref import entry_rows
from _softmax_ref import EDGE_LENGTHS, matrix

from mispmm import formats

U = 2.0 ** -24
TINY = 2.0 ** -126


def gamma(n):
    return n * 2.0 ** -23 / (1.0 - n * 2.0 ** -23)


def exact_scores(csr, q, k, scale, bias):
    """True where q, k (and a finite bias) are multiples of 2^-8, sum |q||k| < 2^8 on every stored entry and scale is a power of two."""
    for x in (q, k) + (() if bias is None else (np.where(np.isfinite(bias), bias, 0.0),)):
        if not np.array_equal(x * 256.0, np.rint(x * 256.0)):
            return False
    if np.frexp(scale)[0] != 0.5:
        return False
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    worst = 0.0
    for h in range(q.shape[0]):
        worst = max(worst, float(np.max((np.abs(ref._head(q, h)).astype(np.float64)[rows] * np.abs(ref._head(k, h)).astype(np.float64)[cols]).sum(axis=1), initial=0.0)))
    return worst < 256.0


def forward_reference(csr, q, k, v, scale, bias):
    """(out [H, M, Dv], tol_out, lse [H, M], tol_lse) in float64; rows without entries: 0 and -Inf with tolerance 0."""
    assert exact_scores(csr, q, k, scale, bias), "the scores are not exact in fp32 -- use narrower operands"
    f32, f64 = np.float32, np.float64
    idx, live, batches = ref.batch_table(csr)
    cols = np.asarray(csr.col_idxs, dtype=np.int64)
    heads, m_rows, dv = q.shape[0], csr.num_rows, v.shape[2]
    nb = idx.shape[1] // ref.BATCH
    out, tol = np.zeros((heads, m_rows, dv)), np.zeros((heads, m_rows, dv))
    lse, ltol = np.full((heads, m_rows), -np.inf), np.zeros((heads, m_rows))
    lens = np.diff(np.asarray(csr.row_ptrs, dtype=np.int64)).astype(f64)
    n_num, n_den = lens + batches + 2.0, 2.0 * batches + 4.0
    later = lambda x: np.cumsum(x[:, ::-1], axis=1)[:, ::-1] - x             # noqa: E731  the sum over the later batches
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for h in range(heads):
            z = ref.scores_f32(csr, q, k, scale, bias, h)                     # determined: one rounding of an exact number
            zs = np.where(live, z[idx], f32(-np.inf)).astype(f32).reshape(m_rows, nb, ref.BATCH)
            vk = np.where(live[:, :, None], ref._head(v, h)[cols[idx]], 0.0).astype(f64)
            top = np.maximum.accumulate(np.max(zs, axis=2), axis=1)          # the running maximum after every batch, fp32
            mu = np.where(np.isinf(top), f32(0), top).astype(f32)
            before = np.concatenate([np.full((m_rows, 1), -np.inf, f32), top[:, :-1]], axis=1)
            mu_before = np.concatenate([np.zeros((m_rows, 1), f32), mu[:, :-1]], axis=1)
            tau = np.where(np.isneginf(before), f32(0), (mu_before - mu).astype(f32)).astype(f64)     # <= 0; the factor is exp(tau)
            e_factor = np.where(tau < 0, (3.0 * np.abs(tau) + 2.0) * U, 0.0)
            chain = np.exp(later(tau))
            e_chain = later(e_factor)
            masked = np.isneginf(zs)
            arg = np.where(masked, 0.0, (zs - mu[:, :, None]).astype(f32).astype(f64))
            w = np.where(masked, 0.0, np.exp(arg))
            e_w = np.where(masked, 0.0, (3.0 * np.abs(arg) + 2.0) * U)
            a = (w * chain[:, :, None]).reshape(m_rows, -1)
            total = a.sum(axis=1, keepdims=True)
            stored = (batches > 0)[:, None]
            p = np.where(stored, a / np.where(stored, total, 1.0), 0.0)
            r = np.einsum("rk,rkc->rc", p, vk)
            e = (e_w + e_chain[:, :, None]).reshape(m_rows, -1)
            dev = np.abs(vk - r[:, None, :])
            flush = np.where(stored, TINY * np.repeat(chain, ref.BATCH, axis=1) * live / np.where(stored, total, 1.0), 0.0)
            out[h] = r
            tol[h] = np.where(stored, 1.01 * (np.einsum("rk,rkc->rc", p * e, dev) + gamma(n_num)[:, None] * np.einsum("rk,rkc->rc", p, np.abs(vk))
                                              + gamma(n_den)[:, None] * np.abs(r) + np.einsum("rk,rkc->rc", flush, np.abs(vk) + np.abs(r)[:, None, :]))
                              + 1e-30, 0.0)
            log_total = np.log(np.where(stored, total, 1.0))[:, 0]
            lse[h] = np.where(stored[:, 0], mu[:, -1].astype(f64) + log_total, -np.inf)
            ltol[h] = np.where(stored[:, 0], 1.01 * ((p * e).sum(axis=1) + gamma(n_den) + 2.0 ** -23 * (np.abs(log_total) + np.abs(np.where(stored[:, 0], lse[h], 0.0))))
                               + 1e-30, 0.0)
    return out, tol, lse, ltol


@functools.lru_cache(maxsize=None)
def case_reference(case):
    op = ref.operands(case)
    return forward_reference(matrix(case.name), op["q"], op["k"], op["v"], op["scale"], op["bias"])


def _worst(got, want, tol):
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, np.where(np.isnan(err), np.inf, err / np.where(tol > 0, tol, 1.0)))
        ratio = np.where((tol == 0) & (err > 0), np.inf, ratio)
    return bool(np.all(err <= tol)), float(np.max(ratio, initial=0.0))


def tight_forward(got, case):
    """out and lse of `case` against the derived reference: (ok, (worst out, worst lse)).  Every element is covered; a row
    without entries must be +0 and -Inf."""
    out, tol, lse, ltol = case_reference(case)
    ok_out, worst_out = _worst(got["out"], out, tol)
    stored = np.isfinite(lse)
    ok_lse, worst_lse = _worst(got["lse"][stored], lse[stored], ltol[stored])
    return ok_out and ok_lse and bool(np.array_equal(np.isneginf(got["lse"]), ~stored)), (worst_out, worst_lse)


# ---- tie rows
TIES = (1, 2, 4, 8, 16)
TIE_CLASSES, TIE_COLS = 64, 2048
TIE_D, TIE_DV = 8, 8


def _tie_count(t, length):
    return 0 if length == 0 else min(t, 1 << (int(length).bit_length() - 1))


@functools.lru_cache(maxsize=None)
def tie_pattern(t):
    """(csr, tied [nnz] bool, wanted class per row): rows of the `edges` lengths; the tied entries of row r hold columns of
    class (7 r + 3) mod 64, all others columns of other classes; no column twice in a row, unsorted.  Where the tied entries sit:
    r mod 3 == 0: from position (5 r) mod 8 on, wrapping at the row's end; 1: the row's last entries; 2: anywhere."""
    rng = np.random.default_rng(5000 + t)
    lens = np.array(EDGE_LENGTHS, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    cols, tied, wanted = np.zeros(ptr[-1], np.int64), np.zeros(ptr[-1], bool), np.zeros(lens.shape[0], np.int64)
    for r, length in enumerate(lens):
        n = _tie_count(t, length)
        wanted[r] = (7 * r + 3) % TIE_CLASSES
        if n == 0:
            continue
        if r % 3 == 0:
            pos = (5 * r % 8 + np.arange(n)) % length
        elif r % 3 == 1:
            pos = length - n + np.arange(n)
        else:
            pos = rng.choice(length, n, replace=False)
        mine = np.zeros(length, bool)
        mine[pos] = True
        own = wanted[r] + TIE_CLASSES * rng.choice(TIE_COLS // TIE_CLASSES, n, replace=False)
        others = np.array([c for c in range(TIE_COLS) if c % TIE_CLASSES != wanted[r]])
        row_cols = np.zeros(length, np.int64)
        row_cols[mine] = own
        row_cols[~mine] = rng.choice(others, length - n, replace=False)
        cols[ptr[r]:ptr[r + 1]] = row_cols
        tied[ptr[r]:ptr[r + 1]] = mine
    csr = formats.CSR(lens.shape[0], TIE_COLS, ptr.astype(np.uint32), cols.astype(np.uint32), np.ones(int(ptr[-1]), np.float32))
    return csr, tied, wanted


@functools.lru_cache(maxsize=None)
def tie_operands(t, through_bias):
    """dict(q [1, M, 8], k [1, K, 8], v [1, K, 8], bias, scale); read-only."""
    csr, tied, wanted = tie_pattern(t)
    rng = np.random.default_rng(6000 + 2 * t + through_bias)
    bits = lambda x: np.array([1.0 if (x >> b) & 1 else -1.0 for b in range(6)], np.float32)   # noqa: E731
    q, k = np.zeros((csr.num_rows, TIE_D), np.float32), np.zeros((csr.num_cols, TIE_D), np.float32)
    if through_bias:
        q[:, :4] = rng.choice(np.array([-1.0, 1.0], np.float32), (csr.num_rows, 4))
        k[:, 4:] = rng.choice(np.array([-1.0, 1.0], np.float32), (csr.num_cols, 4))
        bias, scale = np.where(tied, 0.0, -4096.0).astype(np.float32), 1.0
    else:
        for c in range(csr.num_cols):
            k[c, :6], k[c, 6] = bits(c % TIE_CLASSES), 1.0
        for r in range(csr.num_rows):
            q[r, :6], q[r, 6] = bits(int(wanted[r])), -6.0
        bias, scale = None, 1024.0
    v = 16.0 * rng.integers(-1, 2, (csr.num_cols, TIE_DV)).astype(np.float32)
    res = dict(q=q[None], k=k[None], v=v[None], bias=bias, scale=scale)
    for x in res.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def tie_expected(t, through_bias):
    """(out [1, M, 8], lse [1, M]) in float64, and the scores checked to be what the docstring says."""
    csr, tied, _ = tie_pattern(t)
    op = tie_operands(t, through_bias)
    z, _ = ref.scores_f64(csr, op["q"], op["k"], op["scale"], op["bias"], 0)
    assert np.all(z[tied] == 0.0) and np.all(z[~tied] <= -1024.0), "tie rows: the scores are not what they are meant to be"
    rows, cols = entry_rows(csr.row_ptrs), np.asarray(csr.col_idxs, dtype=np.int64)
    count = np.zeros(csr.num_rows)
    np.add.at(count, rows, tied.astype(np.float64))
    lens = np.diff(np.asarray(csr.row_ptrs, dtype=np.int64))
    assert np.array_equal(count, [_tie_count(t, n) for n in lens])
    out = np.zeros((csr.num_rows, TIE_DV))
    np.add.at(out, rows[tied], op["v"][0].astype(np.float64)[cols[tied]])
    out = out / np.maximum(count, 1.0)[:, None] + 0.0
    assert np.array_equal(out, np.rint(out))
    with np.errstate(divide="ignore"):
        return out[None], np.log(count)[None]


def tie_coverage(t):
    """What the tied entries meet: slots of a batch, the first and the last batch of rows of several batches, the live part of
    a partial last batch."""
    csr, tied, _ = tie_pattern(t)
    ptrs = np.asarray(csr.row_ptrs, dtype=np.int64)
    seen = dict(slots=set(), first_batch=False, last_batch=False, partial_last=False)
    for lo, hi in zip(ptrs[:-1], ptrs[1:]):
        pos = np.argwhere(tied[lo:hi]).ravel()
        nb = -(-(hi - lo) // ref.BATCH)
        seen["slots"].update((pos % ref.BATCH).tolist())
        if nb > 1 and pos.size:
            seen["first_batch"] |= bool((pos // ref.BATCH == 0).any())
            seen["last_batch"] |= bool((pos // ref.BATCH == nb - 1).any())
            seen["partial_last"] |= bool((hi - lo) % ref.BATCH != 0 and (pos // ref.BATCH == nb - 1).any())
    return seen


def tie_check(got, t, through_bias):
    """(ok, elements that differ): out bit for bit; lse bit for bit where a row has one tied entry (+0) or none (-Inf), within
    two fp32 ulps of log t elsewhere (logf, which no grid makes exact)."""
    out, lse = tie_expected(t, through_bias)
    wrong = int((np.ascontiguousarray(got["out"], dtype=np.float32).view(np.uint32) != out.astype(np.float32).view(np.uint32)).sum())
    exact = ~(lse > 0)
    wrong += int((np.ascontiguousarray(got["lse"], dtype=np.float32)[exact].view(np.uint32) != lse[exact].astype(np.float32).view(np.uint32)).sum())
    wrong += int((~(np.abs(got["lse"][~exact].astype(np.float64) - lse[~exact]) <= 2.0 ** -22 * lse[~exact])).sum())
    return wrong == 0, wrong
