"""The fused block-sparse attention forward (include/mispmm_attn.h) for the tests: the table of kernel tags with the smallest
shape that reaches each, operands and masks, the float64 references, the lse tolerance, and the algorithm AS BUILT restated in
numpy float32 -- 32-key steps, one running maximum per matrix row, weights rounded to bf16 before the second product, fp32
rescaling after every step, the divisor summed from the rounded weights by four lanes that meet at the end.

Tolerances.  out is held to the `out` component of tests/test_gpu_softmax_bsr.py::_attention_tolerances, the composed bound of
the three-launch chain, and to nothing wider: its 2^-8 P term for the rounding of P to bf16 is twice what round-to-nearest
needs (2^-9); the fused kernel spends the other half on its divisor, the sum of the ROUNDED weights (off by at most 2^-9
relative), and the two roundings per step of the rescale fit the chain's any-order dot-product term g_L.
lse (float64 logsumexp of the float64 z as reference):
    |lse - exact| <= 1.01 (E_z + (L + 8 T + 16) u + 2 u (|exact| + ln L + 1)),   u = 2^-24
E_z: the largest error of a z of the row -- the SDDMM bound of mispmm.h through the factor scale, plus the rounded scale and the
fma's rounding, exactly as _attention_tolerances forms it (logsumexp moves by at most the largest change of an argument); the
second term bounds the relative error of the fp32 sum of exponentials (header of mispmm_attn.h: every term passes at most
L / 16 + 11 roundings, (3 T + 2) u for its exponential, (3 T + L / 16) u for the chain of rescale factors); the third is logf to
an ulp and the final addition.  1.01 covers second-order terms, as in _attention_tolerances.

fused_rows / fused_f32 take `fault=`: a name of tests/_attn_mutants.py, a deliberate breach of the header put into THIS code and
not a copy of it, for tests/test_attn_mutants_cpu.py; None (the default) is the algorithm and keeps its bits."""
import functools
import itertools

import numpy as np

import _attn_mutants
from _sddmm_bsr_ref import bound as sddmm_bsr_bound, full_mantissa as bf16_full_mantissa
from _softmax_bsr_ref import bf16_round, causal_mask, fma32, pattern

PATTERNS = ["ragged16", "ragged32", "edges16", "edges32"]
WIDTHS = [(8, 64), (64, 8), (128, 128), (40, 72)]
MASKS = ["none", "causal", "leading"]


def tag_of(bs, d, dv, mask, out_bf16):
    """What the dispatcher of fused/attn_bsr.hip picks: D<n> 32-column steps of D held (2 up to D = 64), T<n> tiles of Dv."""
    return f"attn_bsr<b{bs},{'bf16' if out_bf16 else 'f32'},{'mask' if mask else 'nomask'},D{2 if d <= 64 else 4},T{4 if dv <= 64 else 8}>"


# every tag the dispatcher can form -> the smallest (bS, D, Dv, mask, out_bf16) that reaches it
TAGS = {tag_of(bs, d, dv, mask, ob): (bs, d, dv, mask, ob)
        for bs, d, dv, mask, ob in itertools.product((16, 32), (8, 72), (8, 72), (False, True), (False, True))}


def leading_mask(name):
    """-Inf over the whole of the first ceil(n / 2) blocks of every block row of n >= 2 blocks, 0 elsewhere: at 16 x 16 a row of
    3 blocks or more starts with whole 32-key steps in which every key is masked."""
    bsr = pattern(name)
    bs = bsr.block_row_size
    ptrs = np.asarray(bsr.block_row_ptrs, dtype=np.int64)
    m = np.zeros((bsr.num_blocks, bs, bs), np.float32)
    for lo, hi in zip(ptrs[:-1], ptrs[1:]):
        if hi - lo >= 2:
            m[lo:lo + (hi - lo + 1) // 2] = -np.inf
    return m


@functools.lru_cache(maxsize=None)
def mask_of(name, kind):
    """none | causal (block-causal, _softmax_bsr_ref.causal_mask) | leading.  Read-only."""
    return {"none": lambda n: None, "causal": causal_mask, "leading": leading_mask}[kind](name)


@functools.lru_cache(maxsize=None)
def operands(name, d, dv, heads=1):
    """(q, k, v) float32 arrays of bf16 numbers, [H, rows, width]: all 8 significant bits in use.  Read-only."""
    p = pattern(name)
    rng = np.random.default_rng(500 + d + 7 * dv + 1000 * heads)
    return (bf16_full_mantissa(rng, (heads, p.num_rows, d)), bf16_full_mantissa(rng, (heads, p.num_cols, d)),
            bf16_full_mantissa(rng, (heads, p.num_cols, dv)))


def _block_rows(bsr):
    ptrs = np.asarray(bsr.block_row_ptrs, dtype=np.int64)
    cols = np.asarray(bsr.block_col_idxs, dtype=np.int64)
    bs = bsr.block_row_size
    for r, (lo, hi) in enumerate(zip(ptrs[:-1], ptrs[1:])):
        keys = (cols[lo:hi, None] * bs + np.arange(bs)).reshape(-1)
        yield r, lo, hi, keys


def _row_mask(mask, lo, hi, bs):
    """mask[lo:hi] as [bS rows, (hi - lo) * bS keys] in storage order."""
    return mask[lo:hi].transpose(1, 0, 2).reshape(bs, -1)


def lse_reference(name, q, k, mask, scale):
    """(exact lse in float64 per matrix row, its tolerance): see the module docstring.  An empty row: -Inf, tolerance 0."""
    bsr = pattern(name)
    bs = bsr.block_row_size
    q, k = q.astype(np.float64), k.astype(np.float64)
    exact, tol = np.full(bsr.num_rows, -np.inf), np.zeros(bsr.num_rows)
    u = 2.0 ** -24
    for r, lo, hi, keys in _block_rows(bsr):
        if hi == lo:
            continue
        rows = slice(r * bs, (r + 1) * bs)
        s, s_abs = q[rows] @ k[keys].T, np.abs(q[rows]) @ np.abs(k[keys]).T
        z = scale * s + (0.0 if mask is None else _row_mask(mask, lo, hi, bs).astype(np.float64))
        finite = np.isfinite(z)
        zf = np.where(finite, z, 0.0)
        e_z = np.where(finite, scale * sddmm_bsr_bound(False, q.shape[1], s, s_abs) + u * np.abs(scale * s) + u * np.abs(zf), 0.0)
        top = np.max(z, axis=1)
        lse = top + np.log(np.sum(np.exp(z - top[:, None]), axis=1))
        spread = top - np.min(np.where(finite, z, np.inf), axis=1)
        length = float(keys.shape[0])
        exact[rows] = lse
        tol[rows] = 1.01 * (np.max(e_z, axis=1) + (length + 8.0 * spread + 16.0) * u + 2.0 * u * (np.abs(lse) + np.log(length) + 1.0))
    return exact, tol


def _exp32(t, fault=None):
    """v_exp_f32 of fl(t * log2 e), in numpy float32."""
    if fault == "exp_float64":
        return np.exp(t.astype(np.float32).astype(np.float64)).astype(np.float32)
    return np.exp2((t.astype(np.float32) * np.float32(1.44269504088896340736)).astype(np.float32))


def bf16_trunc(v):
    """float32 -> the bf16 number next towards zero, as float32 (a fault: the contract rounds to nearest even)."""
    return (np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def mfma_add(acc, a, b, fault=None):
    """fl32(acc + a @ b) of an fp32 accumulator [m, n] and bf16 numbers a [m, k], b [k, n]: the sum taken in float64 and rounded once
    (the order inside the instruction is its own); `mfma_fp32_sequential`: in fp32, term after term."""
    if fault == "mfma_fp32_sequential":
        acc, a, b = acc.astype(np.float32), a.astype(np.float32), b.astype(np.float32)
        for j in range(a.shape[1]):
            acc = acc + a[:, j:j + 1] * b[j][None, :]           # a product of two bf16 numbers is exact in fp32
        return acc
    return (acc.astype(np.float64) + a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)


def fused_rows(bsr, q, k, v, mask, scale, fault=None):
    """(out [M, Dv], lse [M]) of one head on the pattern `bsr` by the algorithm as built, in numpy float32.  The MFMA sums are taken
    in float64 and rounded once (the order inside the instruction is its own).  fault: a name of tests/_attn_mutants.py (FORWARD or
    HONEST); None: the algorithm."""
    _attn_mutants.check(fault, _attn_mutants.FORWARD)
    f32 = np.float32
    bs = bsr.block_row_size
    out, lse = np.zeros((bsr.num_rows, v.shape[1]), f32), np.full(bsr.num_rows, -np.inf, f32)
    if fault == "scale_bf16":
        scale = bf16_round(f32(scale))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r, lo, hi, keys in _block_rows(bsr):
            if hi == lo:
                continue
            rows = slice(r * bs, (r + 1) * bs)
            s = (q[rows].astype(np.float64) @ k[keys].T.astype(np.float64)).astype(f32)
            if fault == "s_bf16":
                s = bf16_round(s)
            z = f32(scale) * s if mask is None else fma32(f32(scale), s, _row_mask(mask, lo, hi, bs))
            vk = v[keys].astype(np.float64)
            pad = -keys.shape[0] % 32                         # 16 x 16, an odd block count: a half step, scores -Inf, V zeros
            z = np.concatenate([z, np.full((bs, pad), -np.inf, f32)], axis=1)
            vk = np.concatenate([vk, np.zeros((pad, v.shape[1]))], axis=0)
            m = np.full(bs, -np.inf, f32)
            mu = np.zeros(bs, f32)
            l, lx = np.zeros((bs, 4), f32), np.zeros((bs, 4), f32)
            o = np.zeros((bs, v.shape[1]), f32)
            for at in range(0, z.shape[1], 32):
                zs = z[:, at:at + 32]
                m_new = np.fmax(m, np.fmax.reduce(zs, axis=1))                # fmax drops a NaN
                if fault == "stale_max" and at > 0:
                    m_new = m
                mu_new = np.where(np.isinf(m_new), f32(0), m_new)
                alpha = np.where(np.isneginf(m), f32(1), _exp32(mu - mu_new, fault))
                m, mu = m_new, mu_new
                w = _exp32(zs - mu[:, None], fault)
                if fault == "last_key_dropped" and at + 32 >= z.shape[1]:
                    live = np.isfinite(zs)
                    last = 31 - np.argmax(live[:, ::-1], axis=1)
                    w = w.copy()
                    w[live.any(axis=1), last[live.any(axis=1)]] = 0
                wb = bf16_trunc(w) if fault == "w_truncated" else bf16_round(w)
                # lane g of a row: keys 4g .. 4g + 3 of the first 16-key tile, then of the second, summed in that order
                lanes = lambda x: x.reshape(bs, 2, 4, 4).transpose(0, 2, 1, 3).reshape(bs, 4, 8)   # noqa: E731
                t, tx = np.zeros((bs, 4), f32), np.zeros((bs, 4), f32)
                for j in range(8):
                    t = t + lanes(w if fault == "divisor_unrounded" else wb)[:, :, j]
                    tx = tx + lanes(w)[:, :, j]
                l = l + t if fault == "rescale_skips_divisor" and at == 32 else l * alpha[:, None] + t
                lx = lx * alpha[:, None] + tx
                o = mfma_add(o * alpha[:, None], wb, vk[at:at + 32], fault)
                if fault == "acc_bf16":
                    o = bf16_round(o)
            meet = lambda x: (x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3])        # noqa: E731
            out[rows] = o * (f32(1) / meet(l))[:, None]
            lse[rows] = mu + np.log(meet(l if fault == "lse_from_rounded" else lx)).astype(f32)
    return out, lse


def fused_f32(name, q, k, v, mask, scale, fault=None):
    """fused_rows on pattern(name)."""
    return fused_rows(pattern(name), q, k, v, mask, scale, fault)


def out_tolerance(name, q, k, v, scale, mask, out_bf16):
    """The `out` component of tests/test_gpu_softmax_bsr.py::_attention_tolerances, formula for formula, evaluated block by
    block instead of on densified matrices, so that it can be had on ACTIVSg10K (tests/test_attn_fused_cpu.py holds the two
    equal on the small patterns).  [M, Dv] float64."""
    from _softmax_bsr_ref import forward, fwd_bound, layout, lengths, to_rows
    f64 = np.float64
    bsr = pattern(name)
    bs = bsr.block_row_size
    ptrs = np.asarray(bsr.block_row_ptrs, dtype=np.int64)
    rows_of = np.repeat(np.arange(ptrs.shape[0] - 1), np.diff(ptrs))
    cols_of = np.asarray(bsr.block_col_idxs, dtype=np.int64)
    within = np.arange(bs)
    q, k, v = (x.astype(f64) for x in (q, k, v))
    chunks = [slice(lo, min(lo + 4096, bsr.num_blocks)) for lo in range(0, bsr.num_blocks, 4096)]

    def sampled(x, y):                                         # [num_blocks, bS, bS]: <x_r, y_c>
        out = np.empty((bsr.num_blocks, bs, bs))
        for c in chunks:
            out[c] = np.matmul(x[rows_of[c, None] * bs + within], y[cols_of[c, None] * bs + within].transpose(0, 2, 1))
        return out

    def times(blocks, y):                                      # [M, n]: (the block array as a matrix) @ y
        per = np.empty((bsr.num_blocks, bs, y.shape[1]))
        for c in chunks:
            per[c] = np.matmul(blocks[c], y[cols_of[c, None] * bs + within])
        out = np.zeros((ptrs.shape[0] - 1, bs, y.shape[1]))
        filled = np.diff(ptrs) > 0
        if per.shape[0]:
            out[filled] = np.add.reduceat(per, ptrs[:-1][filled], axis=0)
        return out.reshape(-1, y.shape[1])

    row_ptrs, idx = layout(name)

    def per_row_max(blocks):
        vr = to_rows(name, blocks)
        lens = np.diff(row_ptrs)
        red = np.maximum.reduceat(vr, row_ptrs[:-1][lens > 0])
        flat = np.empty(blocks.size)
        flat[idx] = np.repeat(red, lens[lens > 0])
        return flat.reshape(blocks.shape)

    s, s_abs = sampled(q, k), sampled(np.abs(q), np.abs(k))
    e_s = sddmm_bsr_bound(False, q.shape[1], s, s_abs)
    z = scale * s + (0.0 if mask is None else mask.astype(f64))
    finite = np.isfinite(z)
    e_z = np.where(finite, scale * e_s + 2.0 ** -24 * np.abs(scale * s) + 2.0 ** -24 * np.abs(np.where(finite, z, 0.0)), 0.0)
    p, t = forward(name, np.where(finite, z, -np.inf), f64)
    e_row = per_row_max(e_z)
    shift = np.expm1(2 * e_row)
    e_p = p * shift + fwd_bound(True, lengths(name).astype(f64), t + 2 * e_row, p * (1 + shift))
    n_row = np.repeat(np.diff(ptrs) * bs, bs).astype(f64)[:, None]
    gamma = n_row * 2.0 ** -23 / (1.0 - n_row * 2.0 ** -23)
    tol = gamma * times(p + e_p, np.abs(v)) + times(e_p, np.abs(v))
    if out_bf16:
        tol = tol + 2.0 ** -8 * (np.abs(times(p, v)) + tol)
    return 1.01 * tol + 1e-30
