"""mispmm_attn_bsr_fp8_split on the GPU (include/mispmm_attn_fp8_split.h): the fixtures, the float64 `bounds` and the checks of
the one-launch test (test_gpu_attn_fp8.py), on ONE pattern whose step counts are (0, 1, 1, 4, 10, 2) at bS = 16 and
(0, 1, 2, 7, 19, 4) at bS = 32: n < S, n mod S != 0 and n = S for S in SPLITS, a half step that is the last step of the last
non-empty segment, an empty block row.

THE BOUND, written before any run.  Against one wave a merged term passes one more fp32 product (by w_s) and at most S - 1
more fp32 additions, on numerator and divisor alike: (L + 8 T + 16) u of the header's NUMERICS becomes (L + 8 T + 16 + 2 S) u.
bounds() does not take that term, so merge_term() forms what it adds per unit of S -- 2 u in lse, and in out
(1 + 2^-3) 2 u P' |v^| through the same second product, g_nv(U) included -- from the same float64 quantities.  A constant
column of V comes back to (L + 16 + 2 S) u relative.  The bound test PRINTS the worst share of each bound per case."""
import functools

import numpy as np
import pytest
import torch

from mispmm import attn_bsr_fp8, capi_attn_fp8_split, ops
from mispmm.attn_bsr_fp8_split import attention_bsr_fp8_split as split, workspace_bytes

from test_gpu_attn_fp8 import U, bounds, ints, mask_rows, strided, u, wide
from test_gpu_bsr_fp8 import F8, rand_e4m3, same_bits

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 7, 19, 4)  # blocks per block row; as many block rows, the first empty, as the imported bounds() walks
KB = 24                       # block columns; the last one is used by the longest row
H = 2                         # the heads bounds() walks
LONGEST = 4
CASES = [(bs, d, dv) for bs in (16, 32) for d, dv in ((16, 8), (80, 72), (128, 128))]     # D1 / D2, T4 / T8, partly dropped reads
IDS = [f"b{bs}-D{d}-Dv{dv}" for bs, d, dv in CASES]
SPLITS = [1, 2, 3, 8, 64]
GUARD = 64


@functools.lru_cache(maxsize=None)
def pattern(bs):
    rng = np.random.default_rng(3)
    cols = [np.sort(rng.choice(KB - 1, n, replace=False)) for n in COUNTS]
    cols[LONGEST][-1] = KB - 1
    ptrs = np.concatenate([[0], np.cumsum(COUNTS)])
    idxs = np.concatenate(cols).astype(np.int64)
    a = ops.DeviceBSR(len(COUNTS) * bs, KB * bs, bs, bs, len(idxs), torch.tensor(ptrs, dtype=torch.int32, device="cuda"),
                      torch.tensor(idxs, dtype=torch.int32, device="cuda"), None)
    keys = [np.concatenate([c * bs + np.arange(bs) for c in cs]).astype(np.int64) if len(cs) else np.zeros(0, np.int64) for cs in cols]
    return a, ptrs, keys


def run(a, q, k, v, s, mask=None, bf16=False, typed=False, **kw):
    """The two launches on permuted, padded operands (gap bytes NaN), out inside sentinels and a workspace of exactly the bytes
    asked for inside guards; asserts the tag the call leaves (the combine launch's: it names the out type and S); (out, lse) on
    the host."""
    bs, m, d, dv, heads = a.block_row_size, a.num_rows, q.shape[2], v.shape[2], q.shape[0]
    qd, kd, vd = strided(q, 16, 0x7F), strided(k, 16, 0x7F), strided(v, 8, 0x7F)
    if typed:
        qd, kd, vd = qd.view(F8), kd.view(F8), vd.view(F8)
    sentinel = 0x5A5A if bf16 else -12345.0
    box = torch.full((heads, m + 2, dv + 8), sentinel, dtype=torch.int16 if bf16 else torch.float32, device="cuda")
    need = workspace_bytes(a, heads, dv, s)
    assert need == 4 * heads * m * s * (dv + 3)
    ws = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dev = {n: (t.cuda() if torch.is_tensor(t) else t) for n, t in kw.items()}
    _, lse = split(a, qd, kd, vd, mask=None if mask is None else torch.from_numpy(mask).float().cuda(), out_bf16=bf16, return_lse=True, splits=s,
                   out=box[:, 1:m + 1, :dv], workspace=ws[GUARD:GUARD + need], **dev)
    assert capi_attn_fp8_split.last_kernel() == f"attn_bsr_fp8_combine<{'bf16' if bf16 else 'f32'},S{s}>"
    box, ws = box.cpu(), ws.cpu()
    assert bool((box[:, 0] == sentinel).all() and (box[:, -1] == sentinel).all() and (box[:, :, dv:] == sentinel).all()), "a sentinel was written"
    assert bool((ws[:GUARD] == 0xA5).all() and (ws[-GUARD:] == 0xA5).all()), "a guard of the workspace was written"
    return box[:, 1:m + 1, :dv].contiguous().numpy(), lse.cpu().numpy()


def lone_keys(bs, keys):
    """One key per query row by its place in the block row: the longest row's 16-row units visit every step, all rows every slot."""
    lone = np.full(len(COUNTS) * bs, -1)
    steps = -(-len(keys[LONGEST]) // 32)
    for r in range(1, len(COUNTS)):
        for i in range(bs):
            p = (7 * i + 11 * r + 1) % len(keys[r])
            if r == LONGEST:
                p = (i * steps // bs) * 32 + (7 * i) % (16 if bs == 16 and i * steps // bs == steps - 1 else 32)
            lone[r * bs + i] = p
    longest = lone[LONGEST * bs:(LONGEST + 1) * bs]
    assert {p % 32 for p in lone[bs:]} == set(range(32)) and {p // 32 for p in longest} == set(range(steps)) and longest.max() < len(keys[LONGEST])
    return lone


@pytest.mark.parametrize("s", SPLITS)
@pytest.mark.parametrize("bs, d, dv", CASES, ids=IDS)
def test_a_lone_key_per_row_is_bit_for_bit_for_every_split(bs, d, dv, s):
    a, ptrs, keys = pattern(bs)
    rng = np.random.default_rng(d)
    q, k, v = ints(rng, (H, a.num_rows, d), 8), ints(rng, (H, a.num_cols, d), 8), ints(rng, (H, a.num_cols, dv), 15)
    mask = np.full((a.num_blocks, bs, bs), -np.inf, dtype=np.float32)
    lone = lone_keys(bs, keys)
    for row in range(bs, a.num_rows):
        r, i = divmod(row, bs)
        mask[ptrs[r] + lone[row] // bs, i, lone[row] % bs] = 0.0
    qs, ks, vs = (torch.tensor(x, dtype=torch.float32) for x in ((2.0, 0.5), (0.125, 4.0), (0.25, 8.0)))
    out, lse = run(a, q, k, v, s, mask, q_scale=qs, k_scale=ks, v_scale=vs, scale=0.25)
    want, want_lse = np.zeros((H, a.num_rows, dv), np.float32), np.full((H, a.num_rows), -np.inf, np.float32)
    for h in range(H):
        for row in range(bs, a.num_rows):
            key = keys[row // bs][lone[row]]
            want[h, row] = wide(v)[h, key] * float(vs[h])
            want_lse[h, row] = 0.25 * float(qs[h]) * float(ks[h]) * (wide(q)[h, row] @ wide(k)[h, key])
    assert same_bits(out, want) and same_bits(lse, want_lse)


@functools.lru_cache(maxsize=None)
def random_case(bs, d, dv):
    """Random e4m3 bytes of every exponent, a random mask with -Inf, per-head scales; the float64 bounds and what a unit of S adds."""
    a, ptrs, keys = pattern(bs)
    rng = np.random.default_rng(dv)
    q, k, v = rand_e4m3(rng, (H, a.num_rows, d)), rand_e4m3(rng, (H, a.num_cols, d)), rand_e4m3(rng, (H, a.num_cols, dv))
    mask = rng.normal(0, 2, (a.num_blocks, bs, bs)).astype(np.float32)
    mask[rng.random(mask.shape) < 0.2] = -np.inf
    qs, ks, vs = (torch.from_numpy(rng.uniform(0.5, 1.5, H) * s).float() for s in (2.0 ** -6, 2.0 ** -6, 1.0))
    c = (np.float32(d ** -0.5) * qs.numpy() * ks.numpy()).astype(np.float64)          # fp32 products in the kernel's order
    ref = bounds(bs, ptrs, keys, q, k, v, mask, c, vs.numpy().astype(np.float64))
    return q, k, v, mask, (qs, ks, vs), ref, merge_term(bs, ptrs, keys, q, k, v, mask, c, vs.numpy().astype(np.float64))


def merge_term(bs, ptrs, keys, q, k, v, mask, c, vs):
    """What one unit of S adds to the bound of out: (1 + 2^-3) 2 u P' |v^| (1 + g_nv(U)) v_scale, P' = exp(2 E_r) P_x as in bounds()."""
    q64, k64, v64 = wide(q), wide(k), wide(v)
    add = np.zeros((H, q.shape[1], v.shape[2]))
    chain = 2 * (1 if q.shape[2] <= 64 else 2)
    for h in range(H):
        for r in range(1, len(COUNTS)):
            rows, kk, vv, L = slice(r * bs, (r + 1) * bs), k64[h, keys[r]], v64[h, keys[r]], len(keys[r])
            z = c[h] * (q64[h, rows] @ kk.T) + mask_rows(bs, ptrs, mask, r)
            kept = np.isfinite(z)
            n = (q64[h, rows] != 0).astype(float) @ (kk != 0).astype(float).T + chain
            E = np.where(kept, n * U / (1 - n * U) * c[h] * (np.abs(q64[h, rows]) @ np.abs(kk).T) + 2 * u * np.abs(np.where(kept, z, 0)), 0)
            w = np.exp(z - np.where(kept, z, -np.inf).max(axis=1, keepdims=True))
            Pk = np.exp(2 * E.max(axis=1, keepdims=True)) * w / w.sum(axis=1, keepdims=True)
            nv = L + 2 * -(-L // 32) + 2
            add[h, rows] = (1 + 2.0 ** -3) * 2 * u * (1 + nv * U / (1 - nv * U)) * (Pk @ np.abs(vv)) * vs[h]
    return add


@pytest.mark.parametrize("bs, d, dv", CASES, ids=IDS)
def test_one_split_with_own_kv_heads_has_the_bits_of_the_one_launch_kernel(bs, d, dv):
    a, _, _ = pattern(bs)
    q, k, v, mask, (qs, ks, vs), _, _ = random_case(bs, d, dv)
    dev = dict(mask=torch.from_numpy(mask).cuda(), q_scale=qs.cuda(), k_scale=ks.cuda(), v_scale=vs.cuda(), return_lse=True)
    for bf16 in (False, True):
        want = attn_bsr_fp8.attention_bsr_fp8(a, q.cuda(), k.cuda(), v.cuda(), out_bf16=bf16, **dev)
        got = split(a, q.cuda(), k.cuda(), v.cuda(), out_bf16=bf16, splits=1, **dev)
        assert same_bits(got[0].cpu().numpy(), want[0].cpu().numpy()) and same_bits(got[1].cpu().numpy(), want[1].cpu().numpy()), bf16


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("heads, kv_heads", [(2, 1), (4, 2)])
@pytest.mark.parametrize("bs", (16, 32))
def test_shared_kv_heads_have_the_bits_of_k_and_v_repeated_per_query_head(bs, heads, kv_heads, s):
    a, _, _ = pattern(bs)
    rng = np.random.default_rng(heads)
    d, dv, group = 80, 72, heads // kv_heads
    q, k, v = rand_e4m3(rng, (heads, a.num_rows, d)), rand_e4m3(rng, (kv_heads, a.num_cols, d)), rand_e4m3(rng, (kv_heads, a.num_cols, dv))
    mask = torch.from_numpy(rng.normal(0, 2, (a.num_blocks, bs, bs)).astype(np.float32)).cuda()
    qs, ks, vs = (torch.from_numpy(rng.uniform(0.5, 1.5, n) * f).float().cuda() for n, f in ((heads, 0.125), (kv_heads, 0.125), (kv_heads, 1.0)))
    qd, kd, vd = strided(q, 16, 0x7F), strided(k, 16, 0x7F), strided(v, 8, 0x7F)    # permuted [rows, Hkv, width]: the head stride is not rows * ld
    got = split(a, qd, kd, vd, q_scale=qs, k_scale=ks, v_scale=vs, mask=mask, return_lse=True, splits=s)
    rep = lambda t: t.repeat_interleave(group, dim=0).contiguous()                   # noqa: E731
    want = split(a, qd, rep(kd), rep(vd), q_scale=qs, k_scale=rep(ks), v_scale=rep(vs), mask=mask, return_lse=True, splits=s)
    assert same_bits(got[0].cpu().numpy(), want[0].cpu().numpy()) and same_bits(got[1].cpu().numpy(), want[1].cpu().numpy())
    if kv_heads == 1:                                                               # a 2-D k and v beside a 3-D q: one KV head
        flat = split(a, qd, kd[0], vd[0], q_scale=qs, k_scale=ks, v_scale=vs, mask=mask, return_lse=True, splits=s)
        assert same_bits(flat[0].cpu().numpy(), want[0].cpu().numpy()) and same_bits(flat[1].cpu().numpy(), want[1].cpu().numpy())


@pytest.mark.parametrize("s", SPLITS)
@pytest.mark.parametrize("bs, d, dv", CASES, ids=IDS)
def test_random_e4m3_bytes_keep_the_bounds_of_the_header_with_the_merge_term(bs, d, dv, s):
    a, _, _ = pattern(bs)
    q, k, v, mask, (qs, ks, vs), (want, lim, want_lse, lim_lse), add = random_case(bs, d, dv)
    out, lse = run(a, q, k, v, s, mask, q_scale=qs, k_scale=ks, v_scale=vs)
    err, err_lse = np.abs(out[:, bs:] - want[:, bs:]), np.abs(lse[:, bs:] - want_lse[:, bs:])
    lim_s, lim_lse_s = (lim + s * add)[:, bs:], (lim_lse + 2 * s * u)[:, bs:]
    print(f"b{bs} D={d} Dv={dv} S={s}: worst |out - exact| / bound = {np.max(err / lim_s):.4f}, worst |lse - exact| / bound = "
          f"{np.max(err_lse / lim_lse_s):.4f}")
    assert np.all(err <= lim_s) and np.all(err_lse <= lim_lse_s)
    assert not out[:, :bs].view(np.uint8).any() and np.all(lse[:, :bs] == -np.inf), "an empty block row is +0 and -Inf"
    # tie rows: every kept key scores the same, and a constant column of V comes back to (L + 16 + 2 S) 2^-24, not to 2^-4
    rng = np.random.default_rng(s)
    const = rand_e4m3(rng, (H, 1, dv)).expand(H, a.num_cols, dv).contiguous()
    tie = np.where(np.isfinite(mask), np.float32(0), mask)
    out, _ = run(a, torch.zeros_like(q), k, const, s, tie, v_scale=2.0)
    L = np.repeat(np.array(COUNTS[1:]) * bs, bs)[None, :, None]
    assert np.all(np.abs(out[:, bs:] - 2 * wide(const)[:, :1]) <= (L + 16 + 2 * s) * u * np.abs(2 * wide(const)[:, :1]))


@pytest.mark.parametrize("bs", (16, 32))
def test_special_values_and_plumbing(bs):
    a, ptrs, keys = pattern(bs)
    rng = np.random.default_rng(8)
    d, dv, s = 80, 72, 3
    q, k, v = ints(rng, (H, a.num_rows, d), 3), ints(rng, (H, a.num_cols, d), 3), rand_e4m3(rng, (H, a.num_cols, dv))
    lo, hi = ptrs[LONGEST], ptrs[LONGEST + 1]
    base = rng.normal(0, 1, (a.num_blocks, bs, bs)).astype(np.float32)
    base[lo:lo + 13, 10] = -np.inf                                         # row 10 of the longest block row: segments 0 and 1 of 3 wholly masked
    c = np.full(H, np.float32(0.05), np.float64)
    want, lim, _, _ = bounds(bs, ptrs, keys, q, k, v, base, c, np.ones(H))
    add = merge_term(bs, ptrs, keys, q, k, v, base, c, np.ones(H))
    one = torch.ones(H)
    clean, clean_lse = run(a, q, k, v, s, base, scale=0.05)
    for other in (run(a, q, k, v, s, base, scale=0.05, typed=True), run(a, q, k, v, s, base, scale=0.05, q_scale=one, k_scale=1.0, v_scale=one)):
        assert same_bits(clean, other[0]) and same_bits(clean_lse, other[1])
    half = LONGEST * bs + 10
    assert np.isfinite(clean[:, half]).all() and np.isfinite(clean_lse[:, half]).all()
    assert np.all(np.abs(clean[:, bs:] - want[:, bs:]) <= (lim + s * add)[:, bs:])
    # a NaN score, a +Inf score and a row of nothing but -Inf, each in a segment of its own, stay in their matrix rows
    m = base.copy()
    m[lo + 1, 1, bs - 1], m[hi - 1, 4, 0], m[lo:hi, 7] = np.nan, np.inf, -np.inf
    got, lse = run(a, q, k, v, s, m, scale=0.05)
    hit = np.zeros(a.num_rows, bool)
    hit[LONGEST * bs + np.array([1, 4, 7])] = True
    assert np.array_equal(np.isnan(got), np.broadcast_to(hit[None, :, None], got.shape)), "NaN positions differ"
    assert same_bits(got[:, ~hit], clean[:, ~hit]) and same_bits(lse[:, ~hit], clean_lse[:, ~hit]), "another row changed"
    assert all(np.array_equal(lse[h, hit], np.array([np.nan, np.inf, -np.inf], np.float32), equal_nan=True) for h in range(H)), lse[:, hit]
    # a NaN byte in V behind a key that row 10 masks, in another segment than the row's live one: its column of the rows under its block
    vn = v.clone()
    col = int(a.block_col_idxs[lo + 2])
    vn[0, col * bs + 9, 13] = 0xFF
    under = np.repeat([col * bs in keys[r] for r in range(len(COUNTS))], bs)
    got, got_lse = run(a, q, k, vn, s, base, scale=0.05)
    want_nan = np.zeros(clean.shape, bool)
    want_nan[0, under, 13] = True
    assert under[half] and np.array_equal(np.isnan(got), want_nan) and same_bits(got[~want_nan], clean[~want_nan]) and same_bits(got_lse, clean_lse)
    # a workspace one byte short is refused; a graph captured once replays twice to the eager bits
    qd, kd, vd, md = (t.cuda() for t in (q, k, v, torch.from_numpy(base)))
    need = workspace_bytes(a, H, dv, s)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=f"at least {need} bytes"):
        split(a, qd, kd, vd, mask=md, scale=0.05, splits=s, workspace=ws[:need - 1])
    vs = one.cuda()
    eager = split(a, qd, kd, vd, mask=md, scale=0.05, v_scale=vs, splits=s)
    held = torch.empty_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                              # two launches in a row: no parallel branches
        split(a, qd, kd, vd, mask=md, scale=0.05, v_scale=vs, splits=s, out=held, workspace=ws)
    for _ in range(2):
        held.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(held.view(torch.int32), eager.view(torch.int32)) and same_bits(eager.cpu().numpy(), clean)
