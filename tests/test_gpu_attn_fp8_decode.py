"""mispmm_attn_decode_fp8 on the GPU (include/mispmm_attn_fp8_decode.h) on ONE paged cache: six sequences of 0, 1, 2, 3, 7 and 19
pages over 24 cache pages, the 2-page and the 7-page sequence sharing their first page, the last cache page used.  Lengths: one
key in the only page; full pages (seq_lens past the pages: clamped); pages but seq_lens = 0; a last page cut inside its first
16 keys (at bS = 16 behind a half step); 19 pages cut inside the second 16 keys of the last at bS = 32, full at bS = 16 (the odd
page count: a half step).  K and V are a permuted [pages, bS, Hkv, width] view with NaN bytes behind every masked key, in the
pages no sequence lists and in the stride gaps; out and an exact-size workspace sit inside sentinels.

THE BOUND is mispmm_attn_fp8.h NUMERICS with the (L + 8 T + 16 + 2 S) u term of the split header (bound()); its test PRINTS the
worst share.  Pages with seq_lens = 0 are +0 / -Inf here and NaN / -Inf in the unpacked call (a row of nothing but -Inf)."""
import functools

import numpy as np
import pytest
import torch

from mispmm import capi_attn_fp8_decode, ops
from mispmm.attn_bsr_fp8_split import attention_bsr_fp8_split
from mispmm.attn_decode_fp8 import attention_decode_fp8 as decode, workspace_bytes

from test_gpu_attn_fp8 import U, strided, u, wide
from test_gpu_bsr_fp8 import F8, rand_e4m3, same_bits

pytestmark = pytest.mark.gpu

PAGES = (0, 1, 2, 3, 7, 19)
KB, B, DEAD, GUARD = 24, len(PAGES), 3, 64          # DEAD: the sequence with pages and seq_lens = 0
DIMS, HEADS, SPLITS = ((16, 8), (80, 72), (128, 128)), ((2, 2), (6, 2), (16, 1)), (1, 3, 64)   # D1 / D2, T4 / T8; G = 1, 3, 16
# thinned: every pair (dims, heads) once per bS, the split running through them: every value of each axis with bS 16 and with bS 32
CASES = [(bs, *DIMS[a], *HEADS[b], SPLITS[(a + b + bs // 32) % 3]) for bs in (16, 32) for a in range(3) for b in range(3)]
IDS = ["b{}-D{}-Dv{}-H{}over{}-S{}".format(*c) for c in CASES]


@functools.lru_cache(maxsize=None)
def cache(bs):
    """(page_ptrs, page lists, seq_lens as given, unmasked keys per sequence as cache rows, which cache rows hold an unmasked key)."""
    rng = np.random.default_rng(5)
    perm = rng.permutation(KB - 1)
    tails, pool = perm[:5], perm[5:]                                          # a page with a masked key belongs to one sequence alone
    lists = [[], [tails[0]], list(pool[:2]), list(tails[1:4]), [pool[0], *rng.choice(pool[2:], 5, replace=False), tails[4]],
             [*rng.permutation(pool), KB - 1]]
    assert tuple(len(p) for p in lists) == PAGES and lists[2][0] == lists[4][0]
    lens = np.array([0, 1, 2 * bs + 100, 0, 6 * bs + 5, 18 * bs + (21 if bs == 32 else 16)])
    keys = [np.concatenate([p * bs + np.arange(bs) for p in pl] + [np.zeros(0, np.int64)]).astype(np.int64)[:n] for pl, n in zip(lists, lens)]
    live = np.zeros(KB * bs, bool)
    live[np.concatenate(keys)] = True
    return np.concatenate([[0], np.cumsum(PAGES)]), lists, lens, keys, live


@functools.lru_cache(maxsize=None)
def problem(bs, d, dv, h, hkv, small=False):
    """q [B, H, D], k, v [Hkv, rows, width] as bytes -- random e4m3 bytes of every exponent, or small integers -- and per-head scales."""
    rng = np.random.default_rng(d + h)
    if small:
        make = lambda shape, top: torch.from_numpy(rng.integers(-top, top + 1, shape).astype(np.float32)).to(F8).view(torch.uint8)   # noqa: E731
        q, k, v = make((B, h, d), 8), make((hkv, KB * bs, d), 8), make((hkv, KB * bs, dv), 15)
        qs, ks, vs = (torch.tensor(np.resize(x, n), dtype=torch.float32) for x, n in (((2.0, 0.5), h), ((0.125, 4.0), hkv), ((0.25, 8.0), hkv)))
    else:
        q, k, v = rand_e4m3(rng, (B, h, d)), rand_e4m3(rng, (hkv, KB * bs, d)), rand_e4m3(rng, (hkv, KB * bs, dv))
        qs, ks, vs = (torch.from_numpy(rng.uniform(0.5, 1.5, n) * f).float() for n, f in ((h, 2.0 ** -6), (hkv, 2.0 ** -6), (hkv, 1.0)))
    return q, k, v, qs, ks, vs


def i32(x):
    return torch.tensor(np.asarray(x, dtype=np.int64), dtype=torch.int32, device="cuda")


def behind(x, live, fill):
    """x [Hkv, rows, w] with `fill` in every row that holds no unmasked key."""
    x = x.clone()
    x[:, torch.from_numpy(~live)] = fill
    return x


def run(bs, q, k, v, s, lens, bf16=False, typed=False, **kw):
    """The call on a permuted, padded cache and q (gap bytes NaN), out inside sentinels, an exact workspace inside guards; asserts the tag."""
    ptrs, lists, _, _, _ = cache(bs)
    (_, h, d), dv = q.shape, v.shape[2]
    qd = torch.full((B, h, d + 16), 0x7F, dtype=torch.uint8)
    qd[:, :, :d] = q
    qd, kd, vd = qd.cuda()[:, :, :d], strided(k, 16, 0x7F), strided(v, 8, 0x7F)
    if typed:
        qd, kd, vd = qd.view(F8), kd.view(F8), vd.view(F8)
    sentinel = 0x5A5A if bf16 else -12345.0
    box = torch.full((B + 2, h, dv + 8), sentinel, dtype=torch.int16 if bf16 else torch.float32, device="cuda")
    need = workspace_bytes(B, h, h // k.shape[0], dv, s)
    assert need == 4 * B * h * s * (dv + 3)
    ws = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dev = {n: (t.cuda() if torch.is_tensor(t) else t) for n, t in kw.items()}
    _, lse = decode(i32(ptrs), i32(np.concatenate(lists)), bs, qd, kd, vd, seq_lens=None if lens is None else i32(lens), out_bf16=bf16,
                    return_lse=True, splits=s, out=box[1:B + 1, :, :dv], workspace=ws[GUARD:GUARD + need], **dev)
    assert capi_attn_fp8_decode.last_kernel() == f"attn_decode_fp8_combine<{'bf16' if bf16 else 'f32'},S{s}>"
    box, ws = box.cpu(), ws.cpu()
    assert bool((box[0] == sentinel).all() and (box[-1] == sentinel).all() and (box[:, :, dv:] == sentinel).all()), "a sentinel was written"
    assert bool((ws[:GUARD] == 0xA5).all() and (ws[-GUARD:] == 0xA5).all()), "a guard of the workspace was written"
    return box[1:B + 1, :, :dv].contiguous().numpy(), lse.cpu().numpy()


def bound(q, kk, vv, c, vs, s):
    """float64 out and lse of one (b, h) over its L unmasked keys, and the limits of mispmm_attn_fp8.h NUMERICS with
    (L + 8 T + 16 + 2 S) u for the fp32 term: (out, limit, lse, limit)."""
    L = len(kk)
    z = c * (kk @ q)
    n = (kk != 0).astype(float) @ (q != 0).astype(float) + 2 * (1 if len(q) <= 64 else 2)
    Er = (n * U / (1 - n * U) * c * (np.abs(kk) @ np.abs(q)) + 2 * u * np.abs(z)).max()
    w = np.exp(z - z.max())
    P = w / w.sum()
    T = (z.max() - z).max() + 2 * Er
    Pk = np.exp(2 * Er) * P
    f32 = (L + 8 * T + 16 + 2 * s) * u
    dP = (2.0 ** -3 * Pk + 17 / 16 * 2.0 ** -18 * (1 + L * Pk)) / (1 - L * 2.0 ** -17) + (1 + 2.0 ** -3) * (f32 * Pk + 2.0 ** -126) + 2.0 ** -126
    nv = L + 2 * -(-L // 32) + 2
    out, lse = P @ vv * vs, z.max() + np.log(w.sum())
    lim = ((dP + (np.exp(2 * Er) - 1) * P) @ np.abs(vv) + nv * U / (1 - nv * U) * ((Pk + dP) @ np.abs(vv))) * vs + 2 * u * np.abs(out)
    return out, lim, lse, Er + f32 + 2 * u * (np.log(L) + 1) + 2 * u * abs(lse)


@pytest.mark.parametrize("bs, d, dv, h, hkv, s", CASES, ids=IDS)
def test_random_e4m3_bytes_keep_the_bounds_of_the_header_whatever_lies_behind_a_masked_key(bs, d, dv, h, hkv, s):
    _, _, lens, keys, live = cache(bs)
    q, k, v, qs, ks, vs = problem(bs, d, dv, h, hkv)
    out, lse = run(bs, q, behind(k, live, 0x7F), behind(v, live, 0xFF), s, lens, q_scale=qs, k_scale=ks, v_scale=vs)
    q64, k64, v64, g = wide(q), wide(k), wide(v), h // hkv
    c = (np.float32(d ** -0.5) * qs.numpy() * np.repeat(ks.numpy(), g)).astype(np.float64)    # fp32 products in the kernel's order
    worst = [0.0, 0.0]
    for b in range(B):
        if len(keys[b]) == 0:
            assert not out[b].view(np.uint32).any() and np.all(lse[b] == -np.inf), "a sequence without unmasked keys is +0 and -Inf"
            continue
        for hh in range(h):
            want, lim, want_lse, lim_lse = bound(q64[b, hh], k64[hh // g, keys[b]], v64[hh // g, keys[b]], c[hh], float(vs[hh // g]), s)
            err, err_lse = np.abs(out[b, hh] - want), abs(lse[b, hh] - want_lse)
            assert np.all(err <= lim) and err_lse <= lim_lse, (b, hh, np.max(err - lim), err_lse, lim_lse)
            worst = [max(worst[0], np.max(err[lim > 0] / lim[lim > 0], initial=0.0)), max(worst[1], err_lse / lim_lse)]    # a zero column of V: 0 <= 0
    print(f"b{bs} D={d} Dv={dv} H={h} over {hkv} S={s}: worst |out - exact| / bound = {worst[0]:.4f}, worst |lse - exact| / bound = {worst[1]:.4f}")


@pytest.mark.parametrize("bs, d, dv, h, hkv, s", CASES, ids=IDS)
def test_packed_heads_and_nan_tails_have_the_bits_of_the_unpacked_call_on_one_block_row_per_sequence(bs, d, dv, h, hkv, s):
    ptrs, lists, lens, keys, live = cache(bs)
    q, k, v, qs, ks, vs = problem(bs, d, dv, h, hkv)
    idxs = np.concatenate(lists)
    a = ops.DeviceBSR(B * bs, KB * bs, bs, bs, len(idxs), i32(ptrs), i32(idxs), None)
    rows = torch.zeros((h, B * bs, d), dtype=torch.uint8)
    rows[:, ::bs] = q.permute(1, 0, 2)                                            # the token's q in row 0 of its block row
    mask = np.zeros((len(idxs), bs, bs), np.float32)
    for b in range(B):
        gone = np.arange(PAGES[b] * bs) >= len(keys[b])
        mask[ptrs[b]:ptrs[b + 1]][np.broadcast_to(gone.reshape(PAGES[b], 1, bs), (PAGES[b], bs, bs))] = -np.inf
    want, want_lse = attention_bsr_fp8_split(a, rows.cuda(), behind(k, live, 0).cuda(), behind(v, live, 0).cuda(), q_scale=qs.cuda(),
                                             k_scale=ks.cuda(), v_scale=vs.cuda(), mask=torch.from_numpy(mask).cuda(), return_lse=True, splits=s)
    want, want_lse = want[:, ::bs].permute(1, 0, 2).cpu().numpy(), want_lse[:, ::bs].T.cpu().numpy()
    assert np.isnan(want[DEAD]).all() and np.all(want_lse[DEAD] == -np.inf)      # a row of nothing but -Inf there; +0 here
    want[DEAD] = 0.0
    out, lse = run(bs, q, behind(k, live, 0x7F), behind(v, live, 0xFF), s, lens, q_scale=qs, k_scale=ks, v_scale=vs)
    assert same_bits(out, want) and same_bits(lse, want_lse)


@pytest.mark.parametrize("s", SPLITS)
@pytest.mark.parametrize("bs, d, dv, h, hkv", [(16, 80, 72, 6, 2), (32, 128, 128, 16, 1), (32, 16, 8, 2, 2)])
def test_a_lone_unmasked_key_per_sequence_is_bit_for_bit_for_every_split(bs, d, dv, h, hkv, s):
    _, lists, _, _, _ = cache(bs)
    q, k, v, qs, ks, vs = problem(bs, d, dv, h, hkv, small=True)
    lens = np.minimum(1, PAGES)                                                   # the first key of the first page; every later segment is masked
    live = np.zeros(KB * bs, bool)
    live[[pl[0] * bs for pl in lists if pl]] = True
    out, lse = run(bs, q, behind(k, live, 0x7F), behind(v, live, 0xFF), s, lens, q_scale=qs, k_scale=ks, v_scale=vs, scale=0.25)
    want, want_lse = np.zeros((B, h, dv), np.float32), np.full((B, h), -np.inf, np.float32)
    for b in range(1, B):
        for hh in range(h):
            kv, key = hh // (h // hkv), lists[b][0] * bs
            want[b, hh] = wide(v)[kv, key] * float(vs[kv])
            want_lse[b, hh] = 0.25 * float(qs[hh]) * float(ks[kv]) * (wide(q)[b, hh] @ wide(k)[kv, key])
    assert same_bits(out, want) and same_bits(lse, want_lse)


@pytest.mark.parametrize("bs", (16, 32))
def test_plumbing(bs):
    ptrs, lists, lens, _, live = cache(bs)
    d, dv, h, hkv, s = 80, 72, 6, 2, 3
    q, k, v, qs, ks, vs = problem(bs, d, dv, h, hkv)
    scales = dict(q_scale=qs, k_scale=ks, v_scale=vs)
    out, lse = run(bs, q, k, v, s, lens, **scales)
    typed = run(bs, q, k, v, s, lens, typed=True, **scales)
    assert same_bits(out, typed[0]) and same_bits(lse, typed[1])
    half, _ = run(bs, q, k, v, s, lens, bf16=True, **scales)
    assert same_bits(half, torch.from_numpy(out).to(torch.bfloat16).view(torch.int16).numpy())
    full = run(bs, q, k, v, s, np.array(PAGES) * bs, **scales)                    # seq_lens = None: every listed page is full
    none = run(bs, q, k, v, s, None, **scales)
    assert same_bits(full[0], none[0]) and same_bits(full[1], none[1]) and not same_bits(full[0][4], out[4])
    # a workspace one byte short is refused; a graph captured once replays twice to the eager bits
    args = (i32(ptrs), i32(np.concatenate(lists)), bs, q.cuda(), k.cuda(), v.cuda())
    kw = dict(seq_lens=i32(lens), splits=s, **{n: t.cuda() for n, t in scales.items()})
    need = workspace_bytes(B, h, h // hkv, dv, s)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=f"at least {need} bytes"):
        decode(*args, workspace=ws[:need - 1], **kw)
    held = torch.empty((B, h, dv), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                     # two launches in a row: no parallel branches
        decode(*args, out=held, workspace=ws, **kw)
    for _ in range(2):
        held.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(held.cpu().numpy(), out)
