"""mispmm_attn_bsr_fp8 on the GPU (include/mispmm_attn_fp8.h) against float64 numpy on the exactly widened e4m3 bytes.  The
bound test PRINTS the worst observed share of the header's bounds for out and lse."""
import numpy as np
import pytest
import torch

from mispmm import attn_bsr_fp8, capi_attn_fp8, ops

from test_gpu_bsr_fp8 import F8, rand_e4m3, same_bits

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 3, 5, 4)   # blocks per block row: empty, a half step at bS = 16, both stages used in turn
KB = 8                        # block columns; the last one is used by the longest row
H = 2
CASES = [(bs, d, dv) for bs in (16, 32) for d, dv in ((16, 8), (80, 72), (128, 128))]     # D1 / D2, T4 / T8, partly dropped reads
IDS = [f"b{bs}-D{d}-Dv{dv}" for bs, d, dv in CASES]
U, u = 2.0 ** -14, 2.0 ** -24  # per addition inside the 8-bit MFMA (measured, include/mispmm_bsr_fp8.h); fp32


def pattern(bs):
    rng = np.random.default_rng(3)
    cols = [np.sort(rng.choice(KB - 1, n, replace=False)) for n in COUNTS]
    cols[4][-1] = KB - 1
    ptrs = np.concatenate([[0], np.cumsum(COUNTS)])
    idxs = np.concatenate(cols).astype(np.int64)
    a = ops.DeviceBSR(len(COUNTS) * bs, KB * bs, bs, bs, len(idxs), torch.tensor(ptrs, dtype=torch.int32, device="cuda"),
                      torch.tensor(idxs, dtype=torch.int32, device="cuda"), None)
    keys = [np.concatenate([c * bs + np.arange(bs) for c in cs]).astype(np.int64) if len(cs) else np.zeros(0, np.int64) for cs in cols]
    return a, ptrs, keys


def mask_rows(bs, ptrs, mask, r):
    """The mask of block row r as [bs, L]: its blocks side by side."""
    return np.concatenate([mask[e] for e in range(ptrs[r], ptrs[r + 1])], axis=1) if ptrs[r + 1] > ptrs[r] else np.zeros((bs, 0))


def strided(x, pad, fill):
    """x [H, rows, w] on the device as a permuted [rows, H, w + pad] view, the gap columns holding `fill`."""
    t = torch.full((x.shape[1], x.shape[0], x.shape[2] + pad), fill, dtype=x.dtype)
    t[:, :, :x.shape[2]] = x.permute(1, 0, 2)
    return t.cuda().permute(1, 0, 2)[:, :, :x.shape[2]]


def run(a, q, k, v, mask=None, bf16=False, typed=False, **kw):
    """One launch on permuted, padded operands (gap bytes NaN) with out inside sentinels; asserts the tag; (out, lse) on the host."""
    bs, m, d, dv = a.block_row_size, a.num_rows, q.shape[2], v.shape[2]
    qd, kd, vd = strided(q, 16, 0x7F), strided(k, 16, 0x7F), strided(v, 8, 0x7F)
    if typed:
        qd, kd, vd = qd.view(F8), kd.view(F8), vd.view(F8)
    sentinel = 0x5A5A if bf16 else -12345.0
    box = torch.full((H, m + 2, dv + 8), sentinel, dtype=torch.int16 if bf16 else torch.float32, device="cuda")
    dev = {n: (t.cuda() if torch.is_tensor(t) else t) for n, t in kw.items()}
    _, lse = attn_bsr_fp8.attention_bsr_fp8(a, qd, kd, vd, mask=None if mask is None else torch.from_numpy(mask).float().cuda(), out_bf16=bf16,
                                            return_lse=True, out=box[:, 1:m + 1, :dv], **dev)
    assert capi_attn_fp8.last_kernel() == (f"attn_bsr_fp8<b{bs},{'bf16' if bf16 else 'f32'},{'nomask' if mask is None else 'mask'},"
                                           f"D{1 if d <= 64 else 2},T{4 if dv <= 64 else 8}>")
    box = box.cpu()
    assert bool((box[:, 0] == sentinel).all() and (box[:, -1] == sentinel).all() and (box[:, :, dv:] == sentinel).all()), "a sentinel was written"
    return box[:, 1:m + 1, :dv].contiguous().numpy(), lse.cpu().numpy()


def ints(rng, shape, top):
    return torch.from_numpy(rng.integers(-top, top + 1, shape).astype(np.float32)).to(F8).view(torch.uint8)


def wide(t):
    return t.view(F8).to(torch.float64).numpy()


@pytest.mark.parametrize("bs, d, dv", CASES, ids=IDS)
def test_a_lone_key_pins_every_slot_of_both_products_bit_for_bit(bs, d, dv):
    a, ptrs, keys = pattern(bs)
    rng = np.random.default_rng(d)
    q, k, v = ints(rng, (H, a.num_rows, d), 8), ints(rng, (H, a.num_cols, d), 8), ints(rng, (H, a.num_cols, dv), 15)
    mask = np.full((a.num_blocks, bs, bs), -np.inf, dtype=np.float32)
    lone = np.full(a.num_rows, -1)
    for r in range(1, len(COUNTS)):
        for i in range(bs):
            p = (7 * i + 11 * r) % len(keys[r])                           # the row's lone key, by its place in the block row
            mask[ptrs[r] + p // bs, i, p % bs] = 0.0
            lone[r * bs + i] = p
    longest = lone[4 * bs:5 * bs]
    assert {p % 32 for p in lone[bs:]} == set(range(32)) and {p // 32 for p in longest} == set(range(-(-5 * bs // 32)))
    qs, ks, vs = (torch.tensor(x, dtype=torch.float32) for x in ((2.0, 0.5), (0.125, 4.0), (0.25, 8.0)))
    out, lse = run(a, q, k, v, mask, q_scale=qs, k_scale=ks, v_scale=vs, scale=0.25)
    want, want_lse = np.zeros((H, a.num_rows, dv), np.float32), np.full((H, a.num_rows), -np.inf, np.float32)
    for h in range(H):
        for row in range(bs, a.num_rows):
            key = keys[row // bs][lone[row]]
            want[h, row] = wide(v)[h, key] * float(vs[h])
            want_lse[h, row] = 0.25 * float(qs[h]) * float(ks[h]) * (wide(q)[h, row] @ wide(k)[h, key])
    assert same_bits(out, want) and same_bits(lse, want_lse)


@pytest.mark.parametrize("bs", (16, 32))
def test_the_weights_are_e4m3_of_256_w_to_nearest_even_with_subnormals_and_flush(bs):
    a, ptrs, keys = pattern(bs)
    d, dv = 16, 8
    q, k = torch.zeros((H, a.num_rows, d), dtype=torch.uint8), torch.zeros((H, a.num_cols, d), dtype=torch.uint8)
    v = torch.zeros((H, a.num_cols, dv), dtype=torch.uint8)
    mask = np.full((a.num_blocks, bs, bs), -np.inf, dtype=np.float32)
    delta = np.linspace(0.0, 13.6, a.num_rows - bs).astype(np.float32)    # past ln 2^18 = 12.48: the flush; from 9.7 on: subnormals
    for row in range(bs, a.num_rows):
        r, i = divmod(row, bs)
        n = min(len(keys[r]), 32)
        pa, pb = (2 * i) % n, (2 * i + 5) % n                              # two keys of the first step, even and odd; the odd one is V = 1
        mask[ptrs[r] + pa // bs, i, pa % bs] = 0.0
        mask[ptrs[r] + pb // bs, i, pb % bs] = -delta[row - bs]
        v[:, keys[r][pb], 0] = 0x38
    out, _ = run(a, q, k, v, mask)
    table = torch.arange(0, 0x79, dtype=torch.uint8).view(F8).to(torch.float64).numpy()           # every e4m3 number from 0 to 256
    shown = table / (256.0 + table)                                        # 1 / 16 apart or more: out names its weight
    x = 256.0 * np.exp(-delta.astype(np.float64))
    e4m3 = lambda y: torch.from_numpy(y).to(torch.float32).to(F8).to(torch.float32).numpy()      # noqa: E731  torch's cast as the table
    allowed = np.stack([e4m3(x * f) for f in (1 - 2.0 ** -18, 1.0, 1 + 2.0 ** -18)])            # the fp32 exponential: (3 T + 2) u
    for h in range(H):
        near = np.abs(out[h, bs:, 0].astype(np.float64)[:, None] - shown[None, :]).argmin(axis=1)
        assert np.all(np.abs(out[h, bs:, 0] - shown[near]) <= 2.0 ** -22 * shown[near])
        got = table[near]
        assert np.all((got == allowed).any(axis=0)), (delta[~(got == allowed).any(axis=0)], got[~(got == allowed).any(axis=0)])
    assert np.all(got[delta > 12.6] == 0) and np.any((got > 0) & (got < 2.0 ** -6)) and got[0] == 256.0


def bounds(bs, ptrs, keys, q, k, v, mask, c, vs):
    """float64 out and lse with the limits of the header's NUMERICS, block row by block row."""
    q64, k64, v64 = wide(q), wide(k), wide(v)
    m, dv = q.shape[1], v.shape[2]
    out, lim, lse, lim_lse = (np.zeros((H, m, dv)), np.zeros((H, m, dv)), np.full((H, m), -np.inf), np.zeros((H, m)))
    chain = 2 * (1 if q.shape[2] <= 64 else 2)
    for h in range(H):
        for r in range(1, len(COUNTS)):
            rows, kk, vv, L = slice(r * bs, (r + 1) * bs), k64[h, keys[r]], v64[h, keys[r]], len(keys[r])
            with np.errstate(invalid="ignore"):
                z = c[h] * (q64[h, rows] @ kk.T) + mask_rows(bs, ptrs, mask, r)
            n = (q64[h, rows] != 0).astype(float) @ (kk != 0).astype(float).T + chain
            kept = np.isfinite(z)
            E = np.where(kept, n * U / (1 - n * U) * c[h] * (np.abs(q64[h, rows]) @ np.abs(kk).T) + 2 * u * np.abs(np.where(kept, z, 0)), 0)
            Er = E.max(axis=1, keepdims=True)
            zm = np.where(kept, z, -np.inf).max(axis=1, keepdims=True)
            w = np.exp(z - zm)
            P = w / w.sum(axis=1, keepdims=True)
            T = np.where(kept, zm - z, 0).max(axis=1, keepdims=True) + 2 * Er
            Pk = np.exp(2 * Er) * P
            f32 = (L + 8 * T + 16) * u
            dP = (2.0 ** -3 * Pk + 17 / 16 * 2.0 ** -18 * (1 + L * Pk)) / (1 - L * 2.0 ** -17) + (1 + 2.0 ** -3) * (f32 * Pk + 2.0 ** -126) + 2.0 ** -126
            nv = L + 2 * -(-L // 32) + 2
            out[h, rows] = P @ vv * vs[h]
            lim[h, rows] = ((dP + (np.exp(2 * Er) - 1) * P) @ np.abs(vv) + nv * U / (1 - nv * U) * ((Pk + dP) @ np.abs(vv))) * vs[h]
            lse[h, rows] = (zm + np.log(w.sum(axis=1, keepdims=True)))[:, 0]
            lim_lse[h, rows] = (Er + f32 + 2 * u * (np.log(L) + 1))[:, 0] + 2 * u * np.abs(lse[h, rows])
    return out, lim + 2 * u * np.abs(out), lse, lim_lse


@pytest.mark.parametrize("bs, d, dv", CASES, ids=IDS)
def test_random_e4m3_bytes_keep_the_bounds_of_the_header(bs, d, dv):
    a, ptrs, keys = pattern(bs)
    rng = np.random.default_rng(dv)
    q, k, v = rand_e4m3(rng, (H, a.num_rows, d)), rand_e4m3(rng, (H, a.num_cols, d)), rand_e4m3(rng, (H, a.num_cols, dv))
    mask = rng.normal(0, 2, (a.num_blocks, bs, bs)).astype(np.float32)
    mask[rng.random(mask.shape) < 0.2] = -np.inf
    qs, ks, vs = (torch.from_numpy(rng.uniform(0.5, 1.5, H) * s).float() for s in (2.0 ** -6, 2.0 ** -6, 1.0))
    c = (np.float32(d ** -0.5) * qs.numpy() * ks.numpy()).astype(np.float64)          # fp32 products in the kernel's order
    want, lim, want_lse, lim_lse = bounds(bs, ptrs, keys, q, k, v, mask, c, vs.numpy().astype(np.float64))
    out, lse = run(a, q, k, v, mask, q_scale=qs, k_scale=ks, v_scale=vs)
    err, err_lse = np.abs(out[:, bs:] - want[:, bs:]), np.abs(lse[:, bs:] - want_lse[:, bs:])
    print(f"b{bs} D={d} Dv={dv}: worst |out - exact| / bound = {np.max(err / lim[:, bs:]):.4f}, worst |lse - exact| / bound = "
          f"{np.max(err_lse / lim_lse[:, bs:]):.4f}")
    assert np.all(err <= lim[:, bs:]) and np.all(err_lse <= lim_lse[:, bs:])
    assert not out[:, :bs].view(np.uint8).any() and np.all(lse[:, :bs] == -np.inf), "an empty block row is +0 and -Inf"
    # tie rows: every kept key scores the same, and a constant column of V comes back to (L + 16) 2^-24, not to 2^-4
    const = rand_e4m3(rng, (H, 1, dv)).expand(H, a.num_cols, dv).contiguous()
    tie = np.where(np.isfinite(mask), np.float32(0), mask)
    out, _ = run(a, torch.zeros_like(q), k, const, tie, v_scale=2.0)
    L = np.repeat(np.array(COUNTS[1:]) * bs, bs)[None, :, None]
    assert np.all(np.abs(out[:, bs:] - 2 * wide(const)[:, :1]) <= (L + 16) * u * np.abs(2 * wide(const)[:, :1]))


@pytest.mark.parametrize("bs", (16, 32))
def test_special_values_and_plumbing(bs):
    a, ptrs, keys = pattern(bs)
    rng = np.random.default_rng(8)
    d, dv = 80, 72
    q, k, v = ints(rng, (H, a.num_rows, d), 3), ints(rng, (H, a.num_cols, d), 3), rand_e4m3(rng, (H, a.num_cols, dv))
    mask = rng.normal(0, 1, (a.num_blocks, bs, bs)).astype(np.float32)
    mask[ptrs[3]:ptrs[4], 5] = -np.inf                                     # row 5 of block row 3: nothing but -Inf
    one = torch.ones(H)
    out, lse = run(a, q, k, v, mask, scale=0.05)
    for other in (run(a, q, k, v, mask, scale=0.05, typed=True), run(a, q, k, v, mask, scale=0.05, q_scale=one, k_scale=1.0, v_scale=one)):
        assert same_bits(out, other[0]) and same_bits(lse, other[1])
    dead = 3 * bs + 5
    assert np.isnan(out[:, dead]).all() and np.all(lse[:, dead] == -np.inf) and np.isnan(out).sum() == H * dv and not np.isnan(lse).any()
    half, _ = run(a, q, k, v, mask, bf16=True, scale=0.05)
    ok = ~np.isnan(out)
    assert same_bits(half[ok], torch.from_numpy(out).to(torch.bfloat16).view(torch.int16).numpy()[ok]) and np.all((half[~ok] & 0x7FFF) > 0x7F80)
    # a NaN byte in K: the rows of head 1 under its block; one in V: that column of those rows, masked or not
    kn, vn = k.clone(), v.clone()
    col = int(a.block_col_idxs[ptrs[4] + 2])
    kn[1, col * bs + 3, 7] = 0x7F
    vn[0, col * bs + 9, 13] = 0xFF
    under = np.repeat([col * bs in keys[r] for r in range(len(COUNTS))], bs)
    got, got_lse = run(a, q, kn, vn, mask, scale=0.05)
    want_nan = np.isnan(out)
    want_nan[1, under] = True
    want_nan[0, under, 13] = True
    assert np.array_equal(np.isnan(got), want_nan) and np.array_equal(np.isnan(got_lse), np.stack([under & False, under]))
    assert same_bits(got[~want_nan], out[~want_nan])
    # a captured graph replays to the eager bits
    qd, kd, vd, md = (t.cuda() for t in (q, k, v, torch.from_numpy(mask)))
    eager = attn_bsr_fp8.attention_bsr_fp8(a, qd, kd, vd, mask=md, scale=0.05, v_scale=one.cuda())
    held, vs = torch.empty_like(eager), one.cuda()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        attn_bsr_fp8.attention_bsr_fp8(a, qd, kd, vd, mask=md, scale=0.05, v_scale=vs, out=held)
    for _ in range(2):
        held.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(held.view(torch.int32), eager.view(torch.int32)) and same_bits(eager.cpu().numpy(), out)
