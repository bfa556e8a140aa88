"""mispmm_bsrc_slots_fp8 on the GPU (include/mispmm_bsrc_fp8.h) against a float64 product of the exactly widened operands, on
the strips of tests/test_bsrc_fp8_cpu.py: all 8 of them (extra steps: wave 0 reduces) or the first 6 (none: the shared reduce
where C is fp32).  The random-value test PRINTS its worst |acc - exact| / (g_n S) at u = 2^-23 and at the header's u = 2^-14."""
import numpy as np
import pytest
import torch

from mispmm import bsrc_fp8, capi_bsrc_fp8

from test_bsrc_fp8_cpu import COUNTS, K, PAD, strips_matrix, to_bsr

pytestmark = pytest.mark.gpu

CASES = [(bs, bf16) for bs in (16, 32) for bf16 in (False, True)]
IDS = [f"b{bs}-{'c16' if bf16 else 'c32'}" for bs, bf16 in CASES]
F8 = torch.float8_e4m3fn
U = 2.0 ** -14                 # per addition (include/mispmm_bsrc_fp8.h, NUMERICS)
EMPTY = np.repeat(np.array(COUNTS) == 0, 16)
STEPS = np.repeat([1 + -(-max(0, -(-c // 32) - 4) // 3) for c in COUNTS], 16)[:, None]   # of the busiest wave of a strip

f8 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32)).to(F8).view(torch.uint8).numpy()                              # noqa: E731
widen = lambda x: torch.from_numpy(x).view(F8).to(torch.float64).numpy()                                                       # noqa: E731
bf16_bits = lambda x: torch.from_numpy(np.asarray(x)).to(torch.float32).to(torch.bfloat16).view(torch.int16).numpy()           # noqa: E731
same_bits = lambda got, want: np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))   # noqa: E731
device_a = lambda a, bs, rows=len(EMPTY): bsrc_fp8.DeviceBSRCSlotsFP8.from_blocks(*to_bsr(a[:rows], bs))                        # noqa: E731


def rand_e4m3(rng, shape, nonzero=False):
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    x[(x & 0x7F) == 0x7F] = 0x08
    x[((x & 0x7F) == 0) & nonzero] = 0x38
    return x


def run(d, b, bf16, rs=None, cs=None):
    """One launch on strided operands inside sentinels; asserts the tag and the sentinels, returns C [M, n] on the host."""
    m, n = d.num_rows, b.shape[1]
    bd = torch.full((K, n + 8), 0x7F, dtype=torch.uint8)                # gap columns hold NaN: never read
    bd[:, :n] = torch.from_numpy(b)
    sentinel = 0x5A5A if bf16 else -12345.0
    c = torch.full((m + 2, n + 8), sentinel, dtype=torch.int16 if bf16 else torch.float32, device="cuda")
    dev = lambda t: None if t is None else t.cuda()                      # noqa: E731
    bsrc_fp8.spmm_bsrc_slots_fp8(d, bd.cuda()[:, :n], dev(rs), dev(cs), out_bf16=bf16, out=c[1:m + 1, :n])
    share = not bf16 and d.num_steps == m // 4
    assert capi_bsrc_fp8.last_kernel() == (f"bsrc_slots_mfma_fp8<T8,{'c16' if bf16 else 'c32'},{'plain' if rs is None and cs is None else 'scales'},"
                                           f"{'share' if share else 'w0'}>")
    c = c.cpu()
    assert bool((c[0] == sentinel).all() and (c[-1] == sentinel).all() and (c[1:m + 1, n:] == sentinel).all()), "a sentinel around C was written"
    return c[1:m + 1, :n].contiguous().numpy()


@pytest.mark.parametrize("n", [8, 24, 136])
@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_small_integers_are_exact_bit_for_bit(bs, bf16, n):
    rng = np.random.default_rng(n)
    a = strips_matrix(lambda shape: f8(rng.choice([-8, -5, -3, -2, -1, 1, 2, 3, 4, 6, 7, 8], shape)))
    b = f8(rng.integers(-8, 9, (K, n)))
    for rows in (96, 128):                                                # without and with extra steps
        want = widen(a[:rows]) @ widen(b)
        got = run(device_a(a, bs, rows), b, bf16)
        assert a[-16:, K - 1].any() and np.abs(want).max() < 2 ** 24 and same_bits(got, bf16_bits(want) if bf16 else want.astype(np.float32))
        assert not got[EMPTY[:rows]].view(np.uint8).any(), "an empty strip is +0"


@pytest.mark.parametrize("bf16", [False, True], ids=["c32", "c16"])
def test_one_hot_tiles_pin_the_column_deal_the_byte_transpose_and_the_lane_layout(bf16):
    """512 strips, strip s = (i, k) with the tile e_i e_k^T in its first slot over the same 32 columns spread over K: its row i
    must be the B row of list position k, every other row +0."""
    rng = np.random.default_rng(1)
    spread, s = np.sort(rng.choice(K, 32, replace=False)), np.arange(512)
    cols, tiles = np.full((4 * 512, 32), PAD, dtype=np.uint32), np.zeros((4 * 512, 16, 32), dtype=np.uint8)
    cols[0::4], tiles[4 * s, s // 32, s % 32] = spread, 0x38              # 1.0
    b = rand_e4m3(rng, (K, 24), nonzero=True)
    assert len(np.unique(b, axis=0)) == K and np.diff(spread).max() > 1
    d = bsrc_fp8.DeviceBSRCSlotsFP8(512 * 16, K, 4 * 512, 512, torch.zeros(513, dtype=torch.int32, device="cuda"),
                                    torch.from_numpy(cols.view(np.int32)).cuda(), torch.from_numpy(tiles).cuda())
    got = run(d, b, bf16).reshape(512, 16, 24)
    want = np.zeros((512, 16, 24))
    want[s, s // 32] = widen(b)[spread[s % 32]]
    want = bf16_bits(want) if bf16 else want.astype(np.float32)
    wrong = [(int(t) // 32, int(t) % 32) for t in s if not same_bits(got[t], want[t])]
    assert not wrong, f"{len(wrong)} of 512 slots (i, k) misplaced, the first: {wrong[:4]}"


@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_random_e4m3_values_keep_the_bound_of_the_header(bs, bf16):
    rng = np.random.default_rng(11)
    a = strips_matrix(lambda shape: rand_e4m3(rng, shape, nonzero=True))
    d = device_a(a, bs)
    ones = lambda x: np.where(x & 0x7F, 0x38, 0).astype(np.uint8)         # noqa: E731  1.0 where the value is not zero
    for n in (24, 136):
        b = rand_e4m3(rng, (K, n))
        want, scale = widen(a) @ widen(b), widen(a & 0x7F) @ widen(b & 0x7F)
        terms = widen(ones(a)) @ widen(ones(b)) + STEPS + 3
        lim = terms * U / (1 - terms * U) * scale
        got = run(d, b, bf16)
        if bf16:
            f = lambda bits: torch.from_numpy(bits).view(torch.bfloat16).to(torch.float64).numpy()   # noqa: E731
            assert np.all((f(bf16_bits(want - lim)) <= f(got)) & (f(got) <= f(bf16_bits(want + lim))))
        else:
            err, live = np.abs(got.astype(np.float64) - want), scale > 0
            bf16_model = (terms * 2.0 ** -23 / (1 - terms * 2.0 ** -23) * scale)[live]
            print(f"b{bs} N={n}: worst |err| / (g_n S) = {np.max(err[live] / bf16_model):.4f} at u = 2^-23, "
                  f"{np.max(err[live] / lim[live]):.4f} at u = 2^-14, n up to {int(terms.max())}")
            assert np.all(err <= lim)


@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_scales_are_two_separate_fp32_multiplies_and_none_is_no_multiply(bs, bf16):
    rng = np.random.default_rng(5)
    a, b = strips_matrix(lambda shape: rand_e4m3(rng, shape, nonzero=True)), rand_e4m3(rng, (K, 136))
    free = lambda k: torch.from_numpy(rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)).float()   # noqa: E731
    bits = lambda t: t.to(torch.bfloat16).view(torch.int16).numpy() if bf16 else t.numpy()             # noqa: E731
    for rows in (96, 128):                                                # the shared reduce (fp32 C) and wave 0's
        d = device_a(a, bs, rows)
        c0 = torch.from_numpy(run(d, b, False))
        assert same_bits(run(d, b, bf16), bits(c0))
        for rs, cs in ((free(rows), free(136)), (free(rows), None), (None, free(136))):
            want = c0 if rs is None else c0 * rs[:, None]
            want = want.clone() if cs is None else want * cs[None, :]
            want[torch.from_numpy(EMPTY[:rows])] = 0.0                    # an empty strip: +0 whatever the scales
            assert same_bits(run(d, b, bf16, rs, cs), bits(want)), (rows, rs is None, cs is None)


@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_a_nan_byte_of_b_reaches_the_16_rows_of_the_strips_that_occupy_its_column_and_nothing_else(bs, bf16):
    rng = np.random.default_rng(7)
    a, b = strips_matrix(lambda shape: rand_e4m3(rng, shape, nonzero=True)), rand_e4m3(rng, (K, 24))
    occ = (a.reshape(-1, 16, K) & 0x7F).any(axis=1)
    r = int(np.flatnonzero(occ[3] & ~occ[2])[0])                          # strips 2 and 3 share their 32 x 32 blocks
    a[48:56, r], a[56, r] = 0, 0x38                                       # stored zeros in an occupied column: NaN all the same
    d = device_a(a, bs)
    clean = run(d, b, bf16)
    b[r, 13] = 0xFF
    mask = np.zeros(clean.shape, dtype=bool)
    mask[np.repeat(occ[:, r], 16), 13] = True
    assert mask[48:64, 13].all() and not mask[32:48].any() and 16 < mask.sum() < 16 * 6
    got = run(d, b, bf16)
    assert np.array_equal((got & 0x7FFF) > 0x7F80 if bf16 else np.isnan(got), mask)
    assert same_bits(got[~mask], clean[~mask])
