"""mispmm_bsr_fp8 on the GPU (include/mispmm_bsr_fp8.h) against a float64 product of the exactly widened operands.  The
random-value test PRINTS its worst |acc - exact| / (g_n S) at u = 2^-23, the bf16 products' model, which the 8-bit instruction
does not keep (134.0 here on an MI355X at 16 x 16, N = 272): U is the header's measured one."""
import numpy as np
import pytest
import torch

from mispmm import bsr_fp8, capi_bsr_fp8, ops

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 5, 9)      # blocks per block row: empty, half a pair, a pair, an odd pair count, a second round over 4 waves
KB = 10                       # block columns; the last one is used by the longest row
CASES = [(bs, bf16) for bs in (16, 32) for bf16 in (False, True)]
IDS = [f"b{bs}-{'c16' if bf16 else 'c32'}" for bs, bf16 in CASES]
F8 = torch.float8_e4m3fn
U = 2.0 ** -14                 # per addition (include/mispmm_bsr_fp8.h, NUMERICS): measured, see above


def pattern(bs, cols=None):
    rng = np.random.default_rng(3)
    if cols is None:
        cols = [np.sort(rng.choice(KB - 1, n, replace=False)) for n in COUNTS]
        cols[-1][-1] = KB - 1
    ptrs = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    idxs = np.concatenate(cols).astype(np.int64)
    a = ops.DeviceBSR(len(cols) * bs, (int(idxs.max()) + 1) * bs, bs, bs, len(idxs), torch.tensor(ptrs, dtype=torch.int32, device="cuda"),
                      torch.tensor(idxs, dtype=torch.int32, device="cuda"), None)
    return a, ptrs, idxs


def exact(bs, ptrs, idxs, blocks, b):
    """The float64 product block by block: an absent block multiplies nothing, a stored zero multiplies."""
    a64, b64 = (t.view(F8).to(torch.float64).numpy() for t in (blocks.view(-1, bs, bs), b))
    out = np.zeros(((len(ptrs) - 1) * bs, b.shape[1]))
    with np.errstate(invalid="ignore"):
        for r in range(len(ptrs) - 1):
            for e in range(ptrs[r], ptrs[r + 1]):
                out[r * bs:(r + 1) * bs] += a64[e] @ b64[idxs[e] * bs:(idxs[e] + 1) * bs]
    return out


def bf16_bits(x64):
    return torch.from_numpy(np.asarray(x64)).to(torch.float32).to(torch.bfloat16).view(torch.int16).numpy()


def run(a, blocks, b, n, bf16, rs=None, cs=None):
    """One launch on strided operands inside sentinels; asserts the tag and the sentinels, returns C [M, n] on the host."""
    bs, m = a.block_row_size, a.num_rows
    ldb = ldc = n + (16 if n % 16 == 0 else 8)
    bd = torch.full((b.shape[0], ldb), 0x7F, dtype=torch.uint8)         # gap columns hold NaN: never read
    bd[:, :n] = b
    sentinel = 0x5A5A if bf16 else -12345.0
    c = torch.full((m + 2, ldc), sentinel, dtype=torch.int16 if bf16 else torch.float32, device="cuda")
    dev = lambda t: None if t is None else t.cuda()                      # noqa: E731
    bsr_fp8.spmm_bsr_fp8(a, blocks.cuda(), bd.cuda()[:, :n], dev(rs), dev(cs), out_bf16=bf16, out=c[1:m + 1, :n])
    tag = f"bsr_mfma_fp8<b{bs},T{16 if n >= 256 and n % 16 == 0 else 8},{'c16' if bf16 else 'c32'},{'plain' if rs is None and cs is None else 'scales'}>"
    assert capi_bsr_fp8.last_kernel() == tag
    c = c.cpu()
    assert bool((c[0] == sentinel).all() and (c[-1] == sentinel).all() and (c[1:m + 1, n:] == sentinel).all()), "a sentinel around C was written"
    return c[1:m + 1, :n].contiguous()


def rand_e4m3(rng, shape):
    """Finite e4m3 bytes, every exponent and the subnormals with the same weight."""
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    x[(x & 0x7F) == 0x7F] = 0x08
    return torch.from_numpy(x)


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


@pytest.mark.parametrize("n", [8, 24, 136, 272])
@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_small_integers_are_exact_bit_for_bit(bs, bf16, n):
    a, ptrs, idxs = pattern(bs)
    rng = np.random.default_rng(n)
    blocks = torch.from_numpy(rng.integers(-8, 9, a.num_blocks * bs * bs).astype(np.float32)).to(F8).view(torch.uint8)
    b = torch.from_numpy(rng.integers(-8, 9, (a.num_cols, n)).astype(np.float32)).to(F8).view(torch.uint8)
    want = exact(bs, ptrs, idxs, blocks, b)
    assert np.abs(want).max() < 2 ** 24 and idxs.max() == KB - 1 == a.num_cols // bs - 1
    got = run(a, blocks, b, n, bf16).numpy()
    assert same_bits(got, bf16_bits(want) if bf16 else want.astype(np.float32))
    assert not np.any(got[:bs].view(np.uint8)), "an empty block row is +0"


@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_one_hot_operands_pin_the_lane_layout_and_the_byte_transpose(bs, bf16):
    """A = e_i e_k^T, B = e_k (1 .. 8): C must be row i = 1 .. 8, for every slot (i, k) of one MFMA step."""
    cols = [np.arange(32 // bs)]                                          # a pair of 16 x 16 blocks, or one 32 x 32 block
    a, _, _ = pattern(bs, cols)
    slots = [(i, k) for i in range(bs) for k in range(32)]
    blocks = torch.zeros((len(slots), 32 // bs, bs, bs), dtype=torch.uint8)
    b = torch.zeros((len(slots), 32, 8), dtype=torch.uint8)
    one_to_eight = torch.arange(1, 9, dtype=torch.float32).to(F8).view(torch.uint8)
    for s, (i, k) in enumerate(slots):
        blocks[s, k // bs, i, k % bs] = 0x38                              # 1.0
        b[s, k] = one_to_eight
    blocks, b = blocks.cuda(), b.cuda()
    out = torch.full((len(slots), bs, 8), 0x5A5A if bf16 else -7.0, dtype=torch.int16 if bf16 else torch.float32, device="cuda")
    for s in range(len(slots)):
        bsr_fp8.spmm_bsr_fp8(a, blocks[s], b[s], out_bf16=bf16, out=out[s])
    got = ops.bf16_to_f32(out).cpu() if bf16 else out.cpu()
    want = torch.zeros((len(slots), bs, 8))
    want[torch.arange(len(slots)), torch.arange(len(slots)) // 32] = torch.arange(1.0, 9.0)
    wrong = [slots[s] for s in range(len(slots)) if not torch.equal(got[s], want[s])]
    assert not wrong, f"{len(wrong)} of {len(slots)} slots (i, k) misplaced, the first: {wrong[:4]}"


@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_random_e4m3_values_keep_the_bound_of_the_header(bs, bf16):
    a, ptrs, idxs = pattern(bs)
    rng = np.random.default_rng(11)
    counts = np.diff(ptrs)
    steps = np.repeat(np.ceil(np.ceil(counts / 2) / 4) if bs == 16 else np.ceil(counts / 4), bs)[:, None]
    for n in (24, 272):
        blocks, b = rand_e4m3(rng, a.num_blocks * bs * bs), rand_e4m3(rng, (a.num_cols, n))
        want = exact(bs, ptrs, idxs, blocks, b)
        mag = lambda t: t & 0x7F                                          # noqa: E731  |x|: the sign bit cleared
        scale = exact(bs, ptrs, idxs, mag(blocks), mag(b))
        ones = lambda t: torch.where((t & 0x7F) != 0, 0x38, 0).to(torch.uint8)   # noqa: E731  1.0 where the value is not zero
        terms = exact(bs, ptrs, idxs, ones(blocks), ones(b)) + steps + 3
        lim = terms * U / (1 - terms * U) * scale
        got = run(a, blocks, b, n, bf16).numpy()
        if bf16:
            f = lambda bits: torch.from_numpy(bits).view(torch.bfloat16).to(torch.float64).numpy()   # noqa: E731
            assert np.all((f(bf16_bits(want - lim)) <= f(got)) & (f(got) <= f(bf16_bits(want + lim))))
        else:
            err = np.abs(got.astype(np.float64) - want)
            bf16_model = (terms * 2.0 ** -23 / (1 - terms * 2.0 ** -23) * scale)[scale > 0]
            print(f"b{bs} N={n}: worst |err| / (g_n S) = {np.max(err[scale > 0] / bf16_model):.4f} at u = 2^-23, "
                  f"{np.max(err[scale > 0] / lim[scale > 0]):.4f} at u = 2^-14, n up to {int(terms.max())}")
            assert np.all(err <= lim)


@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_scales_are_two_separate_fp32_multiplies_and_none_is_no_multiply(bs, bf16):
    a, _, _ = pattern(bs)
    rng = np.random.default_rng(5)
    for n in (24, 272):
        blocks, b = rand_e4m3(rng, a.num_blocks * bs * bs), rand_e4m3(rng, (a.num_cols, n))
        c0 = run(a, blocks, b, n, False)
        pow2 = lambda k: torch.from_numpy(2.0 ** rng.integers(-3, 4, k)).float() * torch.from_numpy(rng.choice([-1.0, 1.0], k)).float()   # noqa: E731
        free = lambda k: torch.from_numpy(rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)).float()                                   # noqa: E731
        for rs, cs in ((pow2(a.num_rows), pow2(n)), (free(a.num_rows), free(n)), (free(a.num_rows), None), (None, free(n))):
            want = c0 if rs is None else c0 * rs[:, None]
            want = want.clone() if cs is None else want * cs[None, :]
            want[:bs] = 0.0                                               # the empty block row: +0 whatever the scales
            got = run(a, blocks, b, n, bf16, rs, cs)
            assert same_bits(got.numpy(), want.to(torch.bfloat16).view(torch.int16).numpy() if bf16 else want.numpy())


@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_a_nan_byte_reaches_its_rows_or_columns_and_nothing_else(bs, bf16):
    a, ptrs, idxs = pattern(bs)
    rng = np.random.default_rng(7)
    n = 24
    blocks, b = rand_e4m3(rng, a.num_blocks * bs * bs), rand_e4m3(rng, (a.num_cols, n))
    e, z = int(ptrs[3]) + 1, int(ptrs[4]) + 2                              # a block of the row of 5, a block of the row of 9
    krow = int(idxs[z]) * bs + 9                                           # a B row under block z
    blocks.view(-1, bs, bs)[z, :, 9] = 0                                   # explicit zeros of A against that row: NaN all the same
    clean = run(a, blocks, b, n, bf16).numpy()
    blocks.view(-1, bs, bs)[e, 3, 5] = 0x7F
    b[krow, 13] = 0xFF
    mask = np.isnan(exact(bs, ptrs, idxs, blocks, b))
    under = [r for r in range(len(COUNTS)) if krow // bs in idxs[ptrs[r]:ptrs[r + 1]]]
    assert mask[3 * bs + 3].all() and mask[4 * bs:, 13].all() and mask.sum() == n + bs * len(under) - (3 in under)
    got = run(a, blocks, b, n, bf16).numpy()
    nan = (got & 0x7FFF) > 0x7F80 if bf16 else np.isnan(got)
    assert np.array_equal(nan, mask)
    assert same_bits(got[~mask], clean[~mask])


@pytest.mark.parametrize("bs, bf16", CASES, ids=IDS)
def test_float8_tensors_and_their_bytes_agree_and_a_graph_replays_to_the_same_bits(bs, bf16):
    a, _, _ = pattern(bs)
    rng = np.random.default_rng(9)
    n = 136
    blocks, b = rand_e4m3(rng, a.num_blocks * bs * bs).cuda(), rand_e4m3(rng, (a.num_cols, n)).cuda()
    rs = torch.from_numpy(rng.uniform(0.5, 2.0, a.num_rows)).float().cuda()
    eager = bsr_fp8.spmm_bsr_fp8(a, blocks, b, rs, out_bf16=bf16)
    assert capi_bsr_fp8.last_kernel() == f"bsr_mfma_fp8<b{bs},T8,{'c16' if bf16 else 'c32'},scales>"
    typed = bsr_fp8.spmm_bsr_fp8(a, blocks.view(F8), b.view(F8), rs, out_bf16=bf16)
    assert torch.equal(eager, typed)
    out = torch.empty_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bsr_fp8.spmm_bsr_fp8(a, blocks, b, rs, out_bf16=bf16, out=out)
    for _ in range(2):
        out.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
