"""The matrices of the FAST-chain tests (tests/test_gpu_fast_chain.py), built on the host from fixed seeds so that the CPU
suite (tests/test_fma_chain_cpu.py) can check the precondition -- _fma_chain.corpus_is_sharp -- on exactly the data the GPU
tests launch.  Values and B come from _fma_chain.sharp_values.  Shapes stay small: at most 700 rows, 900 columns, N <= 512."""
import numpy as np

from mispmm import formats

from _fma_chain import sharp_values

UNIFORM_WIDTHS = (1, 7, 8, 9, 14, 15, 16, 17, 23)      # the slot counts test_uniform_rows_every_slot_count walks, and 1
MAX_N = 512


def csr_from_lens(rng, m, k, lens):
    lens = np.minimum(np.asarray(lens, dtype=np.int64), k)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cols = np.concatenate([np.sort(rng.choice(k, size=int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)])
    return formats.CSR(m, k, ptr, cols.astype(np.uint32), sharp_values(rng, int(ptr[-1]), np.float32))


def uniform(width):
    rng = np.random.default_rng(9100 + width)
    return csr_from_lens(rng, 257, 600, [width] * 257)


def uniform_sum_only(width):
    """nnz divisible by M, rows NOT uniform: what the general entry point's bet gets wrong (built as in
    test_fuzz_plan_order_and_general_entry_bet: entries moved between rows, the total kept)."""
    rng = np.random.default_rng(9200 + width)
    lens = np.full(257, width, dtype=np.int64)
    for _ in range(60):
        src, dst = rng.integers(0, 257, size=2)
        move = int(rng.integers(0, lens[src] + 1))
        lens[src] -= move
        lens[dst] += move
    assert lens.sum() == 257 * width and lens.min() >= 0 and not np.all(lens == width)
    return csr_from_lens(rng, 257, 600, lens)


def ragged():
    rng = np.random.default_rng(9301)
    m = 300
    lens = rng.integers(1, 13, size=m)
    empty = rng.random(m) < 0.4
    empty[[0, m - 1]] = True
    empty[100:112] = True                                # an interior run of empty rows
    empty[201:204] = True
    lens[empty] = 0
    return csr_from_lens(rng, m, 500, lens)


def long_tail():
    rng = np.random.default_rng(9403)
    m = 200
    lens = np.where(rng.random(m) < 0.1, rng.integers(60, 401, size=m), rng.integers(0, 4, size=m))
    csr = csr_from_lens(rng, m, 900, lens)
    assert csr.nnz // m < 24 and lens.max() > 128         # mean below the long-row dispatch, a row past the 128-entry share length
    return csr


def long_mean():
    rng = np.random.default_rng(9501)
    m = 96
    lens = rng.integers(24, 423, size=m)
    lens[[0, 5, m - 1]] = [24, 422, 32]
    csr = csr_from_lens(rng, m, 900, lens)
    assert csr.nnz // m >= 24
    return csr


def long_only():
    """The rows of long_mean of more than 40 entries: every row beyond the two-body launch's threshold."""
    rng = np.random.default_rng(9502)
    base = np.diff(long_mean().row_ptrs.astype(np.int64))
    lens = base[base > 40]
    return csr_from_lens(rng, lens.shape[0], 900, lens)


def dense_regime():
    rng = np.random.default_rng(9601)
    mask = rng.random((128, 300)) < 0.3
    csr = csr_from_lens(rng, 128, 300, mask.sum(axis=1))
    csr.col_idxs[:] = np.nonzero(mask)[1].astype(np.uint32)   # ascending inside a row: the panel order is the storage order
    return csr


BSR_SHAPES = {(1, 1): (60, 80, 30), (4, 4): (24, 30, 5), (3, 5): (20, 25, 4), (16, 16): (6, 8, 3), (32, 32): (3, 6, 2)}   # (Mb, Kb, most blocks per block row)


def random_bsr(rng, br, bc, mb, kb, max_blocks, empty_rows=(1,)):
    """Unsorted block columns, roughly half of the block entries explicit zeros, empty block rows."""
    ptrs, idxs = [0], []
    for r in range(mb):
        cnt = 0 if r in empty_rows and mb > 1 else int(rng.integers(1, min(kb, max_blocks) + 1))
        idxs += list(rng.permutation(kb)[:cnt])
        ptrs.append(len(idxs))
    data = np.where(rng.random((len(idxs), br, bc)) < 0.5, sharp_values(rng, (len(idxs), br, bc), np.float32), np.float32(0))   # +0, never -0
    return formats.BSR(mb * br, kb * bc, int(data.size), br, bc, np.array(ptrs, np.uint32), np.array(idxs, np.uint32), data.astype(np.float32))


def bsr(br, bc):
    mb, kb, most = BSR_SHAPES[(br, bc)]
    return random_bsr(np.random.default_rng(9700 + 37 * br + bc), br, bc, mb, kb, most)


def bsr_long():
    """16 x 16 blocks, 6 .. 12 blocks per block row: zero-skipping lists of about 48 .. 96 entries per row."""
    rng = np.random.default_rng(9801)
    ptrs, idxs = [0], []
    for r in range(5):
        idxs += list(rng.permutation(14)[:int(rng.integers(6, 13))])
        ptrs.append(len(idxs))
    data = np.where(rng.random((len(idxs), 16, 16)) < 0.5, sharp_values(rng, (len(idxs), 16, 16), np.float32), np.float32(0))
    return formats.BSR(80, 224, int(data.size), 16, 16, np.array(ptrs, np.uint32), np.array(idxs, np.uint32), data.astype(np.float32))


_B = {}


def dense_b(k, n, dtype=np.float32):
    """The first n columns of one seeded [k, MAX_N] operand per (k, dtype), copied contiguous."""
    key = (int(k), np.dtype(dtype))
    if key not in _B:
        _B[key] = sharp_values(np.random.default_rng(9900 + int(k)), (int(k), MAX_N), dtype)
    return np.ascontiguousarray(_B[key][:, :n])


def all_csr_cases():
    """(name, CSR) of every CSR matrix the GPU tests launch (W = 1 has nothing to discriminate and is left out)."""
    cases = [(f"uniform W={w}", uniform(w)) for w in UNIFORM_WIDTHS if w > 1]
    cases += [(f"uniform-sum W={w}", uniform_sum_only(w)) for w in (9, 14)]
    cases += [("ragged", ragged()), ("long tail", long_tail()), ("long mean", long_mean()), ("long only", long_only()),
              ("dense regime", dense_regime())]
    return cases


# ---------------------------------------------------------------------------------------------- the seeded FAST fuzz
def fuzz_csr(seed):
    """test_gpu_fuzz.rand_csr's four row-length styles on its shapes, with sharp values.  Returns (csr, b)."""
    rng = np.random.default_rng(11000 + seed)
    m, k, n = int(rng.integers(1, 300)), int(rng.integers(1, 500)), int(rng.integers(1, 300))
    style = rng.integers(0, 4)
    if style == 0:
        lens = rng.integers(0, min(k, 6) + 1, size=m)
    elif style == 1:
        lens = np.minimum(k, rng.geometric(0.08, size=m) - 1)
    elif style == 2:
        lens = np.full(m, min(k, int(rng.integers(1, 40))))
    else:
        lens = np.where(rng.random(m) < 0.1, min(k, int(rng.integers(60, 400))), rng.integers(0, 4, size=m))
    csr = csr_from_lens(rng, m, k, lens)
    return csr, sharp_values(rng, (k, n), np.float32)


def fuzz_bsr(seed):
    """test_fuzz_bsr's generator with sharp values.  Returns (bsr, b)."""
    rng = np.random.default_rng(12000 + seed)
    br = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 32]))
    bc = br if rng.random() < 0.7 else int(rng.choice([1, 2, 3, 4, 7, 8]))
    mb, kb, n = int(rng.integers(1, 12)), int(rng.integers(1, 14)), int(rng.integers(1, 200))
    ptrs, idxs = [0], []
    for _ in range(mb):
        cnt = int(rng.integers(0, kb + 1))
        idxs += list(rng.permutation(kb)[:cnt])
        ptrs.append(len(idxs))
    data = np.where(rng.random((len(idxs), br, bc)) < 0.5, sharp_values(rng, (len(idxs), br, bc), np.float32), np.float32(0))
    bsr_ = formats.BSR(mb * br, kb * bc, int(data.size), br, bc, np.array(ptrs, np.uint32), np.array(idxs, np.uint32), data)
    return bsr_, sharp_values(rng, (kb * bc, n), np.float32)


# Seeds whose draw is sharp (checked on the CPU by test_fma_chain_cpu.py: a draw of empty or one-entry rows discriminates
# nothing).  The first 12 / 8 run by default; MISPMM_FUZZ_SCALE takes more from the front of the lists.
FUZZ_CSR_SEEDS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49)
FUZZ_BSR_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32)


def fuzz_seeds(pool, count):
    assert count <= len(pool), f"MISPMM_FUZZ_SCALE asks for {count} seeds, {len(pool)} are vetted: add vetted seeds to tests/_fast_corpus.py"
    return list(pool[:count])
