"""The FAST contract's CPU restatement (oracle.rows_fma) pinned against exact rational arithmetic, the row-list builders
pinned against the order the REFERENCE oracle adds in, and the precondition of tests/test_gpu_fast_chain.py -- the corpus
is sharp -- checked here, so that a GPU session never starts on data that could not tell a wrong kernel from a right one.
No GPU."""
import numpy as np
import pytest

from mispmm import formats

import _fast_corpus as corpus
import _fma_chain as fc
from _bits import assert_same_bits
from _ref64 import assert_same_bits64

F32 = np.float32


def f32_bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def same_bits(got, want, what):
    (assert_same_bits if want.dtype == np.float32 else assert_same_bits64)(got, want, what)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rows_fma_equals_the_exact_chain_on_random_row_lists(oracle, dtype):
    for seed, lens, k, n in ((1, [0, 1, 2, 5, 9], 6, 4), (2, [3, 0, 0, 17, 1, 2], 9, 3), (3, [40], 40, 2)):
        rng = np.random.default_rng(seed)
        rp = np.concatenate([[0], np.cumsum(lens)])
        cols = rng.integers(0, k, size=rp[-1])                       # unsorted, repeated columns: list order is all that counts
        vals, b = fc.sharp_values(rng, int(rp[-1]), dtype), fc.sharp_values(rng, (k, n), dtype)
        same_bits(oracle.rows_fma(rp, cols, vals, b), fc.chain_exact(rp, cols, vals, b), f"{np.dtype(dtype).name} seed {seed}")


def test_rows_fma_refuses_mixed_or_foreign_dtypes(oracle):
    rp, cols = [0, 1], [0]
    with pytest.raises(TypeError):
        oracle.rows_fma(rp, cols, np.ones(1, np.float32), np.ones((1, 1), np.float64))
    with pytest.raises(TypeError):
        oracle.rows_fma(rp, cols, np.ones(1, np.float64), np.ones((1, 1), np.float32))
    with pytest.raises(TypeError):
        oracle.rows_fma(rp, cols, np.ones(1, np.float16), np.ones((1, 1), np.float16))
    with pytest.raises(ValueError):
        oracle.rows_fma(rp, [3], np.ones(1, np.float32), np.ones((1, 1), np.float32))


def test_rows_fma_pins_fusion_width_order_and_start_discriminators(oracle):
    """Hand-made elements on which each way of being wrong gives other bits; the expected bits are written out."""
    # (1) fused or not: a = 1 + 2^-12, a * a = 1 + 2^-11 + 2^-24 is a tie in float32 and rounds to 1 + 2^-11;
    #     fma(a, a, -1) = 2^-11 + 2^-24 keeps the last bit, (float)(a * a) - 1 = 2^-11 has lost it
    a = f32_bits(0x3F800800)[0]
    got = oracle.rows_fma([0, 2], [0, 1], np.array([-1.0, a], F32), np.array([[1.0], [a]], F32))
    assert_same_bits(got, f32_bits(0x3A000400).reshape(1, 1), "fused")
    assert_same_bits(fc.chain_unfused([0, 2], [0, 1], np.array([-1.0, a], F32), np.array([[1.0], [a]], F32)), f32_bits(0x3A000000).reshape(1, 1),
                     "the unfused chain")
    assert_same_bits(fc.chain_exact([0, 2], [0, 1], np.array([-1.0, a], F32), np.array([[1.0], [a]], F32)), got, "exact")

    # (2) one rounding, not two: a = 1 + 2^-15, b = (1 - 2^-15) 2^-24, c = 1 + 2^-23.  a b + c = c + 2^-24 - 2^-54 lies just
    #     below the midpoint of two floats: fmaf rounds down to c; rounded to double first it IS the midpoint (2^-54 is lost) and
    #     the second rounding goes to even, one ulp up
    a, b, c = f32_bits(0x3F800100, 0x337FFE00, 0x3F800001)
    vals, bb = np.array([1.0, a], F32), np.array([[c], [b]], F32)
    got = oracle.rows_fma([0, 2], [0, 1], vals, bb)
    assert_same_bits(got, f32_bits(0x3F800001).reshape(1, 1), "single rounding")
    assert_same_bits(fc.chain_exact([0, 2], [0, 1], vals, bb), got, "exact")
    twice = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    assert twice.view(np.uint32) == 0x3F800002                      # what a kernel that went through double would return

    # (3) order: three entries whose chain backwards ends one ulp away
    vals = f32_bits(0x3F5FCE72, 0xC0974220, 0x41148B44)
    bb = f32_bits(0x3E9C6FE5, 0x4037FDBC, 0xC02A39BC).reshape(3, 1)
    assert_same_bits(oracle.rows_fma([0, 3], [0, 1, 2], vals, bb), f32_bits(0xC2180F8C).reshape(1, 1), "list order")
    assert_same_bits(oracle.rows_fma([0, 3], [2, 1, 0], vals[::-1].copy(), bb), f32_bits(0xC2180F8D).reshape(1, 1), "reversed list")
    assert_same_bits(fc.chain_exact([0, 3], [0, 1, 2], vals, bb), f32_bits(0xC2180F8C).reshape(1, 1), "exact")
    rrp, rcols, rvals = fc.reversed_rows([0, 3], [0, 1, 2], vals)
    assert rcols.tolist() == [2, 1, 0] and np.array_equal(rvals, vals[::-1])

    # (4) the chain starts at +0: fma(-0, x, +0) = +0 (a chain started from its first product would keep -0); an empty
    #     row is +0; and -0 products all the way still give +0
    vals, bb = np.array([-0.0, 0.0, -0.0], F32), np.array([[3.0], [-2.0], [5.0]], F32)
    for rp, cols in (([0, 1], [0]), ([0, 3], [0, 1, 2]), ([0, 0], [])):
        got = oracle.rows_fma(rp, cols, vals, bb)
        assert got.view(np.uint32).tolist() == [[0]], (rp, got)
        assert_same_bits(fc.chain_exact(rp, cols, vals, bb), got, "exact zero")
    assert fc.fma_exact(F32(-0.0), F32(3.0), F32(-0.0), F32).view(np.uint32) == 0x80000000   # only -0 + -0 is -0

    # (5) Inf and NaN propagate: Inf * 0 = NaN, Inf - Inf = NaN, a finite tail after an Inf stays Inf
    inf, nan = F32(np.inf), F32(np.nan)
    vals = np.array([1.0, 2.0, 1.0, 1.0, 0.0, 1.0, 1.0], F32)
    bb = np.array([[inf, 1.0], [-inf, 2.0], [nan, 3.0]], F32)
    rp, cols = [0, 2, 4, 5, 7], [0, 1, 0, 2, 0, 0, 1]
    got = oracle.rows_fma(rp, cols, vals, bb)
    want = np.array([[nan, 5.0], [nan, 4.0], [nan, 0.0], [nan, 3.0]], F32)
    assert_same_bits(got, want, "non-finite")
    assert_same_bits(fc.chain_exact(rp, cols, vals, bb), want, "exact non-finite")
    got = oracle.rows_fma([0, 2], [0, 1], np.array([1.0, 7.0], F32), np.array([[inf], [3.0]], F32))
    assert got.view(np.uint32).tolist() == [[0x7F800000]]

    # the same fusion discriminator in float64: a = 1 + 2^-27
    a = np.float64(1 + 2.0 ** -27)
    got = oracle.rows_fma([0, 2], [0, 1], np.array([-1.0, a]), np.array([[1.0], [a]]))
    assert got[0, 0].hex() == "0x1.0000001000000p-26" and (a * a - 1.0).hex() == "0x1.0000000000000p-26"
    assert_same_bits64(fc.chain_exact([0, 2], [0, 1], np.array([-1.0, a]), np.array([[1.0], [a]])), got, "exact f64")


def ragged_host_matrix():
    rng = np.random.default_rng(77)
    lens = [0, 3, 1, 0, 0, 9, 2, 5, 0, 4, 7, 0]
    return corpus.csr_from_lens(rng, len(lens), 20, lens), fc.sharp_values(rng, (20, 5), np.float32)


def test_row_lists_reproduce_the_order_the_reference_oracle_adds_in(oracle):
    """For every format the unfused float32 chain over the list is the REFERENCE oracle's result, bit for bit: the lists
    restate the order of addition and nothing else."""
    csr, b = ragged_host_matrix()
    rng = np.random.default_rng(78)
    coo = formats.csr_to_coo(csr)
    shuffle = rng.permutation(coo.nnz)                              # file order: rows interleaved, a row's entries not by column
    coo = formats.COO(coo.num_rows, coo.num_cols, coo.row_idxs[shuffle], coo.col_idxs[shuffle], coo.data[shuffle])
    assert_same_bits(fc.chain_unfused(*fc.coo_rows(coo), b), oracle.spmm_coo(coo.num_rows, coo.row_idxs, coo.col_idxs, coo.data, b), "COO")
    ellc = formats.csr_to_ell_colmajor(csr)
    assert_same_bits(fc.chain_unfused(*fc.ell_colmajor_rows(ellc), b), oracle.spmm_ell_colmajor(ellc.num_rows, ellc.row_idxs, ellc.data, b), "ELL")
    ellr = formats.ell_colmajor_to_rowmajor(ellc)
    rows_r, rows_c = fc.ell_rowmajor_rows(ellr), fc.ell_colmajor_rows(ellc)
    assert all(np.array_equal(x, y) for x, y in zip(rows_r, rows_c))   # the row-major form keeps the column-major order of addition
    for br, bc in ((1, 1), (4, 4), (3, 5)):
        bsr = corpus.random_bsr(rng, br, bc, 5, 4, 3)
        bb = fc.sharp_values(rng, (bsr.num_cols, 5), np.float32)
        ref = oracle.spmm_bsr(bsr.num_rows, br, bc, bsr.block_row_ptrs, bsr.block_col_idxs, bsr.data, bb)
        kept, skipped = fc.bsr_rows(bsr, skip_zeros=False), fc.bsr_rows(bsr, skip_zeros=True)
        assert kept[0][-1] == bsr.data.size and skipped[0][-1] == np.count_nonzero(bsr.data) < kept[0][-1]
        assert_same_bits(fc.chain_unfused(*kept, bb), ref, f"BSR {br}x{bc}, zeros kept")
        assert_same_bits(fc.chain_unfused(*skipped, bb), ref, f"BSR {br}x{bc}, zeros skipped")
    assert_same_bits(fc.chain_unfused(*fc.csr_rows(csr), b),
                     oracle.spmm_coo(csr.num_rows, formats.csr_to_coo(csr).row_idxs, csr.col_idxs, csr.data, b), "CSR storage order")


def test_any_order_bound_is_the_textbook_gamma():
    scale = np.array([[2.0, 0.5], [1.0, 1.0], [3.0, 0.0]])
    got = fc.any_order_bound([0, 0, 1, 15], scale)
    u = 2.0 ** -24
    assert np.array_equal(got[0], [0.0, 0.0]) and np.array_equal(got[1], u / (1 - u) * scale[1])
    assert np.array_equal(got[2], 14 * u / (1 - 14 * u) * scale[2])
    assert np.array_equal(fc.any_order_bound([0, 3], scale[:1], np.float64), 3 * 2.0 ** -53 / (1 - 3 * 2.0 ** -53) * scale[:1])


def test_corpus_is_sharp_tells_a_sharp_corpus_from_a_blunt_one(oracle):
    csr, b = ragged_host_matrix()
    assert fc.corpus_is_sharp(fc.csr_rows(csr), b)
    grid = (np.round(csr.data * 4) / 4).astype(np.float32)          # exact-grid values: nothing rounds, nothing to tell apart
    assert not fc.corpus_is_sharp((csr.row_ptrs, csr.col_idxs, grid), (np.round(b * 4) / 4).astype(np.float32))
    one = corpus.csr_from_lens(np.random.default_rng(5), 9, 20, [1, 0, 1, 1, 0, 1, 1, 1, 0])
    assert not fc.corpus_is_sharp(fc.csr_rows(one), b)              # rows of at most one entry are not allowed


CSR_CASES = corpus.all_csr_cases()


@pytest.mark.parametrize("name", [name for name, _ in CSR_CASES])
def test_every_csr_corpus_case_is_sharp(oracle, name):
    """In float32 and float64, as CSR, COO, and ELL lists (the three share the order on these matrices, which the GPU tests
    rely on), at a narrow and a wide B."""
    csr = dict(CSR_CASES)[name]
    assert csr.num_rows <= 700 and csr.num_cols <= 900
    for dtype in (np.float32, np.float64):
        for n in (3, 64):
            b = corpus.dense_b(csr.num_cols, n, dtype)
            unfused, backwards, count = fc.sharpness(fc.csr_rows(csr, dtype), b)
            print(f"{name} {np.dtype(dtype).name} N={n}: unfused differs {unfused:.2f}, reversed differs {backwards:.2f} of {count}")
            assert fc.corpus_is_sharp(fc.csr_rows(csr, dtype), b), (name, dtype, n, unfused, backwards)
    ellc = formats.csr_to_ell_colmajor(csr)
    assert all(np.array_equal(x, y) for x, y in zip(fc.ell_colmajor_rows(ellc), fc.csr_rows(csr)))
    assert all(np.array_equal(x, y) for x, y in zip(fc.coo_rows(formats.csr_to_coo(csr)), fc.csr_rows(csr)))


@pytest.mark.parametrize("shape", list(corpus.BSR_SHAPES) + ["long"])
def test_every_bsr_corpus_case_is_sharp(oracle, shape):
    bsr = corpus.bsr_long() if shape == "long" else corpus.bsr(*shape)
    assert bsr.num_rows <= 700 and bsr.num_cols <= 900
    assert 0.4 < np.count_nonzero(bsr.data) / bsr.data.size < 0.6
    b = corpus.dense_b(bsr.num_cols, 64)
    for skip in (False, True):
        assert fc.corpus_is_sharp(fc.bsr_rows(bsr, skip), b), (shape, skip, fc.sharpness(fc.bsr_rows(bsr, skip), b))
    assert fc.corpus_is_sharp(fc.bsr_rows(bsr, True, np.float64), corpus.dense_b(bsr.num_cols, 64, np.float64))


def test_every_vetted_fuzz_seed_is_sharp(oracle):
    assert len(corpus.FUZZ_CSR_SEEDS) >= 12 and len(corpus.FUZZ_BSR_SEEDS) >= 8
    for seed in corpus.FUZZ_CSR_SEEDS:
        csr, b = corpus.fuzz_csr(seed)
        assert fc.corpus_is_sharp(fc.csr_rows(csr), b), f"CSR fuzz seed {seed}: {fc.sharpness(fc.csr_rows(csr), b)}"
    for seed in corpus.FUZZ_BSR_SEEDS:
        bsr, b = corpus.fuzz_bsr(seed)
        for skip in (False, True):
            assert fc.corpus_is_sharp(fc.bsr_rows(bsr, skip), b), f"BSR fuzz seed {seed} skip_zeros={skip}"
