"""The catalogue of the mutation check of the bf16 block-sparse MFMA products: FAULTS (one sentence each, quoting between
backticks the words of include/mispmm.h or csrc/bsr_mfma_tiles.hpp that the fault breaks), HONEST variants that must pass every
check, the cases every check runs on, and `restated`: the lane-order restatement (tests/_bsr_mfma_lanes.py) of a case's kernel
with a fault put in.  OLD are the checks as they stood before this work (the 2e-6 / 2^-8 bounds against the fp32 oracle sum, the
census's integer kind and its sentinel check, on those tests' operands), NEW the four of tests/_bsr_mfma_tight.py."""
import functools

import numpy as np

import _bsr_mfma_lanes as lanes
import _bsr_mfma_tight as tight
from _bsr_mfma_tight import Case
from mispmm import formats

DENSE, COMPACT, WAVES4, ALL = ("bsr16", "bsr32"), ("bsrc", "slots"), ("bsr16", "bsr32", "slots"), ("bsr16", "bsr32", "bsrc", "slots")

# fault -> (the kernels it can be put into, the sentence)
_F = {
    "missing_half_reads_block_0": (("bsr16",), "the left-over half of an odd pair reads the B rows of block 0 under its zero coefficients -- `the missing half of an odd block pair`"),
    "missing_half_reads_next_block_row": (("bsr16",), "the left-over half of an odd pair takes the next block row's first block -- `a block past the row's end, a padding column 0xFFFFFFFF`"),
    "last_odd_block_dropped": (DENSE, "the last block of an odd count is never multiplied -- `multiplies every stored element of a block`"),
    "blocks_past_first_round_dropped": (DENSE, "a wave stops after its first pair or block -- `deals block pairs (16 x 16) or blocks (32 x 32) round-robin over 4 waves`"),
    "wave_partial_lost": (WAVES4, "the partial tile of wave 2 is not added -- `The others add 3 partial tiles`"),
    "wave_partial_added_twice": (WAVES4, "the partial tile of wave 2 is added twice -- `The 4 partial tiles are added in wave order`"),
    "reduce_through_bf16": (WAVES4, "the partial tiles pass through LDS as bf16 -- `the fp32 sum rounded once`"),
    "regroup_even_odd_swapped": (ALL, "regroup_pair hands tile 2w the high half of dword w -- `the low and high bf16 of dword w of every k row`"),
    "regroup_k_rows_swapped": (ALL, "regroup_pair packs k rows 2p + 1, 2p in that order -- `B[k = 8g .. 8g+7][j = c]`"),
    "a_k_slots_reversed": (ALL, "a lane's 8 coefficients meet its 8 B rows in reverse -- `lane (c, g) holds A[i = c][k = 8g .. 8g+7]`"),
    "b32_second_half_takes_first_a": (("bsr32",), "rows 16..31 of a 32 x 32 block are multiplied with the first half's coefficients -- `two for the 16-row halves of a 32 x 32 block`"),
    "row_4r_plus_g": (ALL, "register r of lane group g is stored as row 4r + g -- `register r of a result tile is D[row 4g + r][col c]`"),
    "ncol_without_interleave": (ALL, "tile t is stored at column 16t + c of the super-tile -- `ncol = 16 * TPL * st + TPL * c`"),
    "lane_past_n_not_dropped": (ALL, "a lane whose columns lie past N reads B all the same -- `kDropLoad for ncol >= N`"),
    "padding_reads_column_0": (COMPACT, "a padding slot reads B row 0 under its zero coefficients -- `No product reads a B row for a padding column`"),
    "padding_reads_column_k_minus_1": (COMPACT, "a padding slot reads B row K - 1 under its zero coefficients -- `takes kDropLoad as the WHOLE offset`"),
    "unoccupied_column_kept": (COMPACT, "the helper lists every column of a stored block -- `never read a B row for any other column`"),
    "unused_slot_runs_previous_row": (("slots",), "a slot past the row's step count multiplies the previous block row's step -- `slots past the row's step count hold a padding column list`"),
    "extra_steps_start_one_late": (("slots",), "the extra steps start at extraPtrs[R] + 1 -- `follow the slots at index 4 * numBlockRows + extraPtrs[R] .. extraPtrs[R + 1]`"),
    "extra_steps_end_one_early": (("slots",), "the extra steps end one before extraPtrs[R + 1] -- `block rows with more than 128 occupied columns`"),
    "extra_ptrs_read_without_extra_steps": (("slots",), "the shared-reduce kernel walks extraPtrs -- `extraPtrs must then be all zeros (as the helper writes it) and is not read`"),
    "shared_reduce_rows_of_wrong_wave": (("slots",), "wave q stores its four rows where wave q + 1's belong -- `each of the 4 waves adds and stores 4 of the block row's 16 rows`"),
    "empty_block_row_unwritten": (ALL, "a block row without blocks leaves C as it was -- `An empty block row is written as +0`"),
    "product_rounded_to_bf16": (ALL, "every product is rounded to bf16 before it is added -- `The product of two bf16 values is exact in fp32`"),
    "b_low_mantissa_bit_cleared": (ALL, "B loses the last bit of its mantissa on the way to the operand -- `the lane's TPL interleaved bf16 columns`"),
    "a_low_mantissa_bit_cleared": (ALL, "A loses the last bit of its mantissa on the way to the operand -- `one 16-byte read`"),
    "bf16_c_truncated": (ALL, "a bf16 C is cut off, not rounded -- `rounded to bf16 (nearest even) at both ends`"),
    "bf16_c_from_bf16_partial": (WAVES4, "for a bf16 C the partial tiles are rounded to bf16 before they are added -- `the fp32 sum rounded once, a NaN stays a NaN`"),
    "pack_bf2_halves_swapped": (ALL, "pack_bf2 puts its first argument in the high half -- `in the low half`"),
    "ldc_for_ldb": (ALL, "a B row is found with C's leading dimension -- `B is read through a buffer descriptor of its exact size`"),
}
FAULTS = {name: sentence for name, (_, sentence) in _F.items()}
assert set(FAULTS) == set(lanes.FAULTS)

# what no check of C can see, and why
UNSEEN = {
    "lane_past_n_not_dropped": "a lane's B rows feed only its own TPL output columns, which lie past N and are never stored: the reads cost "
                               "traffic (and past the buffer return zeros) but no element of C depends on them",
    "extra_ptrs_read_without_extra_steps": "without extra steps the call's precondition makes extraPtrs all zeros, so walking it runs nothing; an "
                                           "array that showed the read would break that precondition",
}

# honest variants: name -> the kernels it changes
HONEST = {"reduce_other_wave_order": WAVES4, "tpl_4_for_8": DENSE, "block_columns_permuted": ALL}

NEW = ("tight", "sharp_exact", "specials", "untouched")
OLD = ("old_bound", "old_ints", "old_sentinel")
CHECKS = {"old_bound": tight.old_bound, "old_ints": tight.old_ints, "old_sentinel": tight.old_sentinel, "tight": tight.tight,
          "sharp_exact": tight.sharp_exact, "specials": tight.specials, "untouched": tight.untouched}


def family_of(fault):
    return _F[fault][0] if fault in _F else HONEST.get(fault, ALL)


# ------------------------------------------------------------------------------------------------ the cases
# (N, ldb, ldc): one width per tag of the census table (T4: N = 4, T8: N = 128; the compacted kernels at their smallest legal
# N = 8) and a partial last super-tile, N = 72 (T4) and 136 (T8), with ldb and ldc larger than N and different from each other
WIDTHS = {"bsr16": ((4, 4, 4), (72, 80, 88), (128, 128, 128), (136, 144, 152)),
          "bsr32": ((4, 4, 4), (72, 80, 88), (128, 128, 128), (136, 144, 152)),
          "bsrc": ((8, 8, 8), (136, 144, 152)), "slots": ((8, 8, 8), (136, 144, 152))}
PATTERNS_OF = {"bsr16": ("p16",), "bsr32": ("p32",), "bsrc": ("c16", "c8"), "slots": ("c16", "c8", "c16s", "c8s")}
KIND_OF = {"tight": "tight", "untouched": "tight", "sharp_exact": "sharp", "specials": "specials"}


def new_cases(kernel, kind):
    return [Case(kernel, p, kind, n, ldb, ldc, c16) for p in PATTERNS_OF[kernel] for n, ldb, ldc in WIDTHS[kernel] for c16 in (False, True)]


def old_cases(kernel, kind):
    """run_bf16's rows of the census table (C with a gap of 8, B contiguous) and, for the slots kernel's bound, the ragged case."""
    import _census as census
    family = {"bsr16": "bsr_mfma_bf16", "bsr32": "bsr_mfma_bf16_b32", "bsrc": "bsrc_mfma_bf16", "slots": "bsrc_slots_mfma_bf16"}[kernel]
    out = [Case(kernel, "old:" + row.key, kind, row.spec["n"], row.spec["n"], row.spec["n"] + 8, row.spec["out_bf16"]) for row in census.FAMILIES[family]]
    if kernel == "slots" and kind == "full":
        out.append(Case("slots", "old:ragged", "full", 136, 144, 144, False))
    return out


def cases_of(check, kernel):
    if check == "old_bound":
        return old_cases(kernel, "full")
    if check == "old_ints":
        return old_cases(kernel, "ints")
    if check == "old_sentinel":
        return old_cases(kernel, "full") + old_cases(kernel, "ints")
    return new_cases(kernel, KIND_OF[check])


def shares(case, bsr):
    """The instance mispmm_bsrc_slots_bf16 takes by default: the shared reduce without extra steps and with an fp32 C."""
    return case.kernel == "slots" and not case.out_bf16 and all(len(lanes.occupied(bsr, r)) <= 128 for r in range(bsr.num_rows // 16))


def _permuted(bsr):
    rng = np.random.default_rng(5)
    ptrs = np.asarray(bsr.block_row_ptrs, np.int64)
    perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in zip(ptrs[:-1], ptrs[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
    data = np.asarray(bsr.data).reshape(bsr.num_blocks, bsr.block_row_size, bsr.block_col_size)[perm]
    return formats.BSR(bsr.num_rows, bsr.num_cols, bsr.nnz, bsr.block_row_size, bsr.block_col_size, bsr.block_row_ptrs,
                       np.asarray(bsr.block_col_idxs)[perm], data)


@functools.lru_cache(maxsize=4096)
def restated(case, fault=None):
    """The flat C buffer (tight.c_view) of the case's kernel restated in lane order, with `fault` (a fault or an honest variant)."""
    bsr = tight.operands(case)["bsr"]
    kw = {}
    if fault in HONEST:
        if fault == "reduce_other_wave_order" and case.kernel != "bsrc":
            kw["order"] = (2, 0, 3, 1)
        if fault == "tpl_4_for_8" and case.kernel in DENSE:
            kw["tpl"] = 4
        if fault == "block_columns_permuted":
            bsr = _permuted(bsr)
        fault = None
    elif fault is not None and fault not in FAULTS:
        raise ValueError(f"unknown fault {fault!r}")
    tail = dict(sentinel=tight.SENTINEL, tail=tight.TAIL)
    args = (tight.b_flat(case), bsr.num_cols, case.n, case.ldb, case.ldc, case.out_bf16)
    with np.errstate(all="ignore"):
        if case.kernel in DENSE:
            fn = lanes.bsr16 if case.kernel == "bsr16" else lanes.bsr32
            return fn(bsr.block_row_ptrs, bsr.block_col_idxs, bsr.data, *args, fault=fault, **kw, **tail)
        if case.kernel == "bsrc":
            return lanes.bsrc(*lanes.compact(bsr, fault), *args, fault=fault, **tail)
        extra, cols, tiles = lanes.compact_slots(bsr, fault)
        share = not case.out_bf16 and cols.shape[0] == lanes.SLOTS * (extra.shape[0] - 1)          # what the entry point decides by
        return lanes.slots(extra, cols, tiles, *args, share, fault=fault, **kw, **tail)
