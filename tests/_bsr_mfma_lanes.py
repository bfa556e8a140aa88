"""The five bf16 block-sparse MFMA products restated in numpy, in the order of their lanes (csrc/bsr_mfma_tiles.hpp, spmm_bsr.hip,
bsr_slots.hpp, bsr_bf16_lds.hpp), each taking `fault=None`: a named one-line departure from the kernel as written
(tests/_bsr_mfma_mutants.py holds the catalogue; an unknown name raises ValueError).

Restated as written: lane l = (c = l & 15, g = l >> 4) holds A[i = c][k = 8g .. 8g+7] and B[k = 8g .. 8g+7][j = c]; which B rows
the 32 k slots are (the 16 + 16 columns of a block pair, the 32 columns of one 32 x 32 block under two A halves, 32 occupied
columns of a step); the column interleave ncol = 16 * TPL * st + TPL * c with tile t at column ncol + t; dropped loads (a lane
past N, a B row that is not there, an offset past the buffer) returning zeros; regroup_pair; the round-robin of pairs / blocks
/ slots over the 4 waves; the extra steps behind the slots; the reduce in wave order, the shared form included; store_crow's
row 4g + r; pack_bf2.  B and C are FLAT buffers with their leading dimensions, as the kernels see them.

NOT restated: the order inside one MFMA, which is the hardware's.  A step's 32 products are summed in float64 and rounded to
fp32 once per step (added to the accumulator first where the kernel hands the MFMA an addend).  So this file is for families
with an exact answer and for comparisons within a tolerance, never for bits on operands that make the fp32 sums round.

Values travel as float64 arrays holding fp32 (or bf16) numbers; a bf16 C is returned widened, in a float32 buffer."""
import numpy as np

PAD = 0xFFFFFFFF
DROP = -1
SLOTS = 4

FAULTS = (
    "missing_half_reads_block_0", "missing_half_reads_next_block_row", "last_odd_block_dropped", "blocks_past_first_round_dropped",
    "wave_partial_lost", "wave_partial_added_twice", "reduce_through_bf16", "regroup_even_odd_swapped", "regroup_k_rows_swapped",
    "a_k_slots_reversed", "b32_second_half_takes_first_a", "row_4r_plus_g", "ncol_without_interleave", "lane_past_n_not_dropped",
    "padding_reads_column_0", "padding_reads_column_k_minus_1", "unoccupied_column_kept", "unused_slot_runs_previous_row",
    "extra_steps_start_one_late", "extra_steps_end_one_early", "extra_ptrs_read_without_extra_steps", "shared_reduce_rows_of_wrong_wave",
    "empty_block_row_unwritten", "product_rounded_to_bf16", "b_low_mantissa_bit_cleared", "bf16_c_truncated", "bf16_c_from_bf16_partial",
    "pack_bf2_halves_swapped", "ldc_for_ldb", "a_low_mantissa_bit_cleared",
)


def _known(fault):
    if fault is not None and fault not in FAULTS:
        raise ValueError(f"unknown fault {fault!r}")


def f32(x):
    """Round float64 values to fp32 (nearest even), kept in float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def bf16_rne(x, truncate=False):
    """fp32 values -> the bf16 number v_cvt_pk_bf16_f32 gives (nearest even; a NaN stays a NaN), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    with np.errstate(over="ignore"):
        r = (u if truncate else u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    r = np.where(nan, (u | np.uint32(0x00400000)) & np.uint32(0xFFFF0000), r)
    return r.view(np.float32)


def _clear_low_bit(v):
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFEFFFF)
    return u.view(np.float32).astype(np.float64)


def pick_tpl(n, ldb, ldc):
    """mispmm_bsr_bf16's choice: 8 tiles per lane once N fills 128 columns in whole 16-byte vectors, else 4."""
    return 8 if n >= 128 and n % 8 == 0 and ldb % 8 == 0 and ldc % 8 == 0 else 4


class _Item:
    """What the kernels share of one work item (block row R, super-tile st): the B-row read, the MFMA step, the C-row store."""

    def __init__(self, bflat, k, n, ldb, cbuf, ldc, out_bf16, tpl, st, fault):
        self.b, self.k, self.n, self.ldb, self.c, self.ldc = bflat, k, n, ldb, cbuf, ldc
        self.out_bf16, self.tpl, self.st, self.fault = out_bf16, tpl, st, fault
        self.ncol = 16 * tpl * st + tpl * np.arange(16)             # first of lane column c's TPL interleaved columns
        self.live = self.ncol < n
        self.zero = np.zeros((16, 16, tpl))                         # a tile: [row i][lane column c][tile t]

    def b_operand(self, brow):
        """brow[g][e]: the B row of k slot 8g + e, or DROP -> B[g][e][c][t], what regroup_pair hands tile t of lane (c, g)."""
        fault, tpl = self.fault, self.tpl
        ld = self.ldc if fault == "ldc_for_ldb" else self.ldb
        off = brow[:, :, None, None].astype(np.int64) * ld + self.ncol[None, None, :, None] + np.arange(tpl)[None, None, None, :]
        keep = (brow != DROP)[:, :, None, None] & (off < self.b.shape[0])         # the buffer descriptor holds B's exact size
        if fault != "lane_past_n_not_dropped":
            keep = keep & self.live[None, None, :, None]
        v = np.where(keep, self.b[np.where(keep, off, 0)], 0.0).astype(np.float64)
        if fault == "b_low_mantissa_bit_cleared":
            v = _clear_low_bit(v)
        if fault == "regroup_even_odd_swapped":                     # tile 2w takes the high half of dword w
            v = v[..., np.arange(tpl) ^ 1]
        if fault == "regroup_k_rows_swapped":                       # {lo.h0, hi.h0}: k rows 2p and 2p + 1 change places
            v = v[:, np.arange(8) ^ 1]
        return v

    def mfma(self, a_op, brow, acc):
        """One v_mfma_f32_16x16x32_bf16: a_op[i][g][e] = A[i][k = 8g + e]; 32 products in float64, one rounding with the addend."""
        if self.fault == "a_k_slots_reversed":
            a_op = a_op[:, :, ::-1]
        if self.fault == "a_low_mantissa_bit_cleared":
            a_op = _clear_low_bit(a_op)
        with np.errstate(invalid="ignore", over="ignore"):
            p = a_op[:, :, :, None, None] * self.b_operand(brow)[None]
            if self.fault == "product_rounded_to_bf16":
                p = bf16_rne(p.astype(np.float32)).astype(np.float64)
            return f32(acc + p.sum(axis=(1, 2)))

    def park(self, tile):
        """A partial tile on its way through LDS: fp32 as it is."""
        if self.fault == "reduce_through_bf16" or (self.fault == "bf16_c_from_bf16_partial" and self.out_bf16):
            return bf16_rne(tile.astype(np.float32)).astype(np.float64)
        return tile

    def store(self, row0, tile, rows=None):
        """store_crow: register r of lane (c, g) is row 4g + r of the tile, its TPL tiles the columns ncol .. ncol + TPL - 1."""
        fault, tpl = self.fault, self.tpl
        i = np.arange(16)
        dst_row = 4 * (i % 4) + i // 4 if fault == "row_4r_plus_g" else i
        if fault == "ncol_without_interleave":
            cols = 16 * tpl * self.st + 16 * np.arange(tpl)[None, :] + np.arange(16)[:, None]
        else:
            cols = self.ncol[:, None] + np.arange(tpl)[None, :]
        ok = self.live[:, None] & (cols < self.n)
        vals = tile.astype(np.float32)
        if self.out_bf16:
            if fault == "pack_bf2_halves_swapped":
                vals = vals[..., np.arange(tpl) ^ 1]
            vals = bf16_rne(vals, truncate=fault == "bf16_c_truncated")
        c2 = self.c[:(self.c.shape[0] // self.ldc) * self.ldc].reshape(-1, self.ldc)
        for src in (range(16) if rows is None else rows):
            c2[row0 + dst_row[src], cols[ok]] = vals[src][ok]


def _reduce(item, tiles, order, fault, lost=2):
    """Wave 0 adds the parked tiles of waves 1..3 to its own, in wave order (`order`: an honest variant takes another)."""
    total = None
    for w in order:
        if fault == "wave_partial_lost" and w == lost:
            continue
        t = tiles[w] if w == order[0] else item.park(tiles[w])
        total = t if total is None else f32(total + t)
        if fault == "wave_partial_added_twice" and w == lost:
            total = f32(total + t)
    return total


def _new_c(m, ldc, sentinel, tail):
    return np.full(m * ldc + tail, sentinel, dtype=np.float32)


def bsr16(ptrs, idxs, blocks, bflat, k, n, ldb, ldc, out_bf16, fault=None, tpl=None, order=(0, 1, 2, 3), sentinel=-7.0, tail=64):
    """bsr_mfma_bf16: one workgroup per (block row, super-tile); pair p -> wave p % 4; k slots 0..15 the columns of the pair's
    first block, 16..31 those of its second (zeros when an odd block is left over)."""
    _known(fault)
    ptrs, idxs = np.asarray(ptrs, np.int64), np.asarray(idxs, np.int64)
    blocks = np.asarray(blocks, np.float64).reshape(-1, 16, 16)
    tpl = tpl or pick_tpl(n, ldb, ldc)
    mb = ptrs.shape[0] - 1
    c = _new_c(mb * 16, ldc, sentinel, tail)
    for r in range(mb):
        bs, be = int(ptrs[r]), int(ptrs[r + 1])
        if fault == "empty_block_row_unwritten" and bs == be:
            continue
        npairs = (be - bs + 1) // 2
        for st in range(-(-n // (16 * tpl))):
            it = _Item(bflat, k, n, ldb, c, ldc, out_bf16, tpl, st, fault)
            tiles = []
            for w in range(4):
                acc = it.zero
                for pair in range(w, npairs, 4):
                    if fault == "blocks_past_first_round_dropped" and pair >= 4:
                        break
                    a_op, brow = np.zeros((16, 4, 8)), np.full((4, 8), DROP, np.int64)
                    for g in range(4):
                        b, khalf = bs + 2 * pair + (g >> 1), (g & 1) * 8
                        have = b < be
                        if fault == "last_odd_block_dropped" and (be - bs) % 2 == 1 and b == be - 1:
                            have = False
                        if have or (fault == "missing_half_reads_next_block_row" and b < blocks.shape[0]):
                            a_op[:, g, :] = blocks[b][:, khalf:khalf + 8]
                            brow[g] = idxs[b] * 16 + khalf + np.arange(8)
                        elif fault == "missing_half_reads_block_0" and b == be:
                            brow[g] = idxs[0] * 16 + khalf + np.arange(8)       # the coefficients are zero; the B rows are read
                    acc = it.mfma(a_op, brow, acc)
                tiles.append(acc)
            it.store(r * 16, _reduce(it, tiles, order, fault))
    return c


def bsr32(ptrs, idxs, blocks, bflat, k, n, ldb, ldc, out_bf16, fault=None, tpl=None, order=(0, 1, 2, 3), sentinel=-7.0, tail=64):
    """bsr_mfma_bf16_b32: block b -> wave b % 4; a block's 32 columns are one MFMA's K, its rows two 16-row halves that share
    the B fragment."""
    _known(fault)
    ptrs, idxs = np.asarray(ptrs, np.int64), np.asarray(idxs, np.int64)
    blocks = np.asarray(blocks, np.float64).reshape(-1, 32, 32)
    tpl = tpl or pick_tpl(n, ldb, ldc)
    mb = ptrs.shape[0] - 1
    c = _new_c(mb * 32, ldc, sentinel, tail)
    for r in range(mb):
        bs, be = int(ptrs[r]), int(ptrs[r + 1])
        if fault == "empty_block_row_unwritten" and bs == be:
            continue
        for st in range(-(-n // (16 * tpl))):
            it = _Item(bflat, k, n, ldb, c, ldc, out_bf16, tpl, st, fault)
            tiles = [[], []]
            for w in range(4):
                acc = [it.zero, it.zero]
                for b in range(bs + w, be, 4):
                    if fault == "blocks_past_first_round_dropped" and b >= bs + 4:
                        break
                    if fault == "last_odd_block_dropped" and (be - bs) % 2 == 1 and b == be - 1:
                        continue
                    brow = idxs[b] * 32 + np.arange(32).reshape(4, 8)
                    for h in range(2):
                        half = 0 if fault == "b32_second_half_takes_first_a" else h
                        acc[h] = it.mfma(blocks[b][16 * half:16 * half + 16].reshape(16, 4, 8), brow, acc[h])
                for h in range(2):
                    tiles[h].append(acc[h])
            for h in range(2):
                it.store(r * 32 + 16 * h, _reduce(it, tiles[h], order, fault))
    return c


# ---- the column-compacted layouts: mispmm_bsr_compact_bf16_host / mispmm_bsr_compact_slots_bf16_host in numpy
def occupied(bsr, r, fault=None):
    """[(B row, the 16 coefficients)] of block row r's occupied columns -- a value still non-zero as bf16 -- in storage order."""
    bc = bsr.block_col_size
    data = bf16_rne(np.asarray(bsr.data, np.float32).reshape(-1, 16, bc)).astype(np.float64)
    out = []
    for b in range(int(bsr.block_row_ptrs[r]), int(bsr.block_row_ptrs[r + 1])):
        for j in range(bc):
            if np.any(data[b][:, j] != 0) or fault == "unoccupied_column_kept":
                out.append((int(bsr.block_col_idxs[b]) * bc + j, data[b][:, j]))
    return out


def _fill(occ, s):
    cols, tile = np.full(32, PAD, np.int64), np.zeros((16, 32))
    for kk, (col, vals) in enumerate(occ[32 * s:32 * s + 32]):
        cols[kk], tile[:, kk] = col, vals
    return cols, tile


def compact(bsr, fault=None):
    """(stepPtrs, cols [nSteps, 32], tiles [nSteps, 16, 32]): 32 occupied columns per step, 0xFFFFFFFF padding trails."""
    ptrs, cols, tiles = [0], [], []
    for r in range(bsr.num_rows // 16):
        occ = occupied(bsr, r, fault)
        for s in range(-(-len(occ) // 32)):
            cl, tl = _fill(occ, s)
            cols.append(cl)
            tiles.append(tl)
        ptrs.append(len(cols))
    return np.array(ptrs, np.int64), np.array(cols, np.int64).reshape(-1, 32), np.array(tiles).reshape(-1, 16, 32)


def compact_slots(bsr, fault=None):
    """(extraPtrs, cols, tiles): step R * 4 + w in the fixed slots (all padding past the row's count), the steps past the
    fourth behind them."""
    mb = bsr.num_rows // 16
    fixed, extra, ptrs = [None] * (mb * SLOTS), [], [0]
    for r in range(mb):
        occ = occupied(bsr, r, fault)
        for s in range(max(-(-len(occ) // 32), SLOTS)):
            if s < SLOTS:
                fixed[r * SLOTS + s] = _fill(occ, s)
            else:
                extra.append(_fill(occ, s))
        ptrs.append(len(extra))
    steps = fixed + extra
    return np.array(ptrs, np.int64), np.array([s[0] for s in steps], np.int64), np.array([s[1] for s in steps])


def _padding(cols, k, fault):
    """B rows of a step's 32 column indices as [g][e]: padding takes kDropLoad as the whole offset."""
    pad = 0 if fault == "padding_reads_column_0" else k - 1 if fault == "padding_reads_column_k_minus_1" else DROP
    return np.where(cols == PAD, pad, cols).reshape(4, 8)


def bsrc(step_ptrs, cols, tiles, bflat, k, n, ldb, ldc, out_bf16, fault=None, sentinel=-7.0, tail=64):
    """bsrc_mfma_bf16: one WAVE per (block row, 128 columns), its steps in ascending order into one accumulator."""
    _known(fault)
    mb = step_ptrs.shape[0] - 1
    c = _new_c(mb * 16, ldc, sentinel, tail)
    for r in range(mb):
        s0, s1 = int(step_ptrs[r]), int(step_ptrs[r + 1])
        if fault == "empty_block_row_unwritten" and s0 == s1:
            continue
        for st in range(-(-n // 128)):
            it = _Item(bflat, k, n, ldb, c, ldc, out_bf16, 8, st, fault)
            acc = it.zero
            for s in range(s0, s1):
                acc = it.mfma(tiles[s].reshape(16, 4, 8), _padding(cols[s], k, fault), acc)
            it.store(r * 16, acc)
    return c


def slots(extra_ptrs, cols, tiles, bflat, k, n, ldb, ldc, out_bf16, share, fault=None, order=(0, 1, 2, 3), sentinel=-7.0, tail=64):
    """bsrc_slots_mfma_bf16: wave w multiplies slot R * 4 + w into FRESH accumulators (zeros for an unused slot); extra step i
    goes to wave 1 + i % 3, which adds it into its parked tile; the four tiles are added in wave order -- by wave 0 for all 16
    rows, or with `share` by wave q for rows 4q .. 4q+3 (never taken with extra steps, and extraPtrs is then not used)."""
    _known(fault)
    mb = extra_ptrs.shape[0] - 1
    nsteps = cols.shape[0]
    assert not share or nsteps == mb * SLOTS
    c = _new_c(mb * 16, ldc, sentinel, tail)
    for r in range(mb):
        used = [bool(cols[r * SLOTS + w][0] != PAD) for w in range(SLOTS)]
        if fault == "empty_block_row_unwritten" and not any(used):
            continue
        for st in range(-(-n // 128)):
            it = _Item(bflat, k, n, ldb, c, ldc, out_bf16, 8, st, fault)

            def step(s):
                return it.mfma(tiles[s].reshape(16, 4, 8), _padding(cols[s], k, fault), it.zero)

            wave = []
            for w in range(SLOTS):
                if used[w]:
                    wave.append(step(r * SLOTS + w))
                elif fault == "unused_slot_runs_previous_row" and r > 0:
                    wave.append(step((r - 1) * SLOTS + w))
                else:
                    wave.append(it.zero)
            if not share or fault == "extra_ptrs_read_without_extra_steps":
                ex0, ex1 = int(extra_ptrs[r]), int(extra_ptrs[r + 1])
                if fault == "extra_steps_start_one_late":
                    ex0 = min(ex0 + 1, ex1)
                if fault == "extra_steps_end_one_early":
                    ex1 = max(ex1 - 1, ex0)
                for w in range(1, SLOTS):
                    for e in range(ex0 + w - 1, ex1, SLOTS - 1):
                        wave[w] = f32(it.park(wave[w]) + step((mb * SLOTS + e) % nsteps))     # past the extent: some other step
            if share:
                for q in range(SLOTS):                              # wave q owns rows 4q .. 4q+3: lane group q of every wave
                    total = None
                    for w in order:
                        if fault == "wave_partial_lost" and w == 2:
                            continue
                        t = wave[w] if w == q else it.park(wave[w])
                        total = t if total is None else f32(total + t)
                        if fault == "wave_partial_added_twice" and w == 2:
                            total = f32(total + t)
                    owner = (q + 1) % SLOTS if fault == "shared_reduce_rows_of_wrong_wave" else q
                    moved = np.zeros_like(total)
                    moved[4 * owner:4 * owner + 4] = total[4 * q:4 * q + 4]
                    it.store(r * 16, moved, rows=range(4 * owner, 4 * owner + 4))
            else:
                it.store(r * 16, _reduce(it, wave, order, fault))
    return c


def lds(ptrs, idxs, blocks, bflat, k, n, ldb, ldc, out_bf16, sentinel=-7.0, tail=64):
    """bsr_bf16_lds: two waves split the 64 columns of a super-tile, both walk the block row's pairs in ascending order into
    one accumulator: no partial tiles, no reduce.  (Restated for its exact answers only: takes no fault.)"""
    ptrs, idxs = np.asarray(ptrs, np.int64), np.asarray(idxs, np.int64)
    blocks = np.asarray(blocks, np.float64).reshape(-1, 16, 16)
    mb = ptrs.shape[0] - 1
    c = _new_c(mb * 16, ldc, sentinel, tail)
    for r in range(mb):
        bs, be = int(ptrs[r]), int(ptrs[r + 1])
        for st in range(-(-n // 64)):
            it = _Item(bflat, k, n, ldb, c, ldc, out_bf16, 4, st, None)
            acc = it.zero
            for pair in range((be - bs + 1) // 2):
                a_op, brow = np.zeros((16, 4, 8)), np.full((4, 8), DROP, np.int64)
                for g in range(4):
                    b, khalf = bs + 2 * pair + (g >> 1), (g & 1) * 8
                    if b < be:
                        a_op[:, g, :] = blocks[b][:, khalf:khalf + 8]
                        brow[g] = idxs[b] * 16 + khalf + np.arange(8)
                acc = it.mfma(a_op, brow, acc)
            it.store(r * 16, acc)
    return c
