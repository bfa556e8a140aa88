"""The census of kernel instances: for every kernel family (a `note_kernel` call site of csrc/) the instance keys the
production library can emit, each with the smallest operands that reach it; the keys it cannot emit, with the reason; and
how many instances of every kernel template the built library holds.  tests/test_gpu_census.py runs every row on the GPU
against the project's reference for the operation and checks the key; tests/test_census_cpu.py checks the tables themselves.

The key of a launch is capi.last_kernel() without what depends on the size of the call (`normalise`): the text up to the
closing `>` of the instance, ` batched` and ` plan-order` where present; for csr_hybrid the accumulate mode and the lane group
of its row-gather half.  The `xcd PxQ` figures and the span, row, tile, panel and workgroup counts are dropped.

Rows are derived by reading the dispatcher of each family (the function named next to each table) and were confirmed on an
MI355X by letting the sweep print what it met.  Smallest means: M of a few workgroups with the last one partly filled, K of
at most a few hundred, the smallest N of the dispatch class, row lengths on both sides of the kernel's batch of 8 slots.

Template parameters the tag does not show, and which the census therefore cannot tell apart:
  * row_gather_kernel SC1: C through buffer stores, or plain global stores for a C of 2 GiB or more
    (tests/test_gpu_spmm.py::test_wide_address_fallbacks_for_b_beyond_2gib runs the plain form);
  * bsr_valu WIDE: 64-bit addresses for a B of 2 GiB or more (the same test);
  * bsr_mfma_bf16 PIPE: the register double buffer of the 128-column form, taken only with MISPMM_BSR_PIPE=1 in the tuning
    build;
  * csr_lds_tile_kernel WW: the slot count 8 / 12 / 14 / 16 picked from the row width (the census runs one width per
    accumulate mode; tests/test_gpu_spmm.py::test_csr_lds_tiles_match_oracle walks the widths);
  * the span-list flavour of csr_split (`,longest-first`) is an argument, not an instance: both are kept in the key because
    the kernel reads its rows differently.
`sddmm_csr<zero>` and `sddmm_bsr<zero>` name a memset, not a kernel, and have no row."""
import fnmatch
import functools
import itertools
import re
from collections import namedtuple

import numpy as np

from mispmm import formats

import _fma_chain as fc
import _softmax_ref

Row = namedtuple("Row", "key spec")          # spec: the arguments of the family's builder, a dict
Excluded = namedtuple("Excluded", "pattern why detail")   # pattern: fnmatch over keys; why: one of REASONS

REASONS = ("2gib", "knob", "unreachable")
#   2gib        : reachable only with an operand of 2 GiB or more; `detail` names the existing test that runs it
#   knob        : reachable only through a MISPMM_* knob of the tuning build (-DMISPMM_TUNING); production never launches it
#   unreachable : the instance exists but no production call reaches it; `detail` names the branch that would have to change

WIDE_TEST = "tests/test_gpu_spmm.py::test_wide_address_fallbacks_for_b_beyond_2gib"
F64_WIDE_TEST = "tests/test_gpu_f64.py::test_b_beyond_2gib_takes_the_64_bit_body"
LINE_TEST = ("no GPU test runs it (a known gap: it needs a C or an A of 2 GiB); the rule alone is pinned by "
             "tests/test_uniform_line_cpu.py::test_fallback_rule_keeps_large_arrays_on_the_rolling_body")


# ------------------------------------------------------------------------------------------------ the key
_HYBRID = re.compile(r"^csr_hybrid<(\w+),R(\d+)> split .* \+ row_gather<G(\d+),spans>")
_XCD = re.compile(r" xcd (\d+)x(\d+)")


def normalise(tag):
    """capi.last_kernel() -> instance key."""
    m = _HYBRID.match(tag)
    if m:
        return f"csr_hybrid<{m.group(1)},R{m.group(2)}>+row_gather<G{m.group(3)},spans>"
    close = tag.find(">")
    head, tail = (tag[:close + 1], tag[close + 1:]) if close >= 0 else (tag.split(" ")[0], tag[len(tag.split(" ")[0]):])
    key = head
    for word in (" batched", " plan-order"):
        if word in tail:
            key += word
    return key


def xcd_of(tag):
    """(P, Q) of the first `xcd PxQ` of a tag, or None."""
    m = _XCD.search(tag)
    return (int(m.group(1)), int(m.group(2))) if m else None


_KEY = re.compile(r"^[a-z0-9_]+(<[A-Za-z0-9_,\-]+>)?(\+row_gather<G\d+,spans>)?( batched)?( plan-order)?$")


def parses(key):
    return bool(_KEY.match(key)) and normalise(key.replace("+row_gather", " split 0 spans xcd 1x1 + row_gather")
                                                 if key.startswith("csr_hybrid") else key) == key


# ------------------------------------------------------------------------------------------------ instantiation counts
# __device_stub__ symbols per kernel template in libmispmm.so (`nm -C`, counted by template name only; an instantiation two
# translation units share counts once).  A pull request that adds or removes an instantiation changes a figure here and has
# to decide whether the new instances are reachable: a row in a table below, or an entry in EXCLUSIONS.
INSTANCES = {
    "row_gather_kernel": 392, "row_line_kernel": 96, "sddmm_csr_kernel": 56, "coo_k1": 48, "bsr_valu": 48, "csr_f64_kernel": 32,
    "ell_wide": 24, "csr_wide": 24, "csr_k2": 24, "csr_k1": 24, "bsr_rowblock": 24, "softmax_csr_kernel": 20,
    "softmax_csr_bwd_kernel": 20, "sddmm_bsr_kernel": 20, "bsrc_slots_mfma_bf16": 16, "csr_k3": 12, "softmax_bsr_kernel": 8,
    "softmax_bsr_bwd_kernel": 8, "csr_lds_tile_kernel": 8, "csr_wave_deep": 6, "csr_hybrid": 6, "bsr_mfma_bf16": 6,
    "csr_panel_kernel": 4, "bsr_mfma_bf16_b32": 4, "csr_split": 3, "bsrc_mfma_bf16": 2, "bsr_bf16_lds": 2, "transpose_f32": 1,
    "slab_scatter_kernel": 1, "f32_to_bf16_kernel": 1, "coo_row_bounds": 1, "bsr_mfma_f32": 1, "bf16_to_f32_kernel": 1,
}


# ------------------------------------------------------------------------------------------------ host operands
M_ROWS, K_COLS = 150, 200            # 150 rows: 10 workgroups of 16 lane groups, the last partly filled; 19 of 8


def csr_from_lens(m, k, lens, seed):
    """Rows of the given lengths, columns ascending and distinct inside a row, values with full mantissas (_fma_chain)."""
    rng = np.random.default_rng(seed)
    lens = np.minimum(np.asarray(lens, dtype=np.int64), k)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cols = np.concatenate([np.sort(rng.choice(k, size=int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)])
    return formats.CSR(m, k, ptr, cols.astype(np.uint32), fc.sharp_values(rng, int(ptr[-1]), np.float32))


def row_lengths(shape, m=M_ROWS, seed=0):
    """short: 0..19 entries, either side of the batch of 8 and of 16, empty rows first, last and inside (mean below 24).
    long: 20..70 entries with two rows past the 128-entry share length (mean of 24 or more).
    tail: short rows with a few of 64 entries and more (mean below 24: the two-body launch).
    all-long: every row above the 32 entries of the two-body launch's threshold.
    ell<w>: 0..w entries, the padded width of the ELL being w.  An integer w: every row w entries."""
    rng = np.random.default_rng(1000 + seed)
    if isinstance(shape, int):
        return np.full(m, shape, dtype=np.int64)
    if shape.startswith("ell"):             # ell10 / ell12 / ell14: rows of 0 .. that many entries, the longest several times
        width = int(shape[3:])
        lens = rng.integers(width - 6, width + 1, m)
        lens[[0, m // 2, m - 1]] = [0, width, 0]
        return lens
    if shape == "short":
        lens = rng.integers(1, 20, m)
        lens[[0, m // 2, m - 1]] = 0
        lens[[1, 2, 3, 4]] = [7, 8, 9, 17]
    elif shape == "long":
        lens = rng.integers(20, 71, m)
        lens[[5, m - 2]] = [150, 131]
        lens[[0, 9]] = [3, 0]
    elif shape == "tail":
        lens = rng.integers(0, 10, m)
        lens[[3, m // 3, m // 3 + 1, m // 2, m - 1]] = [190, 64, 129, 77, 33]
    else:
        assert shape == "all-long"
        lens = rng.integers(40, 90, m)
    if lens.sum() % m == 0:                 # keep nnz / M from dividing evenly: the general entry point's bet is another test
        lens[6] += 1
    return lens


def dense(rows, n, dtype=np.float32, seed=0):
    return fc.sharp_values(np.random.default_rng(500 + 7 * n + seed), (rows, n), dtype)


@functools.lru_cache(maxsize=None)
def _matrix(rows, m, k, seed, f64):
    csr = csr_from_lens(m, k, row_lengths(rows, m, seed), 77 + seed)
    if f64:
        csr = formats.CSR(m, k, csr.row_ptrs, csr.col_idxs, fc.sharp_values(np.random.default_rng(78), csr.nnz, np.float64))
    return csr


def spmm_operands(spec):
    """{csr, b}: the host CSR of spec['rows'] (see row_lengths) with spec.get('m', 150) x spec.get('k', 200), and B [k, n].
    The matrix is built once per shape and shared: read-only."""
    m, k = spec.get("m", M_ROWS), spec.get("k", K_COLS)
    csr = _matrix(spec["rows"], m, k, spec.get("seed", 0), bool(spec.get("f64")))
    return {"csr": csr, "b": dense(k, spec["n"], np.float64 if spec.get("f64") else np.float32)}


def block_pattern(bs, counts, nbc, seed, density=0.6):
    """A BSR of bs x bs blocks, counts[r] blocks in block row r at ascending distinct block columns below nbc; a block's
    elements are zero with probability 1 - density."""
    rng = np.random.default_rng(seed)
    cols = [np.sort(rng.choice(nbc, size=int(c), replace=False)) for c in counts]
    ptrs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    nb = int(ptrs[-1])
    data = np.where(rng.random((nb, bs, bs)) < density, fc.sharp_values(rng, (nb, bs, bs), np.float32), np.float32(0))
    return formats.BSR(len(counts) * bs, nbc * bs, nb * bs * bs, bs, bs, ptrs,
                       np.concatenate(cols + [np.zeros(0, np.int64)]).astype(np.uint32), data.astype(np.float32))


BLOCK_COUNTS = [3, 0, 1, 7, 5, 2, 9, 4, 0]      # blocks per block row: empty rows (the last among them), either side of 4 and 8


def bsr_operands(spec):
    """{bsr, b}: spec['bs'] x spec['bs'] blocks, BLOCK_COUNTS blocks per block row (spec.get('counts') replaces them)."""
    bs = spec["bs"]
    counts = spec.get("counts", BLOCK_COUNTS)
    nbc = spec.get("nbc", 12)
    bsr = block_pattern(bs, counts, nbc, 300 + bs, spec.get("density", 0.6))
    return {"bsr": bsr, "b": dense(nbc * bs, spec["n"])}


# ------------------------------------------------------------------------------------------------ the tables
# (lane group, vector width) -> the smallest N whose dispatch (pick_vec on contiguous, aligned operands, then pick_group on
# all of N) takes it: csr_k1 / csr_k2 / coo_k1 / bsr_valu, and row_gather where the column part is all of N
GV_N = {(8, 4): 4, (16, 4): 36, (32, 4): 68, (64, 4): 132, (8, 2): 2, (16, 2): 18, (32, 2): 34, (64, 2): 66,
        (8, 1): 1, (16, 1): 9, (32, 1): 17, (64, 1): 33}
MODES = {"ref64": "reference", "ref32": "reference", "fast": "fast", "ref": "reference"}

FAMILIES = {}
EXCLUSIONS = []


def _rows(family, rows):
    FAMILIES[family] = list(rows)


# ---- row_gather (row_gather.hpp: launch_row_gather_auto -> launch_row_gather -> launch_row_gather_b / launch_row_line)
def _row_gather():
    out = []
    # (rows tag, accumulate tag, ops entry): CsrRows of the CSR unit (kernel 0 / 5), CsrRows of the COO unit (a COO with its
    # row bounds; ELL's occupied slots and the BSR non-zero list are the same instances), UniformRows, EllRows
    combos = [("csr", "ref64", "csr"), ("csr", "fast", "csr"), ("csr", "ref32", "coo"), ("uniform", "ref64", "csr"),
              ("uniform", "fast", "csr"), ("ell", "ref32", "ell"), ("ell", "fast", "ell")]
    for rows, acc, fmt in combos:
        shape = 5 if rows == "uniform" else "short"
        for (g, v), n in GV_N.items():
            body = "roll" if g <= 16 else "batch"
            out.append(Row(f"row_gather<G{g},V{v},{acc},{rows},B128,U8,{body},S16>", dict(fmt=fmt, rows=shape, n=n, acc=MODES[acc])))
        if rows in ("uniform", "ell"):
            # rows of 9..14 slots and 16-byte vectors: the straight-line body with 10 / 12 / 14 slots.  UniformRows: the
            # odd width of each pair; EllRows: the even one as the padded width, shorter rows inside.
            for g, n in ((8, 4), (16, 36)):
                for slots in (10, 12, 14):
                    width = slots - 1 if rows == "uniform" else f"ell{slots}"
                    out.append(Row(f"row_gather<G{g},V4,{acc},{rows},B128,U8,line,S{slots}>", dict(fmt=fmt, rows=width, n=n, acc=MODES[acc])))
    # a mean row of 24 entries or more keeps the row-gather kernel in REFERENCE mode from N = 384 on; the deep body needs
    # 16-lane groups, i.e. column parts of 64 columns: N = 512
    out.append(Row("row_gather<G16,V4,ref64,csr,B128,U16,roll,S32>", dict(fmt="csr", rows="long", n=512, acc="reference", m=40)))
    # batched and plan-order launches: 16-byte vectors and column parts of whole 32-column groups only -- N = 32 (8 lanes)
    # and N = 64 (16 lanes)
    for rows, shape_slots in (("csr", [("short", "roll", 16)]),
                              ("uniform", [(5, "roll", 16), (9, "line", 10), (11, "line", 12), (13, "line", 14)])):
        for acc in ("ref64", "fast"):
            for g, n in ((8, 32), (16, 64)):
                for shape, body, slots in shape_slots:
                    head = f"row_gather<G{g},V4,{acc},{rows},B128,U8,{body},S{slots}>"
                    base = dict(fmt="csr", rows=shape, n=n, acc=MODES[acc])
                    out.append(Row(head + " batched", dict(base, batch=3)))
                    out.append(Row(head + " plan-order", dict(base, plan=True)))
                    out.append(Row(head + " batched plan-order", dict(base, plan=True, batch=3)))
    return out


_rows("row_gather", _row_gather())
# the four tilings xcd_tiling can return, each with a bitwise check (REFERENCE mode, CSR rows): 8x1 narrow N, 4x2 N = 128,
# 2x4 N = 256, 1x8 N = 512.  Not keys: the tiling is an argument of the launch.
ROW_GATHER_TILINGS = {(8, 1): dict(fmt="csr", rows="short", n=64, acc="reference", m=40),
                      (4, 2): dict(fmt="csr", rows="short", n=128, acc="reference", m=40),
                      (2, 4): dict(fmt="csr", rows="short", n=256, acc="reference", m=40),
                      (1, 8): dict(fmt="csr", rows="short", n=512, acc="reference", m=40)}
EXCLUSIONS += [
    Excluded("row_gather<G*,V4,*,uniform,B128,U8,roll,S1[024]>", "2gib", "row_line_fits: (col, val) arrays or C of 2 GiB or more; " + LINE_TEST),
    Excluded("row_gather<G*,V4,*,ell,B128,U8,roll,S1[024]>", "2gib", "row_line_fits: (col, val) arrays or C of 2 GiB or more; " + LINE_TEST),
    Excluded("row_gather<G*,V4,*,uniform,B128,U8,roll,S1[024]> *", "unreachable",
             "launch_row_line declines only past 2 GiB (row_line_fits), where the batched and the row-mapped launches are declined too"),
    Excluded("row_gather<G16,V4,fast,csr,B128,U16,roll,S32>", "knob", "launch_csr: FAST takes csr_split whenever the mean row is long; MISPMM_SPLIT=0"),
    Excluded("row_gather<G16,V4,ref32,csr,B128,U16,roll,S32>", "knob", "launch_rows: long rows of 16-byte vectors take csr_split; MISPMM_SPLIT=0"),
    Excluded("row_gather<G*,V[12],*,*,B128,U8,roll,S16> batched*", "unreachable",
             "mispmm_csr_batch_f32 / mispmm_csr_plan_f32: `vec != 4` sends the operands out one launch each"),
    Excluded("row_gather<G*,V4,ref32,*> batched*", "unreachable", "only the CSR entry points (ref64 / fast) have a batched form"),
    Excluded("row_gather<G*,V4,ref32,csr,B128,U8,roll,S16> plan-order", "unreachable", "no entry point of the COO unit passes a row map"),
    Excluded("row_gather<G*,V4,*,ell,*> *", "unreachable", "mispmm_ell_f32 has neither a batched nor a plan-order form"),
]
# (the bodies behind MISPMM_ROLL / MISPMM_UMAX / MISPMM_BLOCK exist in the tuning build only: the production library holds no
# instance of them, so they need no entry; tests/test_census_cpu.py checks that every instance it does hold is listed)

# ---- csr_k1 / csr_k2 / csr_wide (spmm_csr.hip: launch_grouped), csr_k3 (launch_wave), csr_wave_deep (launch_wave_deep)
for _k in (1, 2):
    _rows(f"csr_k{_k}", [Row(f"csr_k{_k}<G{g},V{v},{acc}>", dict(fmt="csr", rows="short", n=n, acc=MODES[acc], kernel=_k))
                         for acc in ("ref64", "fast") for (g, v), n in GV_N.items()])
_rows("csr_wide", [])
EXCLUSIONS.append(Excluded("csr_wide<*>", "2gib", "launch_csr: a B of 2 GiB or more; " + WIDE_TEST))
# wave per row: the vector narrows until a wave is not mostly idle -- V4 from N = 132, V2 for 66..128, V1 up to 64
_rows("csr_k3", [Row(f"csr_k3<V{v},R{r},{acc}>", dict(fmt="csr", rows="short", n=n, acc=MODES[acc], kernel=k))
                 for acc in ("ref64", "fast") for k, r in ((3, 1), (4, 2)) for v, n in ((4, 132), (2, 66), (1, 1))])
# long rows whose B rows are no 16-byte vectors, N < 384
_rows("csr_wave_deep", [Row(f"csr_wave_deep<V{v},{acc}>", dict(fmt="csr", rows="long", n=n, acc=MODES[acc], kernel=5, spans=False, m=40))
                        for acc in ("ref64", "fast") for v, n in ((2, 66), (1, 1))])
EXCLUSIONS.append(Excluded("csr_wave_deep<V4,*>", "knob", "launch_csr: 16-byte vectors below N = 384 take csr_split; MISPMM_SPLIT=0 or MISPMM_LONGROWS=1"))

# ---- csr_split (csr_split.hpp: launch_split) and csr_hybrid (csr_hybrid.hpp: launch_hybrid)
_rows("csr_split", [
    Row("csr_split<W4,R8,ref64>", dict(fmt="csr", rows="long", n=4, acc="reference", kernel=6, spans=False, m=40)),
    Row("csr_split<W4,R8,fast>", dict(fmt="csr", rows="long", n=4, acc="fast", kernel=6, spans=False, m=40)),
    Row("csr_split<W4,R8,ref64,longest-first>", dict(fmt="csr", rows="long", n=4, acc="reference", kernel=6, spans=True, m=40)),
    Row("csr_split<W4,R8,fast,longest-first>", dict(fmt="csr", rows="long", n=4, acc="fast", kernel=6, spans=True, m=40)),
    # the fp32 arithmetic of COO / ELL / BSR: a COO without a span list (rows in order), one with (every row long: no two-body launch)
    Row("csr_split<W4,R8,ref32>", dict(fmt="coo", rows="long", n=4, acc="reference", spans=False, m=40)),
    Row("csr_split<W4,R8,ref32,longest-first>", dict(fmt="coo", rows="all-long", n=4, acc="reference", m=40)),
])
# one launch, two bodies: N a multiple of 32 up to 256; the production library always aligns the row-gather body to the split
# body's 32-column parts (8 lanes)
_rows("csr_hybrid", [
    Row("csr_hybrid<ref64,R8>+row_gather<G8,spans>", dict(fmt="csr", rows="tail", n=32, acc="reference", m=60)),
    Row("csr_hybrid<fast,R8>+row_gather<G8,spans>", dict(fmt="csr", rows="tail", n=32, acc="fast", m=60)),
    Row("csr_hybrid<ref32,R8>+row_gather<G8,spans>", dict(fmt="coo", rows="tail", n=32, acc="reference", m=60)),
])
EXCLUSIONS.append(Excluded("csr_hybrid<*,R8>+row_gather<G16,spans>", "knob", "launch_hybrid: 64-column parts only with MISPMM_HYBRID_ALIGN=0"))

# ---- coo_k1 (spmm_coo.hip: launch_coo_v): a COO without its row bounds
_rows("coo_k1", [Row(f"coo_k1<G{g},V{v},{acc}>", dict(fmt="coo", rows="short", n=n, acc=MODES[acc], workspace=False))
                 for acc in ("ref32", "fast") for (g, v), n in GV_N.items()])
EXCLUSIONS.append(Excluded("coo_k1<*,wide>", "2gib", "launch_coo: a B of 2 GiB or more; " + WIDE_TEST))

# ---- bsr_valu, bsr_rowblock, bsr_mfma_f32 (spmm_bsr.hip: launch_valu_v / try_rowblock / mispmm_bsr_f32)
# 2 x 2 blocks have no block-row kernel
_rows("bsr_valu", [Row(f"bsr_valu<G{g},V{v},{acc}>", dict(bs=2, nbc=40, counts=[3, 0, 1, 7, 5, 2, 9, 4, 0] * 8, n=n, acc=MODES[acc], kernel=1))
                   for acc in ("ref32", "fast") for (g, v), n in GV_N.items()])
# 16-byte vectors only above N = 128 (below, two columns per lane keep the wave busy)
_rows("bsr_rowblock", [Row(f"bsr_rowblock<BD{bd},RS{min(bd, 8)},V{v},{acc}>", dict(bs=bd, n=n, acc=MODES[acc], kernel=1))
                       for acc in ("ref32", "fast") for bd in (4, 8, 16, 32) for v, n in ((4, 132), (2, 2), (1, 1))])
_rows("bsr_mfma_f32", [Row("bsr_mfma_f32", dict(bs=16, n=4, acc="fast", kernel=0))])

# ---- the bf16 MFMA products (spmm_bsr.hip: mispmm_bsr_bf16, mispmm_bsrc_bf16, mispmm_bsrc_slots_bf16)
# T8: N >= 128 in whole 8-column vectors; T4: everything else in whole 4-column vectors
_rows("bsr_mfma_bf16", [Row(f"bsr_mfma_bf16<T{t},{c}>", dict(op="bsr", bs=16, n=n, out_bf16=c == "c16"))
                        for t, n in ((4, 4), (8, 128)) for c in ("c32", "c16")])
_rows("bsr_mfma_bf16_b32", [Row(f"bsr_mfma_bf16_b32<T{t},{c}>", dict(op="bsr", bs=32, n=n, out_bf16=c == "c16"))
                            for t, n in ((4, 4), (8, 128)) for c in ("c32", "c16")])
_rows("bsr_bf16_lds", [])
EXCLUSIONS.append(Excluded("bsr_bf16_lds<*>", "knob", "MISPMM_BSR_LDS=1"))
_rows("bsrc_mfma_bf16", [Row(f"bsrc_mfma_bf16<{c}>", dict(op="bsrc", bs=16, n=8, out_bf16=c == "c16")) for c in ("c32", "c16")])
# share: no block row has more than 4 steps (at most 4 blocks of 16 columns = 64 occupied columns = 2 steps here) and C is fp32
_rows("bsrc_slots_mfma_bf16", [
    Row("bsrc_slots_mfma_bf16<c32,nt,share>", dict(op="slots", bs=16, n=8, out_bf16=False, counts=[3, 0, 1, 4, 2, 0])),
    Row("bsrc_slots_mfma_bf16<c32,nt>", dict(op="slots", bs=16, n=8, out_bf16=False, counts=[3, 0, 1, 12, 2, 10, 0], density=1.0)),
    Row("bsrc_slots_mfma_bf16<c16,nt>", dict(op="slots", bs=16, n=8, out_bf16=True, counts=[3, 0, 1, 12, 2, 10, 0], density=1.0)),
])
EXCLUSIONS += [
    Excluded("bsrc_slots_mfma_bf16<c16,nt,share>", "knob", "MISPMM_BSR_SHARE=2"),
    Excluded("bsrc_slots_mfma_bf16<c16,plain,share>", "knob", "MISPMM_BSR_SHARE=2"),
    Excluded("bsrc_slots_mfma_bf16<c32,plain*", "2gib", "a C of 2 GiB or more takes plain stores; no test runs it"),
    Excluded("bsrc_slots_mfma_bf16<c16,plain>", "2gib", "a C of 2 GiB or more takes plain stores; no test runs it"),
    Excluded("bsrc_slots_mfma_bf16<*,sc1*", "knob", "MISPMM_BSR_STORE=16 / 18"),
]

# ---- csr_f64 (spmm_f64.hip: launch_f64_acc): 16-byte lanes for even N, lane group from N
_rows("csr_f64", [Row(f"csr_f64<G{g},V{v},{acc}>", dict(fmt="csr", rows="short", n=GV_N[(g, v)], acc=MODES[acc], f64=True))
                  for acc in ("ref", "fast") for v in (2, 1) for g in (8, 16, 32, 64)])
EXCLUSIONS.append(Excluded("csr_f64<*,wide>", "2gib", "launch_f64_acc: B or C of 2 GiB or more; " + F64_WIDE_TEST))

# ---- csr_lds_tile (spmm_tiles.hip), csr_panel (spmm_panels.hip): column parts of whole 64-column groups
_rows("csr_lds_tile", [Row(f"csr_lds_tile<{acc},lds-dma>", dict(rows=9, n=64, acc=MODES[acc])) for acc in ("ref64", "fast")])
_rows("csr_panel", [Row(f"csr_panel<{acc},P{p},R64,lds-dma>", dict(rows="short", n=4, acc=MODES[acc], panel_rows=p, m=100))
                    for acc in ("ref", "fast") for p in (64, 128)])

# ---- sddmm_csr (sddmm.hip: launch_sddmm_shape): per arithmetic 16-byte lanes (V4 fp32 / V2 fp64) or one element per lane,
# lane groups of 8 / 16 / 32 and, with the whole wave, 1 / 2 / 4 register chunks or the chunk loop (C0).  The smallest N of
# each class, except the seven classes no width of tests/test_gpu_sddmm.py reaches: those keep the widths they were reported
# with (fp32 128, 13, 27; fp64 20, 100, 13, 27).
SDDMM_N = {"f32": {(8, 4, 1): 4, (16, 4, 1): 36, (32, 4, 1): 128, (64, 4, 1): 132, (64, 4, 2): 260, (64, 4, 4): 516, (64, 4, 0): 1028,
                   (8, 1, 1): 1, (16, 1, 1): 13, (32, 1, 1): 27, (64, 1, 1): 33, (64, 1, 2): 65, (64, 1, 4): 129, (64, 1, 0): 257},
           "f64": {(8, 2, 1): 2, (16, 2, 1): 20, (32, 2, 1): 34, (64, 2, 1): 100, (64, 2, 2): 130, (64, 2, 4): 258, (64, 2, 0): 514,
                   (8, 1, 1): 1, (16, 1, 1): 13, (32, 1, 1): 27, (64, 1, 1): 33, (64, 1, 2): 65, (64, 1, 4): 129, (64, 1, 0): 257}}
_rows("sddmm_csr", [Row(f"sddmm_csr<{dt},{acc},G{g},V{v},C{c}>", dict(rows="short", n=n, acc=MODES[acc], f64=dt == "f64", m=70, k=90))
                    for dt, accs in (("f32", ("ref64", "fast")), ("f64", ("ref", "fast"))) for acc in accs
                    for (g, v, c), n in SDDMM_N[dt].items()])

# ---- sddmm_bsr (sddmm_bsr.hip: launch_sddmm_bsr_width): whole 8-column vectors (wide) or not, N <= 128 / <= 256 / more
_rows("sddmm_bsr", [Row(f"sddmm_bsr<b{bs},{w},{o},{body}>", dict(pattern=f"ragged{bs}", n=n, out_bf16=o == "bf16"))
                    for bs in (16, 32) for o in ("f32", "bf16")
                    for w, body, n in (("wide", "hold4", 8), ("wide", "hold8", 136), ("wide", "loop8", 264),
                                       ("narrow", "hold4", 4), ("narrow", "loop4", 132))])

# ---- softmax_csr and its backward (softmax_csr.hip: sm_pick_group): the lane group from the mean row, ceil(nnz / M):
# 4 lanes up to 16 entries, then 8 / 16 / 32 up to 32 / 64 / 128, the whole wave beyond.  (mean row, rows): a row shorter
# and one longer than the 4 G entries the registers hold in every matrix.
SOFTMAX_SHAPES = {4: (12, 150), 8: (24, 70), 16: (48, 40), 32: (96, 20), 64: (200, 10)}
for _name in ("softmax_csr", "softmax_csr_bwd"):
    _rows(_name, [Row(f"{_name}<{dt},{acc},G{g},R4>", dict(g=g, acc=MODES[acc], f64=dt == "f64"))
                  for dt, accs in (("f32", ("ref64", "fast")), ("f64", ("ref", "fast"))) for acc in accs for g in SOFTMAX_SHAPES])

def softmax_csr_pattern(g):
    """Row pointers for the lane group g of SOFTMAX_SHAPES: rows around the mean, an empty row, a row of one entry, a
    row that just fits the registers (4 g entries) and one that does not (4 g + 3)."""
    mean, m = SOFTMAX_SHAPES[g]
    rng = np.random.default_rng(40 + g)
    lens = rng.integers(mean - 4, mean + 5, m)
    lens[[0, 1, 2, 3]] = [0, 4 * g + 3, 4 * g, 1]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    assert _softmax_ref.picked_group(m, int(ptr[-1])) == g
    return ptr


# ---- softmax_bsr and its backward (softmax_bsr.hip: launch_fwd_body / launch_bwd_body).  held / walk is the host's word
# for whether any block row can exceed the C blocks held in registers (numBlocks <= C): kept, the kernel takes another path.
SOFTMAX_BSR_HELD = {16: 32, 32: 16}      # kHeld<BS> of csrc/softmax_bsr.hip
SOFTMAX_BSR_PATTERNS = {(16, "held"): "ragged16", (16, "walk"): "edges16", (32, "held"): "ragged32", (32, "walk"): "edges32"}
_rows("softmax_bsr", [Row(f"softmax_bsr<b{bs},{o},{path},C{SOFTMAX_BSR_HELD[bs]},{mk}>",
                          dict(pattern=SOFTMAX_BSR_PATTERNS[(bs, path)], out_bf16=o == "bf16", mask=mk == "mask"))
                      for bs in (16, 32) for o in ("f32", "bf16") for path in ("held", "walk") for mk in ("mask", "nomask")])
_rows("softmax_bsr_bwd", [Row(f"softmax_bsr_bwd<b{bs},{o},{path},C{SOFTMAX_BSR_HELD[bs]},p_{p}>",
                              dict(pattern=SOFTMAX_BSR_PATTERNS[(bs, path)], out_bf16=o == "bf16", p_bf16=p == "bf16"))
                          for bs in (16, 32) for o in ("f32", "bf16") for path in ("held", "walk") for p in ("f32", "bf16")])

# ---- row_stream (spmm_stream.hip): compiled into the tuning build only
EXCLUSIONS.append(Excluded("row_stream<*", "knob", "MISPMM_STREAM=1; the production library does not carry the kernels "
                           "(tests/test_gpu_spmm.py::test_production_library_never_takes_the_persistent_launch)"))


# ------------------------------------------------------------------------------------------------ the sweeps
# What a family's set check launches besides its rows: the cross product of the properties its dispatcher looks at, without
# any expectation.  Every key a sweep meets -- whichever family it falls into -- must be a row of that family's table: an
# instance the tables do not know shows up here.  Launches only; the rows above carry the comparisons.
SWEEP_N = (1, 2, 4, 9, 17, 18, 32, 33, 34, 36, 64, 66, 68, 96, 128, 132, 192, 256, 384, 512)
_ACCS = ("reference", "fast")


def _cross(**axes):
    names = list(axes)
    return [dict(zip(names, values)) for values in itertools.product(*(axes[n] for n in names))]


_LONG_ROWS = (_cross(fmt=["csr"], rows=["long", "tail", "all-long"], kernel=[0, 6], spans=[None, False, True], acc=_ACCS,
                     n=[1, 4, 32, 66, 128, 256, 384, 512], m=[40])
              + _cross(fmt=["coo"], rows=["long", "tail", "all-long"], spans=[None, False], acc=_ACCS, n=[1, 4, 32, 64, 128, 256], m=[40]))
SWEEPS = {
    "row_gather": (_cross(fmt=["csr"], rows=["short", 5, 9, 11, 13, 16], acc=_ACCS, n=SWEEP_N)
                   + _cross(fmt=["coo"], rows=["short"], acc=_ACCS, n=SWEEP_N)
                   + _cross(fmt=["ell"], rows=["short", "ell10", "ell12", "ell14"], acc=_ACCS, n=SWEEP_N)
                   + _cross(fmt=["csr"], rows=["short", 5, 10, 12, 14], acc=_ACCS, n=[4, 32, 64, 96, 128, 256, 512], batch=[2], plan=[None, True])
                   + _cross(fmt=["csr"], rows=["short", 5, 10, 12, 14], acc=_ACCS, n=[4, 32, 64, 96, 128, 256, 512], plan=[True])),
    "csr_k1": _cross(fmt=["csr"], rows=["short", 5], kernel=[1], acc=_ACCS, n=SWEEP_N),
    "csr_k2": _cross(fmt=["csr"], rows=["short", 5], kernel=[2], acc=_ACCS, n=SWEEP_N),
    "csr_k3": _cross(fmt=["csr"], rows=["short", "long"], kernel=[3, 4], acc=_ACCS, n=SWEEP_N, m=[40]),
    "csr_wave_deep": _LONG_ROWS, "csr_split": _LONG_ROWS, "csr_hybrid": _LONG_ROWS,
    "coo_k1": _cross(fmt=["coo"], rows=["short", "long"], workspace=[False], acc=_ACCS, n=SWEEP_N, m=[40]),
    "csr_f64": _cross(fmt=["csr"], rows=["short", "long"], f64=[True], acc=_ACCS, n=SWEEP_N, m=[40]),
    "bsr_valu": _cross(bs=[2], kernel=[0, 1], acc=_ACCS, n=SWEEP_N),
    "bsr_rowblock": _cross(bs=[4, 8, 16, 32], kernel=[0, 1], acc=_ACCS, n=[1, 2, 4, 34, 36, 128, 130, 132, 256]),
    "bsr_mfma_f32": _cross(bs=[16], kernel=[0, 2], acc=["fast"], n=[4, 36, 64, 132]),
    "bsr_mfma_bf16": _cross(op=["bsr"], bs=[16], out_bf16=[False, True], n=[4, 8, 36, 64, 124, 128, 132, 136, 256]),
    "bsr_mfma_bf16_b32": _cross(op=["bsr"], bs=[32], out_bf16=[False, True], n=[4, 8, 36, 64, 124, 128, 132, 136, 256]),
    "bsrc_mfma_bf16": _cross(op=["bsrc"], bs=[16], out_bf16=[False, True], n=[8, 64, 128, 136, 256]),
    "bsrc_slots_mfma_bf16": _cross(op=["slots"], bs=[16], out_bf16=[False, True], n=[8, 64, 128, 136, 256],
                                   counts=[[3, 0, 1, 4, 2, 0], [3, 0, 1, 12, 2, 10, 0]], density=[1.0]),
    "csr_lds_tile": _cross(rows=[1, 8, 9, 12, 13, 14, 15, 16], acc=_ACCS, n=[64, 128, 256, 512]),
    "csr_panel": _cross(rows=["short", "long"], acc=_ACCS, panel_rows=[64, 128], n=[4, 64, 100, 256], m=[100]),
    "sddmm_csr": _cross(rows=["short"], f64=[False, True], acc=_ACCS, m=[70], k=[90],
                        n=sorted({1, 2, 3, 4, 8, 9, 16, 17, 18, 32, 33, 34, 36, 64, 65, 66, 68, 128, 129, 130, 132, 255, 256, 257, 258,
                                  260, 512, 514, 516, 1024, 1028})),
    "sddmm_bsr": _cross(pattern=["ragged16", "ragged32"], out_bf16=[False, True], n=[1, 4, 8, 33, 128, 129, 132, 136, 256, 257, 264, 520]),
    "softmax_csr": _cross(g=list(SOFTMAX_SHAPES), acc=_ACCS, f64=[False, True]),
    "softmax_csr_bwd": _cross(g=list(SOFTMAX_SHAPES), acc=_ACCS, f64=[False, True]),
    "softmax_bsr": _cross(pattern=["ragged16", "edges16", "ragged32", "edges32"], out_bf16=[False, True], mask=[False, True]),
    "softmax_bsr_bwd": _cross(pattern=["ragged16", "edges16", "ragged32", "edges32"], out_bf16=[False, True], p_bf16=[False, True]),
}


def family_of(key):
    """The table a key belongs to: its text up to `<`."""
    return key.split("<")[0].split(" ")[0]


def excluded(key):
    """The EXCLUSIONS entry a key falls under, or None."""
    for e in EXCLUSIONS:
        if fnmatch.fnmatchcase(key, e.pattern):
            return e
    return None


def all_rows():
    return [(family, row) for family, rows in FAMILIES.items() for row in rows]
