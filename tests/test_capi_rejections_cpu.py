"""What every compute entry point of the C ABI rejects, or accepts as a no-op, BEFORE any device work: status and
mispmm_last_error() text, row by row, in the order the checks fire.

Every row below returns from argument validation: the non-null pointers are the constant 16 and are never dereferenced
(the operand lists of the batch / plan entries are real host arrays that hold that constant).  The module is for machines
without a GPU, where a check that wrongly passes cannot reach a device; it skips where there is one.  The host-only
entries (*_host, mispmm_autotune_pick) are covered by test_capi_cpu.py.
"""
import ctypes

import pytest

from mispmm import capi

try:
    import torch
    _HAS_GPU = torch.cuda.is_available()
except ImportError:
    _HAS_GPU = False
pytestmark = pytest.mark.skipif(_HAS_GPU, reason="rejection table: only where no call can reach a device")

OK, INV, UNS = capi.OK, capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
P = ctypes.c_void_p(16)          # a pointer that must be non-null; never dereferenced
P8 = ctypes.c_void_p(8)          # non-null but not 16-byte aligned
LIST = (ctypes.c_void_p * 1)(16)  # a host list of one device pointer
NULLS = (ctypes.c_void_p * 1)(None)
BIG = dict(K=1 << 20, ldb=1 << 10)   # K * ldb * 4 bytes = 4 GiB (bf16: 2 GiB)
NOMSG = None                     # UNSUPPORTED without a message of its own: the text is not looked at

# entry -> (parameter names in call order, arguments that pass every check)
ENTRIES = {
    "mispmm_csr_f32": ("stream M K nnz rowPtrs colIdxs vals B N ldb C ldc kernel acc",
                       dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, vals=P, B=P, N=8, ldb=8, C=P, ldc=8, kernel=0, acc=0)),
    "mispmm_csr_uniform_f32": ("stream M K rowNnz colIdxs vals B N ldb C ldc acc",
                               dict(M=4, K=4, rowNnz=2, colIdxs=P, vals=P, B=P, N=8, ldb=8, C=P, ldc=8, acc=0)),
    "mispmm_csr_split_f32": ("stream M K nnz rowPtrs colIdxs vals spans numSpans B N ldb C ldc acc",
                             dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, vals=P, spans=P, numSpans=4, B=P, N=8, ldb=8, C=P, ldc=8, acc=0)),
    "mispmm_csr_hybrid_f32": ("stream M K nnz colIdxs vals spans numSpans numLongSpans B N ldb C ldc acc",
                              dict(M=4, K=4, nnz=3, colIdxs=P, vals=P, spans=P, numSpans=4, numLongSpans=4, B=P, N=8, ldb=8, C=P, ldc=8,
                                   acc=0)),
    "mispmm_csr_batch_f32": ("stream M K nnz rowPtrs colIdxs vals uniformRowNnz batch B_list N ldb C_list ldc acc",
                             dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, vals=P, uniformRowNnz=0, batch=1, B_list=LIST, N=8, ldb=8,
                                  C_list=LIST, ldc=8, acc=0)),
    "mispmm_csr_plan_f32": ("stream M K nnz rowPtrs colIdxs vals uniformRowNnz rowMap batch B_list N ldb C_list ldc acc",
                            dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, vals=P, uniformRowNnz=0, rowMap=None, batch=1, B_list=LIST, N=8, ldb=8,
                                 C_list=LIST, ldc=8, acc=0)),
    "mispmm_csr_lds_tile_f32": ("stream M K rowNnz numTiles maxTileCols tileRowPtrs tileColPtrs tileCols slots vals rowMap B N ldb C ldc acc",
                                dict(M=4, K=4, rowNnz=2, numTiles=1, maxTileCols=4, tileRowPtrs=P, tileColPtrs=P, tileCols=P, slots=P, vals=P,
                                     rowMap=P, B=P, N=64, ldb=64, C=P, ldc=64, acc=0)),
    "mispmm_csr_panel_f32": ("stream M K nnz rowPtrs colIdxs vals panelPtrs panelRows B N ldb C ldc acc",
                             dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, vals=P, panelPtrs=P, panelRows=128, B=P, N=8, ldb=8, C=P, ldc=8, acc=0)),
    "mispmm_coo_f32": ("stream M K nnz rowIdxs colIdxs vals B N ldb C ldc workspace kernel acc",
                       dict(M=4, K=4, nnz=3, rowIdxs=P, colIdxs=P, vals=P, B=P, N=8, ldb=8, C=P, ldc=8, workspace=P, kernel=0, acc=0)),
    "mispmm_rows_split_f32": ("stream M K nnz colIdxs vals spans numSpans B N ldb C ldc acc",
                              dict(M=4, K=4, nnz=3, colIdxs=P, vals=P, spans=P, numSpans=4, B=P, N=8, ldb=8, C=P, ldc=8, acc=0)),
    "mispmm_rows_hybrid_f32": ("stream M K nnz colIdxs vals spans numSpans numLongSpans B N ldb C ldc acc",
                               dict(M=4, K=4, nnz=3, colIdxs=P, vals=P, spans=P, numSpans=4, numLongSpans=4, B=P, N=8, ldb=8, C=P, ldc=8,
                                    acc=0)),
    "mispmm_ell_compact_f32": ("stream M K nnz rowPtrs colIdxs vals B N ldb C ldc acc",
                               dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, vals=P, B=P, N=8, ldb=8, C=P, ldc=8, acc=0)),
    "mispmm_bsr_nonzeros_f32": ("stream M K nnz rowPtrs colIdxs vals B N ldb C ldc acc",
                                dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, vals=P, B=P, N=8, ldb=8, C=P, ldc=8, acc=0)),
    "mispmm_ell_f32": ("stream M K width colIdxs vals B N ldb C ldc kernel acc",
                       dict(M=4, K=4, width=2, colIdxs=P, vals=P, B=P, N=8, ldb=8, C=P, ldc=8, kernel=0, acc=0)),
    "mispmm_bsr_f32": ("stream Mb K bR bC numBlocks ptrs idxs blocks B N ldb C ldc kernel acc",
                       dict(Mb=2, K=8, bR=4, bC=4, numBlocks=2, ptrs=P, idxs=P, blocks=P, B=P, N=8, ldb=8, C=P, ldc=8, kernel=0, acc=0)),
    "mispmm_bsr_bf16": ("stream Mb K bR bC numBlocks ptrs idxs blocks B N ldb C ldc c_bf16",
                        dict(Mb=2, K=32, bR=16, bC=16, numBlocks=2, ptrs=P, idxs=P, blocks=P, B=P, N=8, ldb=8, C=P, ldc=8, c_bf16=0)),
    "mispmm_bsrc_bf16": ("stream Mb K nSteps stepPtrs cols tiles B N ldb C ldc c_bf16",
                         dict(Mb=2, K=32, nSteps=2, stepPtrs=P, cols=P, tiles=P, B=P, N=8, ldb=8, C=P, ldc=8, c_bf16=0)),
    "mispmm_bsrc_slots_bf16": ("stream Mb K nSteps extraPtrs cols tiles B N ldb C ldc c_bf16",
                               dict(Mb=2, K=32, nSteps=8, extraPtrs=P, cols=P, tiles=P, B=P, N=8, ldb=8, C=P, ldc=8, c_bf16=0)),
    "mispmm_csr_f64": ("stream M K nnz rowPtrs colIdxs vals B N ldb C ldc acc",
                       dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, vals=P, B=P, N=8, ldb=8, C=P, ldc=8, acc=0)),
    "mispmm_sddmm_csr_f32": ("stream M K nnz rowPtrs colIdxs X ldx Y ldy N out acc",
                             dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, X=P, ldx=8, Y=P, ldy=8, N=8, out=P, acc=0)),
    "mispmm_sddmm_csr_f64": ("stream M K nnz rowPtrs colIdxs X ldx Y ldy N out acc",
                             dict(M=4, K=4, nnz=3, rowPtrs=P, colIdxs=P, X=P, ldx=8, Y=P, ldy=8, N=8, out=P, acc=0)),
    "mispmm_sddmm_bsr_bf16": ("stream Mb K bS numBlocks ptrs idxs X ldx Y ldy N out out_bf16",
                              dict(Mb=2, K=32, bS=16, numBlocks=2, ptrs=P, idxs=P, X=P, ldx=8, Y=P, ldy=8, N=8, out=P, out_bf16=0)),
    "mispmm_softmax_csr_f32": ("stream M nnz rowPtrs scores out acc", dict(M=4, nnz=3, rowPtrs=P, scores=P, out=P, acc=0)),
    "mispmm_softmax_csr_f64": ("stream M nnz rowPtrs scores out acc", dict(M=4, nnz=3, rowPtrs=P, scores=P, out=P, acc=0)),
    "mispmm_softmax_csr_bwd_f32": ("stream M nnz rowPtrs p dp ds acc", dict(M=4, nnz=3, rowPtrs=P, p=P, dp=P, ds=P, acc=0)),
    "mispmm_softmax_csr_bwd_f64": ("stream M nnz rowPtrs p dp ds acc", dict(M=4, nnz=3, rowPtrs=P, p=P, dp=P, ds=P, acc=0)),
    "mispmm_softmax_bsr_f32": ("stream Mb bS numBlocks ptrs scores mask scale out out_bf16",
                               dict(Mb=2, bS=16, numBlocks=2, ptrs=P, scores=P, mask=P, scale=1.0, out=P, out_bf16=0)),
    "mispmm_softmax_bsr_bwd_f32": ("stream Mb bS numBlocks ptrs p p_bf16 dp scale ds ds_bf16",
                                   dict(Mb=2, bS=16, numBlocks=2, ptrs=P, p=P, p_bf16=0, dp=P, scale=1.0, ds=P, ds_bf16=0)),
}


def _all_wrong(entry, **more):
    """every pointer null, every id and mode unknown, every leading dimension too small: the text names the first check"""
    names, good = ENTRIES[entry]
    bad = {k: None for k, v in good.items() if v is P or v is LIST}
    for k in ("ldb", "ldc", "ldx", "ldy"):
        if k in good:
            bad[k] = 1
    if "kernel" in good:
        bad["kernel"] = 9
    if "acc" in good:
        bad["acc"] = 5
    bad.update(more)
    return bad


def _row_list(entry, prefix, big_text):
    """the rows shared by the entries that take one row list (rowPtrs, colIdxs, vals) and refuse a B of 2 GiB"""
    return [
        (entry, dict(acc=2), INV, f"{prefix}: unknown accumulate mode 2"),
        (entry, dict(acc=-1, M=0), INV, f"{prefix}: unknown accumulate mode -1"),
        (entry, dict(M=0, rowPtrs=None, colIdxs=None, vals=None, B=None, C=None, ldb=1), OK, None),
        (entry, dict(N=0, rowPtrs=None, colIdxs=None, vals=None, B=None, C=None), OK, None),
        (entry, dict(rowPtrs=None), INV, f"{prefix}: rowPtrs is null"),
        (entry, dict(colIdxs=None), INV, f"{prefix}: colIdxs or vals is null"),
        (entry, dict(vals=None), INV, f"{prefix}: colIdxs or vals is null"),
        (entry, dict(nnz=0, colIdxs=None, vals=None, B=None), INV, "B or C is null"),
        (entry, dict(B=None), INV, "B or C is null"),
        (entry, dict(C=None), INV, "B or C is null"),
        (entry, dict(ldb=7), INV, "leading dimension smaller than N (N=8 ldb=7 ldc=8)"),
        (entry, dict(ldc=7), INV, "leading dimension smaller than N (N=8 ldb=8 ldc=7)"),
        (entry, dict(BIG), UNS, big_text),
        (entry, _all_wrong(entry), INV, f"{prefix}: unknown accumulate mode 5"),
        (entry, _all_wrong(entry, acc=1), INV, f"{prefix}: rowPtrs is null"),
    ]


def _softmax_csr(entry, what):
    tag = entry[len("mispmm_"):]
    rows = [
        (entry, dict(acc=2), INV, f"{tag}: unknown accumulate mode 2"),
        (entry, dict(acc=7, nnz=0), INV, f"{tag}: unknown accumulate mode 7"),
        (entry, dict(M=0, nnz=0, rowPtrs=None), OK, None),
        (entry, dict(nnz=0, rowPtrs=None), OK, None),
        (entry, dict(rowPtrs=None), INV, f"{tag}: {what} is null"),
        (entry, _all_wrong(entry), INV, f"{tag}: unknown accumulate mode 5"),
        (entry, _all_wrong(entry, acc=1), INV, f"{tag}: {what} is null"),
    ]
    for name in ENTRIES[entry][0].split()[4:-1]:   # scores, out / p, dp, ds
        rows.append((entry, {name: None}, INV, f"{tag}: {what} is null"))
    return rows


def _sddmm_csr(entry):
    tag = entry[len("mispmm_"):]
    return [
        (entry, dict(acc=2), INV, f"{tag}: unknown accumulate mode 2"),
        (entry, dict(acc=2, nnz=0), INV, f"{tag}: unknown accumulate mode 2"),
        (entry, dict(M=0, rowPtrs=None, out=None), OK, None),
        (entry, dict(nnz=0, N=0, rowPtrs=None, out=None, X=None), OK, None),
        (entry, dict(rowPtrs=None), INV, f"{tag}: rowPtrs, colIdxs or out is null"),
        (entry, dict(colIdxs=None), INV, f"{tag}: rowPtrs, colIdxs or out is null"),
        (entry, dict(out=None), INV, f"{tag}: rowPtrs, colIdxs or out is null"),
        (entry, dict(ldx=7), INV, f"{tag}: leading dimension smaller than N (N=8 ldx=7 ldy=8)"),
        (entry, dict(ldy=7), INV, f"{tag}: leading dimension smaller than N (N=8 ldx=8 ldy=7)"),
        (entry, dict(X=None), INV, f"{tag}: X or Y is null"),
        (entry, dict(Y=None), INV, f"{tag}: X or Y is null"),
        (entry, dict(M=1 << 20, ldx=1 << 10), UNS, f"{tag}: X or Y spans 2 GiB or more (M=1048576 ldx=1024 K=4 ldy=8)"),
        (entry, dict(K=1 << 20, ldy=1 << 10), UNS, f"{tag}: X or Y spans 2 GiB or more (M=4 ldx=8 K=1048576 ldy=1024)"),
        (entry, _all_wrong(entry), INV, f"{tag}: unknown accumulate mode 5"),
        (entry, _all_wrong(entry, acc=1), INV, f"{tag}: rowPtrs, colIdxs or out is null"),
    ]


_LD = "leading dimension smaller than N (N=8 ldb=7 ldc=8)"
_PLAN_MAP = ("csr_plan: the row-mapped kernel takes 16-byte-aligned operands with N a multiple of 32 (per XCD column part), "
             "C below 2 GiB and short rows: multiply from the unpermuted arrays")
_TILE_SHAPE = "csr_lds_tile: 16-byte-aligned operands, column parts of whole 64-column groups, B and C below 2 GiB"
_PANEL_SHAPE = "csr_panel: N a multiple of 4 with 16-byte-aligned B, C, ldb, ldc; B, C and the entries below 2 GiB"
_BSRC = "bsrc_bf16: N / ldb / ldc must be multiples of 8, operands 16-byte aligned, B below 2 GiB"
_SLOTS = "bsrc_slots_bf16: N / ldb / ldc must be multiples of 8, operands 16-byte aligned, B below 2 GiB"
_BF16_SHAPE = "bsr_bf16: N/ldb/ldc must be multiples of 4 and operands vector-aligned"

ROWS = [
    # ---- mispmm_csr_f32: kernel id, mode, no-op shapes, row list, dense operands; a B of 2 GiB is taken (64-bit body)
    ("mispmm_csr_f32", dict(kernel=7), INV, "csr: unknown kernel id 7"),
    ("mispmm_csr_f32", dict(kernel=-1, M=0), INV, "csr: unknown kernel id -1"),
    ("mispmm_csr_f32", dict(acc=2), INV, "csr: unknown accumulate mode 2"),
    ("mispmm_csr_f32", dict(acc=2, M=0, N=0), INV, "csr: unknown accumulate mode 2"),
    ("mispmm_csr_f32", dict(M=0, rowPtrs=None, B=None, C=None, ldb=1), OK, None),
    ("mispmm_csr_f32", dict(N=0, rowPtrs=None, B=None, C=None), OK, None),
    ("mispmm_csr_f32", dict(rowPtrs=None), INV, "csr: rowPtrs is null"),
    ("mispmm_csr_f32", dict(colIdxs=None), INV, "csr: colIdxs or vals is null"),
    ("mispmm_csr_f32", dict(vals=None), INV, "csr: colIdxs or vals is null"),
    ("mispmm_csr_f32", dict(nnz=0, colIdxs=None, vals=None, C=None), INV, "B or C is null"),
    ("mispmm_csr_f32", dict(B=None), INV, "B or C is null"),
    ("mispmm_csr_f32", dict(C=None), INV, "B or C is null"),
    ("mispmm_csr_f32", dict(ldb=7), INV, _LD),
    ("mispmm_csr_f32", dict(ldc=7), INV, "leading dimension smaller than N (N=8 ldb=8 ldc=7)"),
    ("mispmm_csr_f32", _all_wrong("mispmm_csr_f32"), INV, "csr: unknown kernel id 9"),
    ("mispmm_csr_f32", _all_wrong("mispmm_csr_f32", kernel=6), INV, "csr: unknown accumulate mode 5"),
    ("mispmm_csr_f32", _all_wrong("mispmm_csr_f32", kernel=6, acc=1), INV, "csr: rowPtrs is null"),

    # ---- mispmm_csr_uniform_f32
    ("mispmm_csr_uniform_f32", dict(acc=2), INV, "csr_uniform: unknown accumulate mode 2"),
    ("mispmm_csr_uniform_f32", dict(acc=2, M=0), INV, "csr_uniform: unknown accumulate mode 2"),
    ("mispmm_csr_uniform_f32", dict(M=0, colIdxs=None, B=None), OK, None),
    ("mispmm_csr_uniform_f32", dict(N=0, colIdxs=None, B=None), OK, None),
    ("mispmm_csr_uniform_f32", dict(colIdxs=None), INV, "csr_uniform: colIdxs or vals is null"),
    ("mispmm_csr_uniform_f32", dict(vals=None), INV, "csr_uniform: colIdxs or vals is null"),
    ("mispmm_csr_uniform_f32", dict(M=1 << 20, rowNnz=1 << 13), INV, "csr_uniform: more than 2^32 entries"),
    ("mispmm_csr_uniform_f32", dict(rowNnz=0, colIdxs=None, vals=None, B=None), INV, "B or C is null"),
    ("mispmm_csr_uniform_f32", dict(B=None), INV, "B or C is null"),
    ("mispmm_csr_uniform_f32", dict(C=None), INV, "B or C is null"),
    ("mispmm_csr_uniform_f32", dict(ldb=7), INV, _LD),
    ("mispmm_csr_uniform_f32", dict(BIG), UNS, "csr_uniform: B of 2 GiB or more: use mispmm_csr_f32"),
    ("mispmm_csr_uniform_f32", _all_wrong("mispmm_csr_uniform_f32"), INV, "csr_uniform: unknown accumulate mode 5"),
    ("mispmm_csr_uniform_f32", _all_wrong("mispmm_csr_uniform_f32", acc=0), INV, "csr_uniform: colIdxs or vals is null"),

    # ---- mispmm_csr_split_f32
    ("mispmm_csr_split_f32", dict(acc=2), INV, "csr_split: unknown accumulate mode 2"),
    ("mispmm_csr_split_f32", dict(acc=2, N=0), INV, "csr_split: unknown accumulate mode 2"),
    ("mispmm_csr_split_f32", dict(M=0, rowPtrs=None, spans=None), OK, None),
    ("mispmm_csr_split_f32", dict(N=0, rowPtrs=None, spans=None), OK, None),
    ("mispmm_csr_split_f32", dict(rowPtrs=None, spans=None), INV, "csr_split: rowPtrs and spans are both null"),
    ("mispmm_csr_split_f32", dict(spans=P8), INV, "csr_split: spans must be 16-byte aligned"),
    ("mispmm_csr_split_f32", dict(numSpans=3), INV, "csr_split: 3 spans cannot describe 4 rows (M + 3 per shared row)"),
    ("mispmm_csr_split_f32", dict(numSpans=5), INV, "csr_split: 5 spans cannot describe 4 rows (M + 3 per shared row)"),
    ("mispmm_csr_split_f32", dict(colIdxs=None), INV, "csr_split: colIdxs or vals is null"),
    ("mispmm_csr_split_f32", dict(spans=None, numSpans=99, B=None), INV, "B or C is null"),     # rows in order: numSpans ignored
    ("mispmm_csr_split_f32", dict(rowPtrs=None, numSpans=7, C=None), INV, "B or C is null"),    # spans alone will do
    ("mispmm_csr_split_f32", dict(ldb=7), INV, _LD),
    ("mispmm_csr_split_f32", dict(BIG), UNS, "csr_split: B of 2 GiB or more: use mispmm_csr_f32"),
    ("mispmm_csr_split_f32", dict(N=6, ldb=6, ldc=6), UNS,
     "csr_split: B and C rows must be 16-byte vectors (N, ldb, ldc multiples of 4, aligned): use mispmm_csr_f32"),
    ("mispmm_csr_split_f32", dict(B=P8), UNS,
     "csr_split: B and C rows must be 16-byte vectors (N, ldb, ldc multiples of 4, aligned): use mispmm_csr_f32"),
    ("mispmm_csr_split_f32", _all_wrong("mispmm_csr_split_f32"), INV, "csr_split: unknown accumulate mode 5"),
    ("mispmm_csr_split_f32", _all_wrong("mispmm_csr_split_f32", acc=1), INV, "csr_split: rowPtrs and spans are both null"),

    # ---- mispmm_csr_hybrid_f32: the shape refusals carry no message
    ("mispmm_csr_hybrid_f32", dict(acc=2), INV, "csr_hybrid: unknown accumulate mode 2"),
    ("mispmm_csr_hybrid_f32", dict(acc=2, M=0), INV, "csr_hybrid: unknown accumulate mode 2"),
    ("mispmm_csr_hybrid_f32", dict(M=0, spans=None), OK, None),
    ("mispmm_csr_hybrid_f32", dict(N=0, spans=None), OK, None),
    ("mispmm_csr_hybrid_f32", dict(spans=None), INV, "csr_hybrid: spans must be a 16-byte aligned device array"),
    ("mispmm_csr_hybrid_f32", dict(spans=P8), INV, "csr_hybrid: spans must be a 16-byte aligned device array"),
    ("mispmm_csr_hybrid_f32", dict(numSpans=3), INV, "csr_hybrid: 3 spans cannot describe 4 rows (M + 3 per shared row)"),
    ("mispmm_csr_hybrid_f32", dict(numSpans=6), INV, "csr_hybrid: 6 spans cannot describe 4 rows (M + 3 per shared row)"),
    ("mispmm_csr_hybrid_f32", dict(numLongSpans=5), INV, "csr_hybrid: 5 long spans: a multiple of 4 that covers the 0 chunk groups is needed"),
    ("mispmm_csr_hybrid_f32", dict(numLongSpans=2), INV, "csr_hybrid: 2 long spans: a multiple of 4 that covers the 0 chunk groups is needed"),
    ("mispmm_csr_hybrid_f32", dict(numSpans=7, numLongSpans=0), INV,
     "csr_hybrid: 0 long spans: a multiple of 4 that covers the 1 chunk groups is needed"),
    ("mispmm_csr_hybrid_f32", dict(colIdxs=None), INV, "csr_hybrid: colIdxs or vals is null"),
    ("mispmm_csr_hybrid_f32", dict(B=None), INV, "B or C is null"),
    ("mispmm_csr_hybrid_f32", dict(ldb=7), INV, _LD),
    ("mispmm_csr_hybrid_f32", dict(BIG), UNS, NOMSG),
    ("mispmm_csr_hybrid_f32", dict(N=6, ldb=6, ldc=6), UNS, NOMSG),
    ("mispmm_csr_hybrid_f32", _all_wrong("mispmm_csr_hybrid_f32"), INV, "csr_hybrid: unknown accumulate mode 5"),
    ("mispmm_csr_hybrid_f32", _all_wrong("mispmm_csr_hybrid_f32", acc=1), INV, "csr_hybrid: spans must be a 16-byte aligned device array"),

    # ---- mispmm_csr_batch_f32: shapes without a batched kernel go out one launch each, so nothing else is refused here
    ("mispmm_csr_batch_f32", dict(acc=2), INV, "csr_batch: unknown accumulate mode 2"),
    ("mispmm_csr_batch_f32", dict(acc=2, batch=0), INV, "csr_batch: unknown accumulate mode 2"),
    ("mispmm_csr_batch_f32", dict(batch=0, B_list=None, rowPtrs=None), OK, None),
    ("mispmm_csr_batch_f32", dict(M=0, B_list=None, rowPtrs=None), OK, None),
    ("mispmm_csr_batch_f32", dict(N=0, B_list=None, rowPtrs=None), OK, None),
    ("mispmm_csr_batch_f32", dict(B_list=None), INV, "csr_batch: null operand list"),
    ("mispmm_csr_batch_f32", dict(C_list=None), INV, "csr_batch: null operand list"),
    ("mispmm_csr_batch_f32", dict(rowPtrs=None), INV, "csr_batch: rowPtrs is null"),
    ("mispmm_csr_batch_f32", dict(colIdxs=None), INV, "csr_batch: colIdxs or vals is null"),
    ("mispmm_csr_batch_f32", dict(B_list=NULLS), INV, "B or C is null"),
    ("mispmm_csr_batch_f32", dict(C_list=NULLS), INV, "B or C is null"),
    ("mispmm_csr_batch_f32", dict(ldb=7), INV, _LD),
    ("mispmm_csr_batch_f32", dict(rowPtrs=None, uniformRowNnz=3, ldc=7), INV, "leading dimension smaller than N (N=8 ldb=8 ldc=7)"),
    ("mispmm_csr_batch_f32", _all_wrong("mispmm_csr_batch_f32"), INV, "csr_batch: unknown accumulate mode 5"),
    ("mispmm_csr_batch_f32", _all_wrong("mispmm_csr_batch_f32", acc=0), INV, "csr_batch: null operand list"),

    # ---- mispmm_csr_plan_f32
    ("mispmm_csr_plan_f32", dict(acc=2), INV, "csr_plan: unknown accumulate mode 2"),
    ("mispmm_csr_plan_f32", dict(acc=2, batch=0), INV, "csr_plan: unknown accumulate mode 2"),
    ("mispmm_csr_plan_f32", dict(batch=0, B_list=None, rowPtrs=None), OK, None),
    ("mispmm_csr_plan_f32", dict(M=0, B_list=None, rowPtrs=None), OK, None),
    ("mispmm_csr_plan_f32", dict(N=0, B_list=None, rowPtrs=None), OK, None),
    ("mispmm_csr_plan_f32", dict(B_list=None), INV, "csr_plan: null operand list"),
    ("mispmm_csr_plan_f32", dict(C_list=None), INV, "csr_plan: null operand list"),
    ("mispmm_csr_plan_f32", dict(rowPtrs=None), INV, "csr_plan: rowPtrs is null"),
    ("mispmm_csr_plan_f32", dict(vals=None), INV, "csr_plan: colIdxs or vals is null"),
    ("mispmm_csr_plan_f32", dict(B_list=NULLS), INV, "B or C is null"),
    ("mispmm_csr_plan_f32", dict(ldb=7), INV, _LD),
    ("mispmm_csr_plan_f32", dict(BIG), UNS, "csr_plan: B of 2 GiB or more: multiply from the unpermuted arrays (mispmm_csr_f32)"),
    ("mispmm_csr_plan_f32", dict(rowMap=P, N=6, ldb=6, ldc=6), UNS, _PLAN_MAP),
    ("mispmm_csr_plan_f32", dict(rowMap=P, nnz=200), UNS, _PLAN_MAP),
    ("mispmm_csr_plan_f32", dict(rowMap=P, N=16, ldb=16, ldc=16), UNS, _PLAN_MAP),
    ("mispmm_csr_plan_f32", _all_wrong("mispmm_csr_plan_f32"), INV, "csr_plan: unknown accumulate mode 5"),
    ("mispmm_csr_plan_f32", _all_wrong("mispmm_csr_plan_f32", acc=0), INV, "csr_plan: null operand list"),

    # ---- mispmm_csr_lds_tile_f32
    ("mispmm_csr_lds_tile_f32", dict(acc=2), INV, "csr_lds_tile: unknown accumulate mode 2"),
    ("mispmm_csr_lds_tile_f32", dict(acc=2, numTiles=0), INV, "csr_lds_tile: unknown accumulate mode 2"),
    ("mispmm_csr_lds_tile_f32", dict(M=0, slots=None), OK, None),
    ("mispmm_csr_lds_tile_f32", dict(N=0, slots=None), OK, None),
    ("mispmm_csr_lds_tile_f32", dict(numTiles=0, slots=None), OK, None),
    ("mispmm_csr_lds_tile_f32", dict(tileRowPtrs=None), INV, "csr_lds_tile: null pointer"),
    ("mispmm_csr_lds_tile_f32", dict(tileColPtrs=None), INV, "csr_lds_tile: null pointer"),
    ("mispmm_csr_lds_tile_f32", dict(tileCols=None), INV, "csr_lds_tile: null pointer"),
    ("mispmm_csr_lds_tile_f32", dict(slots=None), INV, "csr_lds_tile: null pointer"),
    ("mispmm_csr_lds_tile_f32", dict(vals=None), INV, "csr_lds_tile: null pointer"),
    ("mispmm_csr_lds_tile_f32", dict(rowMap=None), INV, "csr_lds_tile: null pointer"),
    ("mispmm_csr_lds_tile_f32", dict(B=None), INV, "B or C is null"),
    ("mispmm_csr_lds_tile_f32", dict(ldb=63), INV, "leading dimension smaller than N (N=64 ldb=63 ldc=64)"),
    ("mispmm_csr_lds_tile_f32", dict(rowNnz=0), UNS, "csr_lds_tile: rows of one width of 1..16 entries (got 0)"),
    ("mispmm_csr_lds_tile_f32", dict(rowNnz=17), UNS, "csr_lds_tile: rows of one width of 1..16 entries (got 17)"),
    ("mispmm_csr_lds_tile_f32", dict(maxTileCols=129), UNS, "csr_lds_tile: a tile lists 129 columns, the LDS image holds 128"),
    ("mispmm_csr_lds_tile_f32", dict(N=8, ldb=8, ldc=8), UNS, _TILE_SHAPE),
    ("mispmm_csr_lds_tile_f32", dict(N=62, ldb=62, ldc=62), UNS, _TILE_SHAPE),
    ("mispmm_csr_lds_tile_f32", dict(BIG), UNS, _TILE_SHAPE),
    ("mispmm_csr_lds_tile_f32", dict(M=1 << 20, ldc=1 << 10), UNS, _TILE_SHAPE),
    ("mispmm_csr_lds_tile_f32", _all_wrong("mispmm_csr_lds_tile_f32"), INV, "csr_lds_tile: unknown accumulate mode 5"),
    ("mispmm_csr_lds_tile_f32", _all_wrong("mispmm_csr_lds_tile_f32", acc=1, rowNnz=0), INV, "csr_lds_tile: null pointer"),

    # ---- mispmm_csr_panel_f32: rowPtrs is not read
    ("mispmm_csr_panel_f32", dict(acc=2), INV, "csr_panel: unknown accumulate mode 2"),
    ("mispmm_csr_panel_f32", dict(acc=2, M=0), INV, "csr_panel: unknown accumulate mode 2"),
    ("mispmm_csr_panel_f32", dict(M=0, panelPtrs=None), OK, None),
    ("mispmm_csr_panel_f32", dict(N=0, panelPtrs=None), OK, None),
    ("mispmm_csr_panel_f32", dict(panelPtrs=None), INV, "csr_panel: null pointer"),
    ("mispmm_csr_panel_f32", dict(colIdxs=None), INV, "csr_panel: null pointer"),
    ("mispmm_csr_panel_f32", dict(vals=None), INV, "csr_panel: null pointer"),
    ("mispmm_csr_panel_f32", dict(rowPtrs=None, nnz=0, colIdxs=None, vals=None, B=None), INV, "B or C is null"),
    ("mispmm_csr_panel_f32", dict(ldb=7), INV, _LD),
    ("mispmm_csr_panel_f32", dict(panelRows=32), UNS, "csr_panel: panels of 64 or 128 B rows (got 32; build them with mispmm_csr_panel_rows())"),
    ("mispmm_csr_panel_f32", dict(N=6, ldb=6, ldc=6), UNS, _PANEL_SHAPE),
    ("mispmm_csr_panel_f32", dict(BIG), UNS, _PANEL_SHAPE),
    ("mispmm_csr_panel_f32", dict(M=1 << 20, ldc=1 << 10), UNS, _PANEL_SHAPE),
    ("mispmm_csr_panel_f32", dict(nnz=1 << 29), UNS, _PANEL_SHAPE),
    ("mispmm_csr_panel_f32", _all_wrong("mispmm_csr_panel_f32"), INV, "csr_panel: unknown accumulate mode 5"),
    ("mispmm_csr_panel_f32", _all_wrong("mispmm_csr_panel_f32", acc=1, panelRows=3), INV, "csr_panel: null pointer"),

    # ---- mispmm_coo_f32: a B of 2 GiB is taken (64-bit body)
    ("mispmm_coo_f32", dict(kernel=3), INV, "coo: unknown kernel id 3"),
    ("mispmm_coo_f32", dict(kernel=-2, M=0), INV, "coo: unknown kernel id -2"),
    ("mispmm_coo_f32", dict(acc=2), INV, "coo: unknown accumulate mode 2"),
    ("mispmm_coo_f32", dict(acc=2, N=0), INV, "coo: unknown accumulate mode 2"),
    ("mispmm_coo_f32", dict(M=0, rowIdxs=None, B=None), OK, None),
    ("mispmm_coo_f32", dict(N=0, rowIdxs=None, B=None), OK, None),
    ("mispmm_coo_f32", dict(rowIdxs=None), INV, "coo: null index or value array"),
    ("mispmm_coo_f32", dict(colIdxs=None), INV, "coo: null index or value array"),
    ("mispmm_coo_f32", dict(vals=None), INV, "coo: null index or value array"),
    ("mispmm_coo_f32", dict(nnz=0, rowIdxs=None, colIdxs=None, vals=None, B=None), INV, "B or C is null"),
    ("mispmm_coo_f32", dict(C=None), INV, "B or C is null"),
    ("mispmm_coo_f32", dict(ldb=7), INV, _LD),
    ("mispmm_coo_f32", dict(kernel=2, workspace=None), INV, "coo: kernel 2 needs the prepared row boundaries"),
    ("mispmm_coo_f32", _all_wrong("mispmm_coo_f32"), INV, "coo: unknown kernel id 9"),
    ("mispmm_coo_f32", _all_wrong("mispmm_coo_f32", kernel=2), INV, "coo: unknown accumulate mode 5"),
    ("mispmm_coo_f32", _all_wrong("mispmm_coo_f32", kernel=2, acc=0), INV, "coo: null index or value array"),

    # ---- mispmm_rows_split_f32
    ("mispmm_rows_split_f32", dict(acc=2), INV, "rows_split: unknown accumulate mode 2"),
    ("mispmm_rows_split_f32", dict(acc=2, M=0), INV, "rows_split: unknown accumulate mode 2"),
    ("mispmm_rows_split_f32", dict(M=0, spans=None), OK, None),
    ("mispmm_rows_split_f32", dict(N=0, spans=None), OK, None),
    ("mispmm_rows_split_f32", dict(spans=None), INV, "rows_split: spans is null or not 16-byte aligned"),
    ("mispmm_rows_split_f32", dict(spans=P8), INV, "rows_split: spans is null or not 16-byte aligned"),
    ("mispmm_rows_split_f32", dict(numSpans=5), INV, "rows_split: 5 spans for 4 rows (one per row: share_len = 0xFFFFFFFF)"),
    ("mispmm_rows_split_f32", dict(colIdxs=None), INV, "rows_split: colIdxs or vals is null"),
    ("mispmm_rows_split_f32", dict(vals=None), INV, "rows_split: colIdxs or vals is null"),
    ("mispmm_rows_split_f32", dict(B=None), INV, "B or C is null"),
    ("mispmm_rows_split_f32", dict(ldb=7), INV, _LD),
    ("mispmm_rows_split_f32", dict(BIG), UNS, "rows_split: B of 2 GiB or more"),
    ("mispmm_rows_split_f32", dict(N=6, ldb=6, ldc=6), UNS, "rows_split: B and C rows must be 16-byte vectors"),
    ("mispmm_rows_split_f32", _all_wrong("mispmm_rows_split_f32"), INV, "rows_split: unknown accumulate mode 5"),
    ("mispmm_rows_split_f32", _all_wrong("mispmm_rows_split_f32", acc=1), INV, "rows_split: spans is null or not 16-byte aligned"),

    # ---- mispmm_rows_hybrid_f32: the shape refusals carry no message
    ("mispmm_rows_hybrid_f32", dict(acc=2), INV, "rows_hybrid: unknown accumulate mode 2"),
    ("mispmm_rows_hybrid_f32", dict(acc=2, M=0), INV, "rows_hybrid: unknown accumulate mode 2"),
    ("mispmm_rows_hybrid_f32", dict(M=0, spans=None), OK, None),
    ("mispmm_rows_hybrid_f32", dict(N=0, spans=None), OK, None),
    ("mispmm_rows_hybrid_f32", dict(spans=None), INV, "rows_hybrid: spans is null or not 16-byte aligned"),
    ("mispmm_rows_hybrid_f32", dict(spans=P8), INV, "rows_hybrid: spans is null or not 16-byte aligned"),
    ("mispmm_rows_hybrid_f32", dict(numSpans=5), INV, "rows_hybrid: 5 spans for 4 rows (one per row: share_len = 0xFFFFFFFF)"),
    ("mispmm_rows_hybrid_f32", dict(numLongSpans=5), INV, "rows_hybrid: 5 long spans of 4: a multiple of 4 is needed"),
    ("mispmm_rows_hybrid_f32", dict(numLongSpans=2), INV, "rows_hybrid: 2 long spans of 4: a multiple of 4 is needed"),
    ("mispmm_rows_hybrid_f32", dict(colIdxs=None), INV, "rows_hybrid: colIdxs or vals is null"),
    ("mispmm_rows_hybrid_f32", dict(B=None), INV, "B or C is null"),
    ("mispmm_rows_hybrid_f32", dict(ldb=7), INV, _LD),
    ("mispmm_rows_hybrid_f32", dict(BIG), UNS, NOMSG),
    ("mispmm_rows_hybrid_f32", dict(N=6, ldb=6, ldc=6), UNS, NOMSG),
    ("mispmm_rows_hybrid_f32", _all_wrong("mispmm_rows_hybrid_f32"), INV, "rows_hybrid: unknown accumulate mode 5"),
    ("mispmm_rows_hybrid_f32", _all_wrong("mispmm_rows_hybrid_f32", acc=1), INV, "rows_hybrid: spans is null or not 16-byte aligned"),

    # ---- mispmm_ell_f32: a B of 2 GiB is taken (64-bit body)
    ("mispmm_ell_f32", dict(kernel=2), INV, "ell: unknown kernel id 2"),
    ("mispmm_ell_f32", dict(kernel=-1, M=0), INV, "ell: unknown kernel id -1"),
    ("mispmm_ell_f32", dict(acc=2), INV, "ell: unknown accumulate mode 2"),
    ("mispmm_ell_f32", dict(acc=2, N=0), INV, "ell: unknown accumulate mode 2"),
    ("mispmm_ell_f32", dict(M=0, colIdxs=None, B=None), OK, None),
    ("mispmm_ell_f32", dict(N=0, colIdxs=None, B=None), OK, None),
    ("mispmm_ell_f32", dict(colIdxs=None), INV, "ell: colIdxs or vals is null"),
    ("mispmm_ell_f32", dict(vals=None), INV, "ell: colIdxs or vals is null"),
    ("mispmm_ell_f32", dict(width=0, colIdxs=None, vals=None, B=None), INV, "B or C is null"),
    ("mispmm_ell_f32", dict(C=None), INV, "B or C is null"),
    ("mispmm_ell_f32", dict(ldb=7), INV, _LD),
    ("mispmm_ell_f32", _all_wrong("mispmm_ell_f32"), INV, "ell: unknown kernel id 9"),
    ("mispmm_ell_f32", _all_wrong("mispmm_ell_f32", kernel=1), INV, "ell: unknown accumulate mode 5"),
    ("mispmm_ell_f32", _all_wrong("mispmm_ell_f32", kernel=1, acc=1), INV, "ell: colIdxs or vals is null"),

    # ---- mispmm_bsr_f32
    ("mispmm_bsr_f32", dict(kernel=3), INV, "bsr: unknown kernel id 3"),
    ("mispmm_bsr_f32", dict(acc=2), INV, "bsr: unknown accumulate mode 2"),
    ("mispmm_bsr_f32", dict(acc=2, Mb=0), INV, "bsr: unknown accumulate mode 2"),
    ("mispmm_bsr_f32", dict(bR=0), INV, "bsr: zero block dimension"),
    ("mispmm_bsr_f32", dict(bC=0, Mb=0), INV, "bsr: zero block dimension"),
    ("mispmm_bsr_f32", dict(Mb=0, ptrs=None, B=None), OK, None),
    ("mispmm_bsr_f32", dict(N=0, ptrs=None, B=None), OK, None),
    ("mispmm_bsr_f32", dict(ptrs=None), INV, "bsr: blockRowPtrs is null"),
    ("mispmm_bsr_f32", dict(idxs=None), INV, "bsr: null block arrays"),
    ("mispmm_bsr_f32", dict(blocks=None), INV, "bsr: null block arrays"),
    ("mispmm_bsr_f32", dict(numBlocks=0, idxs=None, blocks=None, B=None), INV, "B or C is null"),
    ("mispmm_bsr_f32", dict(C=None), INV, "B or C is null"),
    ("mispmm_bsr_f32", dict(ldb=7), INV, _LD),
    ("mispmm_bsr_f32", dict(kernel=2, acc=1), UNS, "bsr: MFMA kernel needs 16x16 blocks, N/ldb/ldc multiples of 4, 16-byte aligned operands"),
    ("mispmm_bsr_f32", dict(kernel=2, acc=1, bR=16, bC=16, K=16, N=6, ldb=6, ldc=6), UNS,
     "bsr: MFMA kernel needs 16x16 blocks, N/ldb/ldc multiples of 4, 16-byte aligned operands"),
    ("mispmm_bsr_f32", dict(kernel=2, acc=1, bR=16, bC=16, **BIG), UNS,
     "bsr: MFMA kernel needs 16x16 blocks, N/ldb/ldc multiples of 4, 16-byte aligned operands"),
    ("mispmm_bsr_f32", dict(kernel=2, acc=0, bR=16, bC=16, K=16), UNS, "bsr: the MFMA kernel has FAST (fused) numerics only"),
    ("mispmm_bsr_f32", _all_wrong("mispmm_bsr_f32", bR=0), INV, "bsr: unknown kernel id 9"),
    ("mispmm_bsr_f32", _all_wrong("mispmm_bsr_f32", bR=0, kernel=2), INV, "bsr: unknown accumulate mode 5"),
    ("mispmm_bsr_f32", _all_wrong("mispmm_bsr_f32", bR=0, kernel=2, acc=0), INV, "bsr: zero block dimension"),
    ("mispmm_bsr_f32", _all_wrong("mispmm_bsr_f32", kernel=2, acc=0), INV, "bsr: blockRowPtrs is null"),

    # ---- mispmm_bsr_bf16: no mode; the block shape is looked at before the no-op shapes
    ("mispmm_bsr_bf16", dict(bR=8, bC=8), UNS, "bsr_bf16: only 16x16 or 32x32 blocks (got 8x8)"),
    ("mispmm_bsr_bf16", dict(bC=32, Mb=0), UNS, "bsr_bf16: only 16x16 or 32x32 blocks (got 16x32)"),
    ("mispmm_bsr_bf16", dict(Mb=0, ptrs=None), OK, None),
    ("mispmm_bsr_bf16", dict(N=0, ptrs=None, bR=32, bC=32), OK, None),
    ("mispmm_bsr_bf16", dict(ptrs=None), INV, "bsr_bf16: null pointer"),
    ("mispmm_bsr_bf16", dict(B=None), INV, "bsr_bf16: null pointer"),
    ("mispmm_bsr_bf16", dict(C=None), INV, "bsr_bf16: null pointer"),
    ("mispmm_bsr_bf16", dict(idxs=None), INV, "bsr_bf16: null block arrays"),
    ("mispmm_bsr_bf16", dict(blocks=None), INV, "bsr_bf16: null block arrays"),
    ("mispmm_bsr_bf16", dict(ldb=7), INV, "bsr_bf16: leading dimension smaller than N"),
    ("mispmm_bsr_bf16", dict(ldc=7), INV, "bsr_bf16: leading dimension smaller than N"),
    ("mispmm_bsr_bf16", dict(N=6, ldb=6, ldc=6), UNS, _BF16_SHAPE),
    ("mispmm_bsr_bf16", dict(K=1 << 21, ldb=1 << 10), UNS, _BF16_SHAPE),
    ("mispmm_bsr_bf16", dict(C=P8), UNS, _BF16_SHAPE),
    ("mispmm_bsr_bf16", dict(blocks=P8), UNS, _BF16_SHAPE),
    ("mispmm_bsr_bf16", _all_wrong("mispmm_bsr_bf16", bR=3), UNS, "bsr_bf16: only 16x16 or 32x32 blocks (got 3x16)"),
    ("mispmm_bsr_bf16", _all_wrong("mispmm_bsr_bf16"), INV, "bsr_bf16: null pointer"),

    # ---- mispmm_bsrc_bf16
    ("mispmm_bsrc_bf16", dict(Mb=0, stepPtrs=None), OK, None),
    ("mispmm_bsrc_bf16", dict(N=0, stepPtrs=None), OK, None),
    ("mispmm_bsrc_bf16", dict(stepPtrs=None), INV, "bsrc_bf16: null pointer"),
    ("mispmm_bsrc_bf16", dict(B=None), INV, "bsrc_bf16: null pointer"),
    ("mispmm_bsrc_bf16", dict(C=None), INV, "bsrc_bf16: null pointer"),
    ("mispmm_bsrc_bf16", dict(cols=None), INV, "bsrc_bf16: null step arrays"),
    ("mispmm_bsrc_bf16", dict(tiles=None), INV, "bsrc_bf16: null step arrays"),
    ("mispmm_bsrc_bf16", dict(nSteps=0, cols=None, tiles=None, ldb=7), INV, "bsrc_bf16: leading dimension smaller than N"),
    ("mispmm_bsrc_bf16", dict(ldc=7), INV, "bsrc_bf16: leading dimension smaller than N"),
    ("mispmm_bsrc_bf16", dict(N=4, ldb=4, ldc=4), UNS, _BSRC),
    ("mispmm_bsrc_bf16", dict(ldb=12), UNS, _BSRC),
    ("mispmm_bsrc_bf16", dict(cols=P8), UNS, _BSRC),
    ("mispmm_bsrc_bf16", dict(K=1 << 21, ldb=1 << 10), UNS, _BSRC),
    ("mispmm_bsrc_bf16", _all_wrong("mispmm_bsrc_bf16"), INV, "bsrc_bf16: null pointer"),

    # ---- mispmm_bsrc_slots_bf16
    ("mispmm_bsrc_slots_bf16", dict(Mb=0, extraPtrs=None), OK, None),
    ("mispmm_bsrc_slots_bf16", dict(N=0, extraPtrs=None), OK, None),
    ("mispmm_bsrc_slots_bf16", dict(extraPtrs=None), INV, "bsrc_slots_bf16: null pointer"),
    ("mispmm_bsrc_slots_bf16", dict(cols=None), INV, "bsrc_slots_bf16: null pointer"),
    ("mispmm_bsrc_slots_bf16", dict(tiles=None), INV, "bsrc_slots_bf16: null pointer"),
    ("mispmm_bsrc_slots_bf16", dict(B=None), INV, "bsrc_slots_bf16: null pointer"),
    ("mispmm_bsrc_slots_bf16", dict(C=None), INV, "bsrc_slots_bf16: null pointer"),
    ("mispmm_bsrc_slots_bf16", dict(nSteps=7), INV, "bsrc_slots_bf16: nSteps 7 is less than 4 slots per block row"),
    ("mispmm_bsrc_slots_bf16", dict(Mb=1 << 29, nSteps=1 << 31, N=1024, ldb=1024, ldc=1024), UNS,
     "bsrc_slots_bf16: 536870912 block rows x 1024 columns exceed the grid of this kernel"),
    ("mispmm_bsrc_slots_bf16", dict(ldb=7), INV, "bsrc_slots_bf16: leading dimension smaller than N"),
    ("mispmm_bsrc_slots_bf16", dict(N=4, ldb=4, ldc=4), UNS, _SLOTS),
    ("mispmm_bsrc_slots_bf16", dict(tiles=P8), UNS, _SLOTS),
    ("mispmm_bsrc_slots_bf16", dict(K=1 << 21, ldb=1 << 10), UNS, _SLOTS),
    ("mispmm_bsrc_slots_bf16", _all_wrong("mispmm_bsrc_slots_bf16", nSteps=0), INV, "bsrc_slots_bf16: null pointer"),

    # ---- mispmm_csr_f64: its own wording of the dense checks; a B or C of 2 GiB is taken (64-bit body)
    ("mispmm_csr_f64", dict(acc=2), INV, "csr_f64: unknown accumulate mode 2"),
    ("mispmm_csr_f64", dict(acc=2, M=0), INV, "csr_f64: unknown accumulate mode 2"),
    ("mispmm_csr_f64", dict(M=0, rowPtrs=None, B=None), OK, None),
    ("mispmm_csr_f64", dict(N=0, rowPtrs=None, B=None), OK, None),
    ("mispmm_csr_f64", dict(rowPtrs=None), INV, "csr_f64: rowPtrs is null"),
    ("mispmm_csr_f64", dict(colIdxs=None), INV, "csr_f64: colIdxs or vals is null"),
    ("mispmm_csr_f64", dict(vals=None), INV, "csr_f64: colIdxs or vals is null"),
    ("mispmm_csr_f64", dict(nnz=0, colIdxs=None, vals=None, B=None), INV, "csr_f64: B or C is null"),
    ("mispmm_csr_f64", dict(C=None), INV, "csr_f64: B or C is null"),
    ("mispmm_csr_f64", dict(ldb=7), INV, "csr_f64: leading dimension smaller than N (N=8 ldb=7 ldc=8)"),
    ("mispmm_csr_f64", dict(ldc=7), INV, "csr_f64: leading dimension smaller than N (N=8 ldb=8 ldc=7)"),
    ("mispmm_csr_f64", _all_wrong("mispmm_csr_f64"), INV, "csr_f64: unknown accumulate mode 5"),
    ("mispmm_csr_f64", _all_wrong("mispmm_csr_f64", acc=1), INV, "csr_f64: rowPtrs is null"),

    # ---- mispmm_sddmm_bsr_bf16: no mode; N == 0 with blocks to write is device work (a memset) and has no row
    ("mispmm_sddmm_bsr_bf16", dict(bS=8), UNS, "sddmm_bsr_bf16: only 16x16 or 32x32 blocks (got bS=8)"),
    ("mispmm_sddmm_bsr_bf16", dict(bS=0, Mb=0), UNS, "sddmm_bsr_bf16: only 16x16 or 32x32 blocks (got bS=0)"),
    ("mispmm_sddmm_bsr_bf16", dict(Mb=0, ptrs=None), OK, None),
    ("mispmm_sddmm_bsr_bf16", dict(numBlocks=0, N=0, ptrs=None, bS=32), OK, None),
    ("mispmm_sddmm_bsr_bf16", dict(ptrs=None), INV, "sddmm_bsr_bf16: blockRowPtrs, blockColIdxs or out is null"),
    ("mispmm_sddmm_bsr_bf16", dict(idxs=None), INV, "sddmm_bsr_bf16: blockRowPtrs, blockColIdxs or out is null"),
    ("mispmm_sddmm_bsr_bf16", dict(out=None), INV, "sddmm_bsr_bf16: blockRowPtrs, blockColIdxs or out is null"),
    ("mispmm_sddmm_bsr_bf16", dict(ldx=7), INV, "sddmm_bsr_bf16: leading dimension smaller than N (N=8 ldx=7 ldy=8)"),
    ("mispmm_sddmm_bsr_bf16", dict(ldy=7), INV, "sddmm_bsr_bf16: leading dimension smaller than N (N=8 ldx=8 ldy=7)"),
    ("mispmm_sddmm_bsr_bf16", dict(K=20), INV, "sddmm_bsr_bf16: K=20 is not a multiple of the block size 16"),
    ("mispmm_sddmm_bsr_bf16", dict(K=20, N=0), INV, "sddmm_bsr_bf16: K=20 is not a multiple of the block size 16"),
    ("mispmm_sddmm_bsr_bf16", dict(X=None), INV, "sddmm_bsr_bf16: X or Y is null"),
    ("mispmm_sddmm_bsr_bf16", dict(Y=None), INV, "sddmm_bsr_bf16: X or Y is null"),
    ("mispmm_sddmm_bsr_bf16", dict(Mb=1 << 20, ldx=128), UNS,
     "sddmm_bsr_bf16: X or Y spans 2 GiB or more (rows=16777216 ldx=128 K=32 ldy=8)"),
    ("mispmm_sddmm_bsr_bf16", dict(K=1 << 24, ldy=128), UNS, "sddmm_bsr_bf16: X or Y spans 2 GiB or more (rows=32 ldx=8 K=16777216 ldy=128)"),
    ("mispmm_sddmm_bsr_bf16", _all_wrong("mispmm_sddmm_bsr_bf16", bS=5), UNS, "sddmm_bsr_bf16: only 16x16 or 32x32 blocks (got bS=5)"),
    ("mispmm_sddmm_bsr_bf16", _all_wrong("mispmm_sddmm_bsr_bf16", K=20), INV, "sddmm_bsr_bf16: blockRowPtrs, blockColIdxs or out is null"),

    # ---- mispmm_softmax_bsr_f32 / _bwd_f32: scale, block size, no-op shapes, pointers (mask may be null); no size is declined
    ("mispmm_softmax_bsr_f32", dict(scale=0.0), INV, "softmax_bsr_f32: scale must be finite and > 0 (got 0)"),
    ("mispmm_softmax_bsr_f32", dict(scale=-1.0, Mb=0), INV, "softmax_bsr_f32: scale must be finite and > 0 (got -1)"),
    ("mispmm_softmax_bsr_f32", dict(scale=float("inf")), INV, "softmax_bsr_f32: scale must be finite and > 0 (got inf)"),
    ("mispmm_softmax_bsr_f32", dict(scale=float("nan")), INV, "softmax_bsr_f32: scale must be finite and > 0 (got nan)"),
    ("mispmm_softmax_bsr_f32", dict(bS=8), UNS, "softmax_bsr_f32: only 16x16 or 32x32 blocks (got bS=8)"),
    ("mispmm_softmax_bsr_f32", dict(bS=8, numBlocks=0), UNS, "softmax_bsr_f32: only 16x16 or 32x32 blocks (got bS=8)"),
    ("mispmm_softmax_bsr_f32", dict(Mb=0, ptrs=None), OK, None),
    ("mispmm_softmax_bsr_f32", dict(numBlocks=0, ptrs=None, bS=32), OK, None),
    ("mispmm_softmax_bsr_f32", dict(ptrs=None), INV, "softmax_bsr_f32: blockRowPtrs, scores or out is null"),
    ("mispmm_softmax_bsr_f32", dict(scores=None), INV, "softmax_bsr_f32: blockRowPtrs, scores or out is null"),
    ("mispmm_softmax_bsr_f32", dict(out=None, mask=None), INV, "softmax_bsr_f32: blockRowPtrs, scores or out is null"),
    ("mispmm_softmax_bsr_f32", _all_wrong("mispmm_softmax_bsr_f32", scale=0.0, bS=8), INV, "softmax_bsr_f32: scale must be finite and > 0 (got 0)"),
    ("mispmm_softmax_bsr_f32", _all_wrong("mispmm_softmax_bsr_f32", bS=8), UNS, "softmax_bsr_f32: only 16x16 or 32x32 blocks (got bS=8)"),
    ("mispmm_softmax_bsr_f32", _all_wrong("mispmm_softmax_bsr_f32"), INV, "softmax_bsr_f32: blockRowPtrs, scores or out is null"),
    ("mispmm_softmax_bsr_bwd_f32", dict(scale=0.0), INV, "softmax_bsr_bwd_f32: scale must be finite and > 0 (got 0)"),
    ("mispmm_softmax_bsr_bwd_f32", dict(scale=float("inf"), Mb=0), INV, "softmax_bsr_bwd_f32: scale must be finite and > 0 (got inf)"),
    ("mispmm_softmax_bsr_bwd_f32", dict(bS=64), UNS, "softmax_bsr_bwd_f32: only 16x16 or 32x32 blocks (got bS=64)"),
    ("mispmm_softmax_bsr_bwd_f32", dict(Mb=0, ptrs=None), OK, None),
    ("mispmm_softmax_bsr_bwd_f32", dict(numBlocks=0, ptrs=None), OK, None),
    ("mispmm_softmax_bsr_bwd_f32", dict(ptrs=None), INV, "softmax_bsr_bwd_f32: blockRowPtrs, p, dp or ds is null"),
    ("mispmm_softmax_bsr_bwd_f32", dict(p=None), INV, "softmax_bsr_bwd_f32: blockRowPtrs, p, dp or ds is null"),
    ("mispmm_softmax_bsr_bwd_f32", dict(dp=None), INV, "softmax_bsr_bwd_f32: blockRowPtrs, p, dp or ds is null"),
    ("mispmm_softmax_bsr_bwd_f32", dict(ds=None), INV, "softmax_bsr_bwd_f32: blockRowPtrs, p, dp or ds is null"),
    ("mispmm_softmax_bsr_bwd_f32", _all_wrong("mispmm_softmax_bsr_bwd_f32", scale=-2.0, bS=8), INV,
     "softmax_bsr_bwd_f32: scale must be finite and > 0 (got -2)"),
    ("mispmm_softmax_bsr_bwd_f32", _all_wrong("mispmm_softmax_bsr_bwd_f32"), INV, "softmax_bsr_bwd_f32: blockRowPtrs, p, dp or ds is null"),
]
ROWS += _row_list("mispmm_ell_compact_f32", "ell_compact", "ell_compact: B of 2 GiB or more: use mispmm_ell_f32")
ROWS += _row_list("mispmm_bsr_nonzeros_f32", "bsr_nonzeros", "bsr_nonzeros: B of 2 GiB or more: use mispmm_bsr_f32")
ROWS += _sddmm_csr("mispmm_sddmm_csr_f32") + _sddmm_csr("mispmm_sddmm_csr_f64")
ROWS += _softmax_csr("mispmm_softmax_csr_f32", "rowPtrs, scores or out") + _softmax_csr("mispmm_softmax_csr_f64", "rowPtrs, scores or out")
ROWS += _softmax_csr("mispmm_softmax_csr_bwd_f32", "rowPtrs, p, dp or ds") + _softmax_csr("mispmm_softmax_csr_bwd_f64", "rowPtrs, p, dp or ds")


def _call(entry, overrides):
    names, good = ENTRIES[entry]
    unknown = set(overrides) - set(good)
    assert not unknown, f"{entry}: no parameter named {sorted(unknown)}"
    args = dict(good, stream=None)
    args.update(overrides)
    return getattr(capi.lib(), entry)(*[args[n] for n in names.split()])


def test_every_compute_entry_point_has_rows():
    """every entry of the table is a symbol of the library, has a row for each kind of outcome, and no row is the good call"""
    covered = {r[0] for r in ROWS}
    assert covered == set(ENTRIES)
    for entry in ENTRIES:
        assert hasattr(capi.lib(), entry), entry
        statuses = {r[2] for r in ROWS if r[0] == entry}
        assert OK in statuses and (INV in statuses or UNS in statuses), entry
    assert all(r[1] for r in ROWS)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_rejections_and_noops(entry):
    l = capi.lib()
    for i, (name, overrides, status, text) in enumerate(ROWS):
        if name != entry:
            continue
        shown = {k: (v.value if isinstance(v, ctypes.c_void_p) else v) for k, v in overrides.items()
                 if not isinstance(v, ctypes.Array)}
        got = _call(entry, overrides)
        message = l.mispmm_last_error().decode()
        assert got == status, f"row {i} {entry}{shown}: status {got}, expected {status} ({message!r})"
        if status != OK and text is not NOMSG:
            assert message == text, f"row {i} {entry}{shown}"
