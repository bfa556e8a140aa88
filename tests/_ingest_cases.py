"""The corpus of the ingest tests: malformed sparse structures that every way in must refuse, and valid-but-unusual ones
that every way in must keep accepting (the validity contract of include/mispmm.h).  Everything is generated here; files are
written only where a test asks (write(), into its tmp_path).

A case is one matrix in one format, as TEXT (what `cuspmm` and the formats.read_* functions parse) and, where the defect
survives in memory, as a CONTAINER (what ops.*.from_host and the library's mispmm_*_check_host take).  A defect of the text
alone -- a token that is no number -- has no container (`mem is None`); a defect that uint32 arrays cannot hold as written has
the container a careless reader would have built: "-1" is 0xFFFFFFFF there, a negative or oversized header field a row count
that the arrays do not back.  `want` is the substring the refusal of the text must contain, `want_mem` that of the container.

Base matrix: 6 x 7, 11 entries, rows of 2, 0, 3, 1, 2, 3 entries; ELL width 3.  A 6 x 7 matrix has no 2- or 3-wide block
columns, so the BSR base is the same pattern on 6 x 6 (column 6 moved to 5), as 2 x 2 and as 2 x 3 blocks.

No GPU is involved anywhere in this module: malformed input never goes near one."""
import os

import numpy as np

from mispmm import formats

M, K, NNZ = 6, 7, 11
PTRS = [0, 2, 2, 5, 6, 8, 11]
COLS = [1, 4, 0, 3, 6, 2, 1, 5, 0, 4, 6]
VALS = [1.5, -2.25, 0.75, 3.0, -1.125, 2.5, -0.5, 4.0, 1.25, -3.5, 0.625]
ROWS = [r for r in range(M) for _ in range(PTRS[r + 1] - PTRS[r])]
COLS6 = [min(c, 5) for c in COLS]                      # the BSR base: 6 x 6
DENSE_N = 2                                            # columns of the dense.in beside every sparse file
U32 = 0xFFFFFFFF


def u32(xs):
    return (np.asarray(xs, dtype=np.int64) & U32).astype(np.uint32)


def f32(xs):
    return np.asarray(xs, dtype=np.float32)


def dense_b(k, n=DENSE_N):
    """A small exact operand: multiples of 1/8 of both signs."""
    return ((np.arange(k * n, dtype=np.float32).reshape(k, n) % 13) - 6) / 8


def _line(xs):
    return " ".join(x if isinstance(x, str) else repr(float(x)) if isinstance(x, float) else str(int(x)) for x in xs)


def dense_text(b):
    return f"{b.shape[0]} {b.shape[1]}\n" + "".join(_line([float(v) for v in row]) + "\n" for row in b)


def csr_text(m, k, nnz, ptrs, cols, vals):
    return f"{m} {k} {nnz}\n{_line(ptrs)}\n{_line(cols)}\n{_line([float(v) for v in vals])}\n"


def coo_text(m, k, nnz, rows, cols, vals):
    return f"{m} {k} {nnz}\n" + "".join(f"{_line([r])} {_line([c])} {_line([float(v)])}\n" for r, c, v in zip(rows, cols, vals))


def bsr_text(m, k, nnz, br, bc, nblocks, ptrs, idxs, blocks):
    return (f"{m} {k} {nnz} {br} {bc} {nblocks}\n{_line(ptrs)}\n{_line(idxs)}\n"
            + "".join(_line([float(v) for v in np.asarray(b).reshape(-1)]) + "\n" for b in blocks))


def ell_texts(m, k, nnz, width, idx, val):
    """(index file, values file) of either layout: one line per line of the 2-D arrays, 0xFFFFFFFF written as -1."""
    def tok(x):
        return x if isinstance(x, str) else str(-1 if int(x) == U32 else int(x))
    return (f"{m} {k} {nnz} {width}\n" + "".join(" ".join(tok(x) for x in line) + "\n" for line in idx),
            "".join(_line([float(v) for v in line]) + "\n" for line in val))


class Case:
    """fmt: csr | coo | ell_cm | ell_rm | bsr | dense.  files: name -> text of the directory `cuspmm -d` reads (a dense.in is
    added).  mem: the container or None.  cli: False where the command line does not read this format (row-major ELL)."""

    def __init__(self, name, fmt, files, mem=None, want=None, want_mem=None, b=None):
        self.name, self.fmt, self.files, self.mem, self.want, self.want_mem = name, fmt, dict(files), mem, want, want_mem or want
        self.cli = fmt != "ell_rm"
        if "dense.in" not in self.files:
            self.b = b if b is not None else dense_b(mem.num_cols if mem is not None else K)
            self.files["dense.in"] = dense_text(self.b)

    def write(self, directory):
        os.makedirs(directory, exist_ok=True)
        for name, text in self.files.items():
            with open(os.path.join(directory, name), "w") as f:
                f.write(text)
        return str(directory)

    def path(self, directory, suffix):
        return os.path.join(str(directory), next(n for n in self.files if n.endswith(suffix)))

    def __repr__(self):
        return self.name


CLI_FLAG = {"csr": "--csr", "coo": "--coo", "ell_cm": "--ell", "bsr": "--bsr", "dense": "--csr"}


def read(case, directory):
    """The formats.read_* call for the case's files in `directory`."""
    if case.fmt == "csr":
        return formats.read_csr(case.path(directory, ".csr"))
    if case.fmt == "coo":
        return formats.read_coo(case.path(directory, ".coo"))
    if case.fmt == "bsr":
        return formats.read_bsr(case.path(directory, ".bsr"))
    if case.fmt == "ell_cm":
        return formats.read_ell_colmajor(case.path(directory, "_rowind.ell"), case.path(directory, "_values_colmajor.ell"))
    if case.fmt == "ell_rm":
        return formats.read_ell_rowmajor(case.path(directory, "_colind.ell"), case.path(directory, "_values.ell"))
    return formats.read_dense(case.path(directory, "dense.in"))


NUMPY_CHECK = {"csr": formats.check_csr, "coo": formats.check_coo, "ell_cm": formats.check_ell, "ell_rm": formats.check_ell,
               "bsr": formats.check_bsr}


# ---------------------------------------------------------------------------------------------------------------- builders
def _csr(name, m=M, k=K, ptrs=PTRS, cols=COLS, vals=VALS, want=None, want_mem=None, tail=""):
    numeric = all(not isinstance(x, str) for x in list(ptrs) + list(cols))      # a token that is no number has no container
    box = formats.CSR(m & U32, k, u32(ptrs), u32(cols), f32(vals)) if numeric else None
    return Case(name, "csr", {"a.csr": csr_text(m, k, len(cols), ptrs, cols, vals) + tail}, box, want, want_mem)


def _coo(name, m=M, k=K, rows=ROWS, cols=COLS, vals=VALS, want=None, want_mem=None):
    return Case(name, "coo", {"a.coo": coo_text(m, k, len(vals), rows, cols, vals)},
                formats.COO(m, k, u32(rows), u32(cols), f32(vals)), want, want_mem)


def _base_csr(cols=COLS, k=K):
    return formats.CSR(M, k, u32(PTRS), u32(cols), f32(VALS))


def _ell_cm(name, idx=None, val=None, m=M, k=K, want=None):
    base = formats.csr_to_ell_colmajor(_base_csr(), reference_width=True)
    idx = base.row_idxs if idx is None else idx
    val = base.data if val is None else val
    w = idx.shape[1]
    i, v = ell_texts(m, k, NNZ, w, idx, val)
    return Case(name, "ell_cm", {"a_rowind.ell": i, "a_values_colmajor.ell": v}, formats.ELLColMajor(m, k, NNZ, w, idx, val), want)


def _ell_rm(name, idx=None, val=None, m=M, k=K, want=None):
    base = formats.csr_to_ell_rowmajor(_base_csr())
    idx = base.col_idxs if idx is None else idx
    val = base.data if val is None else val
    w = idx.shape[1]
    i, v = ell_texts(m, k, NNZ, w, idx, val)
    return Case(name, "ell_rm", {"a_colind.ell": i, "a_values.ell": v}, formats.ELLRowMajor(m, k, NNZ, w, idx, val), want)


def _bsr(name, br=2, bc=2, m=6, k=6, ptrs=None, idxs=None, blocks=None, want=None):
    base = formats.csr_to_bsr(_base_csr(COLS6, 6), 2, bc if bc else 2)
    ptrs = base.block_row_ptrs.tolist() if ptrs is None else ptrs
    idxs = base.block_col_idxs.tolist() if idxs is None else idxs
    blocks = base.data if blocks is None else blocks
    text = bsr_text(m, k, int(np.asarray(blocks).size), br, bc, len(idxs), ptrs, idxs, blocks)
    return Case(name, "bsr", {"a.bsr": text}, formats.BSR(m, k, int(np.asarray(blocks).size), br, bc, u32(ptrs), u32(idxs), f32(blocks)), want)


def _with(xs, at, value):
    out = list(xs)
    out[at] = value
    return out


def _dense(name, text, want):
    return Case(name, "dense", {"a.csr": csr_text(M, K, NNZ, PTRS, COLS, VALS), "dense.in": text}, None, want)


# ---------------------------------------------------------------------------------------------------------------- malformed
def malformed():
    cm = formats.csr_to_ell_colmajor(_base_csr(), reference_width=True).row_idxs
    rm = formats.csr_to_ell_rowmajor(_base_csr()).col_idxs
    cm_bad, rm_k, rm_fe = cm.copy(), rm.copy(), rm.copy()
    cm_bad[2, 0] = M                       # column 2 holds one entry, slot 0: flat position 2 * 3
    rm_k[2, 1] = K                         # row 2 holds three entries: flat position 2 * 3 + 1
    rm_fe[2, 1] = 0xFFFFFFFE
    b22 = formats.csr_to_bsr(_base_csr(COLS6, 6), 2, 2)
    p22 = b22.block_row_ptrs.tolist()
    good_b = dense_text(dense_b(K)).split("\n")
    return [
        _csr("csr-column-equals-K", cols=_with(COLS, 4, K), want="colIdxs[4] = 7 is not below K = 7"),
        _csr("csr-column-minus-one", cols=_with(COLS, 4, -1), want="colIdxs[4] = -1 is not an index",
             want_mem="colIdxs[4] = 4294967295 is not below K = 7"),
        _csr("csr-column-2^31", cols=_with(COLS, 4, 1 << 31), want="colIdxs[4] = 2147483648 is not below K = 7"),
        _csr("csr-row-pointers-decrease", ptrs=_with(PTRS, 2, 1), want="rowPtrs decrease at row 1 (2 then 1)"),
        _csr("csr-first-row-pointer-one", ptrs=_with(PTRS, 0, 1), want="rowPtrs[0] = 1, must be 0"),
        _csr("csr-last-row-pointer-nnz-plus-one", ptrs=_with(PTRS, M, NNZ + 1), want="rowPtrs[M = 6] = 12, nnz = 11"),
        _csr("csr-last-row-pointer-nnz-minus-one", ptrs=_with(PTRS, M, NNZ - 1), want="rowPtrs[M = 6] = 10, nnz = 11"),
        _csr("csr-token-is-no-number", cols=_with(COLS, 4, "x7"), want="colIdxs[4]: not a number: 'x7'"),
        _csr("csr-negative-header-field", m=-6, want="numRows = -6 is not a count",
             want_mem="rowPtrs holds 7 entries, M + 1 = 4294967291 are needed"),
        _csr("csr-header-larger-than-the-file", m=U32, want="header promises",
             want_mem="rowPtrs holds 7 entries, M + 1 = 4294967296 are needed"),
        _coo("coo-row-equals-M", rows=_with(ROWS, 3, M), want="rowIdxs[3] = 6 is not below M = 6"),
        _coo("coo-column-equals-K", cols=_with(COLS, 3, K), want="colIdxs[3] = 7 is not below K = 7"),
        _coo("coo-row-minus-one", rows=_with(ROWS, 3, -1), want="rowIdxs[3] = -1 is not an index",
             want_mem="rowIdxs[3] = 4294967295 is not below M = 6"),
        _coo("coo-column-minus-one", cols=_with(COLS, 3, -1), want="colIdxs[3] = -1 is not an index",
             want_mem="colIdxs[3] = 4294967295 is not below K = 7"),
        _ell_cm("ell-colmajor-row-equals-M", idx=cm_bad, want="rowIdxs[6] = 6 is not below M = 6"),
        _ell_rm("ell-rowmajor-column-equals-K", idx=rm_k, want="colIdxs[7] = 7 is not below K = 7"),
        _ell_rm("ell-rowmajor-column-0xFFFFFFFE", idx=rm_fe, want="colIdxs[7] = 4294967294 is not below K = 7"),
        _bsr("bsr-block-column-equals-K-over-bC", idxs=_with(b22.block_col_idxs.tolist(), 1, 3),
             want="blockColIdxs[1] = 3 is not below K / bC = 3"),
        _bsr("bsr-2x3-block-column-equals-K-over-bC", bc=3, idxs=_with(formats.csr_to_bsr(_base_csr(COLS6, 6), 2, 3).block_col_idxs.tolist(), 1, 2),
             want="blockColIdxs[1] = 2 is not below K / bC = 2"),
        _bsr("bsr-block-row-pointers-decrease", ptrs=_with(p22, 1, p22[2] + 1), want=f"blockRowPtrs decrease at row 1 ({p22[2] + 1} then {p22[2]})"),
        _bsr("bsr-last-block-row-pointer-is-not-numBlocks", ptrs=_with(p22, 3, p22[3] + 1),
             want=f"blockRowPtrs[M / bR = 3] = {p22[3] + 1}, numBlocks = {p22[3]}"),
        _bsr("bsr-zero-block-rows", br=0, want="block shape 0 x 2 must be positive"),
        _bsr("bsr-M-is-no-multiple-of-bR", m=5, want="M = 5 is not a multiple of bR = 2"),
        _dense("dense-short-row", "\n".join(_with(good_b, 3, good_b[3].split()[0])), "row 2 holds 1 tokens, 2 are needed"),
        _dense("dense-token-is-no-number", "\n".join(_with(good_b, 2, good_b[2].split()[0] + " abc")), "row 1, token 1: not a number: 'abc'"),
        _dense("dense-header-is-not-two-numbers", "\n".join(_with(good_b, 0, "7")), "header is not two numbers"),
    ]


# ---------------------------------------------------------------------------------------------------------------- valid but unusual
def unusual():
    nan, inf = float("nan"), float("inf")
    rev = list(range(NNZ))[::-1]
    cm = formats.csr_to_ell_colmajor(_base_csr(), reference_width=True)
    # one more column line, all padding, and a row (1) that no slot names: all-padding lines of both layouts
    cm_idx = np.concatenate([cm.row_idxs, np.full((1, 3), formats.ELL_PAD, np.uint32)])
    cm_val = np.concatenate([cm.data, np.zeros((1, 3), np.float32)])
    b22 = formats.csr_to_bsr(_base_csr(COLS6, 6), 2, 2)
    b23 = formats.csr_to_bsr(_base_csr(COLS6, 6), 2, 3)
    # block row 1 emptied, block row 0 listing its blocks in descending order and one of them twice
    row0 = list(range(b22.block_row_ptrs[0], b22.block_row_ptrs[1]))[::-1]
    row0 = row0 + row0[:1]
    row2 = list(range(b22.block_row_ptrs[2], b22.block_row_ptrs[3]))
    pick = row0 + row2
    return [
        _csr("csr-base-with-an-empty-row"),
        _csr("csr-unsorted-columns", cols=[4, 1, 6, 0, 3, 2, 5, 1, 6, 4, 0]),
        _csr("csr-repeated-pairs", cols=[4, 4, 3, 3, 3, 2, 1, 1, 0, 0, 6]),
        _csr("csr-explicit-zeros", vals=_with(_with(VALS, 2, 0.0), 7, -0.0)),
        _csr("csr-nan-and-inf-values", vals=_with(_with(_with(VALS, 0, nan), 5, inf), 9, -inf)),
        _csr("csr-no-entries", ptrs=[0] * (M + 1), cols=[], vals=[]),
        _csr("csr-one-row", m=1, ptrs=[0, 3], cols=[0, 3, 6], vals=VALS[:3]),
        _csr("csr-one-column", k=1, ptrs=[0, 1, 1, 2, 2, 2, 3], cols=[0, 0, 0], vals=VALS[:3]),
        _csr("csr-one-by-one", m=1, k=1, ptrs=[0, 1], cols=[0], vals=[2.5]),
        _csr("csr-trailing-blank-lines", tail="\n\n  \n"),
        _coo("coo-base"),
        _coo("coo-reverse-order", rows=[ROWS[i] for i in rev], cols=[COLS[i] for i in rev], vals=[VALS[i] for i in rev]),
        _coo("coo-repeated-pairs-and-zeros", cols=[4, 4, 3, 3, 3, 2, 1, 1, 0, 0, 6], vals=_with(VALS, 3, 0.0)),
        _coo("coo-nan-and-inf-values", vals=_with(_with(VALS, 1, nan), 6, inf)),
        _coo("coo-no-entries", rows=[], cols=[], vals=[]),
        _coo("coo-one-by-one", m=1, k=1, rows=[0], cols=[0], vals=[-1.5]),
        _ell_cm("ell-colmajor-base-with-an-all-padding-row"),
        _ell_cm("ell-colmajor-all-padding-column", idx=cm_idx, val=cm_val, k=K + 1),
        _ell_cm("ell-colmajor-no-slots", idx=np.zeros((K, 0), np.uint32), val=np.zeros((K, 0), np.float32)),
        _ell_rm("ell-rowmajor-base-with-an-all-padding-row"),
        _bsr("bsr-2x2-base"),
        _bsr("bsr-2x3-base", bc=3, ptrs=b23.block_row_ptrs.tolist(), idxs=b23.block_col_idxs.tolist(), blocks=b23.data),
        _bsr("bsr-empty-block-row-unsorted-repeated-block-columns", ptrs=[0, len(row0), len(row0), len(pick)],
             idxs=[int(b22.block_col_idxs[i]) for i in pick], blocks=b22.data[pick]),
        _bsr("bsr-nan-inf-and-zero-blocks", blocks=np.concatenate([np.full((1, 2, 2), nan, np.float32), np.zeros((1, 2, 2), np.float32),
                                                                  np.full((1, 2, 2), inf, np.float32), b22.data[3:]])),
        _bsr("bsr-no-blocks", ptrs=[0, 0, 0, 0], idxs=[], blocks=np.zeros((0, 2, 2), np.float32)),
    ]


# ---------------------------------------------------------------------------------------------------------------- references
def oracle_product(orc, case, b):
    """The oracle's product of the case's container with b (float32 [K, N]), in the arithmetic of that format's REFERENCE mode."""
    a = case.mem
    if case.fmt == "csr":
        return orc.spmm_csr(a.row_ptrs, a.col_idxs, a.data, b)
    if case.fmt == "coo":
        return orc.spmm_coo(a.num_rows, a.row_idxs, a.col_idxs, a.data, b)
    if case.fmt == "ell_cm":
        return orc.spmm_ell_colmajor(a.num_rows, a.row_idxs, a.data, b)
    if case.fmt == "ell_rm":     # slot order inside a row, fp32 product then fp32 add: the COO arithmetic on its occupied slots
        live = a.col_idxs != formats.ELL_PAD
        rows = np.repeat(np.arange(a.num_rows, dtype=np.uint32), live.sum(axis=1))
        return orc.spmm_coo(a.num_rows, rows, a.col_idxs[live], a.data[live], b)
    return orc.spmm_bsr(a.num_rows, a.block_row_size, a.block_col_size, a.block_row_ptrs, a.block_col_idxs, a.data, b)
