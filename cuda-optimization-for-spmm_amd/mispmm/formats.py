"""Host-side sparse/dense containers and the reference's on-disk text formats.

Python mirror (numpy only) of the data layer either side of the SpMM hot path:
the MatrixMarket inputs under the reference's data/ and the text wire formats
its C++ constructors parse.  Written from scratch; the wire formats are those of
  dense.in            /root/reference/src/formats/dense.cu:9-36
  *.csr               /root/reference/src/formats/sparse_csr.cu:12-51
  *.coo               /root/reference/src/formats/sparse_coo.cu (header + "r c v" lines)
  *.bsr               /root/reference/src/formats/sparse_bsr.cu:17-61
  *_rowind.ell / *_values_colmajor.ell  (column-major ELL, the pair the CLI loads)
                      /root/reference/src/formats/sparse_ell.cu:12-53
  *_colind.ell / *_values.ell           (row-major ELL, written by the converter,
                      /root/reference/utils/python_utils/convert_mtx.py:198-239)
and the writers reproduce what utils/python_utils/convert_mtx.py emits.

Index arrays are uint32 (the reference's MT), values float32 (its DT) unless a
caller asks for float64.  ELL padding index is 0xFFFFFFFF (text "-1").
"""
from dataclasses import dataclass

import numpy as np

ELL_PAD = np.uint32(0xFFFFFFFF)


# --------------------------------------------------------------------------
# containers
# --------------------------------------------------------------------------
@dataclass
class Dense:
    data: np.ndarray  # [num_rows, num_cols], row-major

    @property
    def num_rows(self):
        return self.data.shape[0]

    @property
    def num_cols(self):
        return self.data.shape[1]


@dataclass
class CSR:
    num_rows: int
    num_cols: int
    row_ptrs: np.ndarray
    col_idxs: np.ndarray
    data: np.ndarray

    @property
    def nnz(self):
        return int(self.col_idxs.shape[0])

    def to_dense(self):
        d = np.zeros((self.num_rows, self.num_cols), dtype=self.data.dtype)
        rows = np.repeat(np.arange(self.num_rows), np.diff(self.row_ptrs.astype(np.int64)))
        d[rows, self.col_idxs.astype(np.int64)] = self.data
        return d


@dataclass
class COO:
    num_rows: int
    num_cols: int
    row_idxs: np.ndarray
    col_idxs: np.ndarray
    data: np.ndarray

    @property
    def nnz(self):
        return int(self.data.shape[0])


@dataclass
class ELLColMajor:
    """The reference's SparseMatrixELL: one line per column of A."""
    num_rows: int
    num_cols: int
    nnz: int
    max_col_nnz: int
    row_idxs: np.ndarray  # [num_cols, max_col_nnz] uint32, pad ELL_PAD
    data: np.ndarray      # [num_cols, max_col_nnz]


@dataclass
class ELLRowMajor:
    """Row-major ELL: what the row-parallel HIP kernel consumes."""
    num_rows: int
    num_cols: int
    nnz: int
    width: int
    col_idxs: np.ndarray  # [num_rows, width] uint32, pad ELL_PAD
    data: np.ndarray      # [num_rows, width]


@dataclass
class BSR:
    num_rows: int
    num_cols: int
    nnz: int               # stored elements incl. explicit zeros (convert_mtx.py:41)
    block_row_size: int
    block_col_size: int
    block_row_ptrs: np.ndarray
    block_col_idxs: np.ndarray
    data: np.ndarray       # [num_blocks, block_row_size, block_col_size]

    @property
    def num_blocks(self):
        return int(self.block_col_idxs.shape[0])

    @property
    def num_block_rows(self):
        return self.num_rows // self.block_row_size

    def to_dense(self):
        d = np.zeros((self.num_rows, self.num_cols), dtype=self.data.dtype)
        br, bc = self.block_row_size, self.block_col_size
        for i in range(self.num_block_rows):
            for b in range(int(self.block_row_ptrs[i]), int(self.block_row_ptrs[i + 1])):
                j = int(self.block_col_idxs[b])
                d[i * br:(i + 1) * br, j * bc:(j + 1) * bc] = self.data[b]
        return d


# --------------------------------------------------------------------------
# MatrixMarket (coordinate) reader, from scratch
# --------------------------------------------------------------------------
def read_mtx(path):
    """Read a MatrixMarket *coordinate* file -> COO in file order with symmetric
    entries expanded (mirror entries appended after the stored ones, diagonal
    not duplicated).  Values are float64; `pattern` entries become 1.0.
    Returns (COO, field) where field is 'real' | 'integer' | 'pattern'."""
    with open(path, "r") as f:
        header = f.readline().split()
        if len(header) < 5 or header[0] != "%%MatrixMarket" or header[1].lower() != "matrix":
            raise ValueError(f"{path}: not a MatrixMarket matrix file")
        layout, field, symmetry = header[2].lower(), header[3].lower(), header[4].lower()
        if layout != "coordinate":
            raise ValueError(f"{path}: only coordinate layout is supported, got {layout}")
        if field not in ("real", "integer", "pattern", "double"):
            raise ValueError(f"{path}: unsupported field {field}")
        if symmetry not in ("general", "symmetric", "skew-symmetric"):
            raise ValueError(f"{path}: unsupported symmetry {symmetry}")
        line = f.readline()
        while line.startswith("%") or not line.strip():
            line = f.readline()
        rows, cols, entries = (int(x) for x in line.split()[:3])
        body = np.loadtxt(f, dtype=np.float64, ndmin=2, comments="%") if entries else np.zeros((0, 3))
    if body.shape[0] != entries:
        raise ValueError(f"{path}: expected {entries} entries, found {body.shape[0]}")
    r = body[:, 0].astype(np.int64) - 1
    c = body[:, 1].astype(np.int64) - 1
    v = np.ones(entries, dtype=np.float64) if field == "pattern" else body[:, 2].astype(np.float64)
    if symmetry != "general":
        off = r != c
        sign = -1.0 if symmetry == "skew-symmetric" else 1.0
        r, c, v = (np.concatenate([r, c[off]]), np.concatenate([c, r[off]]),
                   np.concatenate([v, sign * v[off]]))
    if entries and (r.min() < 0 or c.min() < 0 or r.max() >= rows or c.max() >= cols):
        raise ValueError(f"{path}: index out of range")
    return COO(rows, cols, r.astype(np.uint32), c.astype(np.uint32), v), field


# --------------------------------------------------------------------------
# conversions
# --------------------------------------------------------------------------
def coo_to_csr(coo, dtype=np.float32):
    """Row-major sort, duplicates summed (what scipy's coo.tocsr() yields)."""
    r = coo.row_idxs.astype(np.int64)
    c = coo.col_idxs.astype(np.int64)
    v = coo.data.astype(np.float64)
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    if r.size:
        key = r * coo.num_cols + c
        first = np.concatenate([[True], key[1:] != key[:-1]])
        seg = np.cumsum(first) - 1
        v = np.bincount(seg, weights=v, minlength=int(seg[-1]) + 1)
        r, c = r[first], c[first]
    row_ptrs = np.zeros(coo.num_rows + 1, dtype=np.int64)
    np.add.at(row_ptrs, r + 1, 1)
    row_ptrs = np.cumsum(row_ptrs)
    return CSR(coo.num_rows, coo.num_cols, row_ptrs.astype(np.uint32), c.astype(np.uint32), v.astype(dtype))


def csr_to_coo(csr):
    rows = np.repeat(np.arange(csr.num_rows, dtype=np.uint32), np.diff(csr.row_ptrs.astype(np.int64)))
    return COO(csr.num_rows, csr.num_cols, rows, csr.col_idxs.copy(), csr.data.copy())


def csr_to_ell_rowmajor(csr, width=None):
    counts = np.diff(csr.row_ptrs.astype(np.int64))
    w = int(counts.max()) if counts.size and width is None else int(width or 0)
    if counts.size and counts.max() > w:
        raise ValueError("ELL width smaller than the longest row")
    col = np.full((csr.num_rows, w), ELL_PAD, dtype=np.uint32)
    val = np.zeros((csr.num_rows, w), dtype=csr.data.dtype)
    rows = np.repeat(np.arange(csr.num_rows), counts)
    slot = np.arange(csr.nnz) - np.repeat(csr.row_ptrs[:-1].astype(np.int64), counts)
    col[rows, slot] = csr.col_idxs
    val[rows, slot] = csr.data
    return ELLRowMajor(csr.num_rows, csr.num_cols, csr.nnz, w, col, val)


def csr_to_ell_colmajor(csr, reference_width=False):
    """Column-major ELL (one padded line per column of A, rows ascending).
    reference_width=True sizes the padding like the reference converter does --
    by the longest ROW (convert_mtx.py:252 takes getnnz(axis=1) of the CSC) --
    so files match its output; False uses the true longest column."""
    r = np.repeat(np.arange(csr.num_rows, dtype=np.int64), np.diff(csr.row_ptrs.astype(np.int64)))
    c = csr.col_idxs.astype(np.int64)
    order = np.lexsort((r, c))
    r, c, v = r[order], c[order], csr.data[order]
    col_counts = np.bincount(c, minlength=csr.num_cols)
    row_counts = np.diff(csr.row_ptrs.astype(np.int64))
    w = int(row_counts.max() if reference_width else col_counts.max()) if csr.nnz else 0
    if csr.nnz and col_counts.max() > w:
        raise ValueError("reference-width column-major ELL cannot hold the longest column")
    col_start = np.concatenate([[0], np.cumsum(col_counts)[:-1]])
    slot = np.arange(csr.nnz) - np.repeat(col_start, col_counts)
    ridx = np.full((csr.num_cols, w), ELL_PAD, dtype=np.uint32)
    val = np.zeros((csr.num_cols, w), dtype=csr.data.dtype)
    ridx[c, slot] = r.astype(np.uint32)
    val[c, slot] = v
    return ELLColMajor(csr.num_rows, csr.num_cols, csr.nnz, w, ridx, val)


def ell_colmajor_to_csr(ell):
    """Row-parallel view of a column-major ELL.  Within each row the entries keep
    ascending column order, then ascending slot -- the order in which the
    reference's spmmELLCpu (spmm_ell.cpp:16-29) accumulates into that row."""
    valid = ell.row_idxs.astype(np.int32) >= 0
    cols, slots = np.nonzero(valid)            # C order: column, then slot
    rows = ell.row_idxs[cols, slots].astype(np.int64)
    vals = ell.data[cols, slots]
    order = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    row_ptrs = np.zeros(ell.num_rows + 1, dtype=np.int64)
    np.add.at(row_ptrs, rows + 1, 1)
    return CSR(ell.num_rows, ell.num_cols, np.cumsum(row_ptrs).astype(np.uint32),
               cols.astype(np.uint32), vals.copy())


def ell_colmajor_to_rowmajor(ell):
    return csr_to_ell_rowmajor(ell_colmajor_to_csr(ell))


def csr_to_bsr(csr, block_row_size, block_col_size=None):
    """Blocks with at least one stored entry, block-row-major, block columns
    ascending, explicit zeros inside blocks (scipy tobsr semantics)."""
    br = int(block_row_size)
    bc = int(block_col_size or block_row_size)
    if csr.num_rows % br or csr.num_cols % bc:
        raise ValueError("matrix shape is not a multiple of the block shape")
    r = np.repeat(np.arange(csr.num_rows, dtype=np.int64), np.diff(csr.row_ptrs.astype(np.int64)))
    c = csr.col_idxs.astype(np.int64)
    nbc = csr.num_cols // bc
    key = (r // br) * nbc + (c // bc)
    ukeys, inv = np.unique(key, return_inverse=True)
    data = np.zeros((ukeys.shape[0], br, bc), dtype=csr.data.dtype)
    data[inv, r % br, c % bc] = csr.data
    brow = ukeys // nbc
    ptrs = np.zeros(csr.num_rows // br + 1, dtype=np.int64)
    np.add.at(ptrs, brow + 1, 1)
    return BSR(csr.num_rows, csr.num_cols, int(data.size), br, bc, np.cumsum(ptrs).astype(np.uint32),
               (ukeys % nbc).astype(np.uint32), data)


# --------------------------------------------------------------------------
# validity (the contract of include/mispmm.h, restated in numpy; the messages
# are those of the library's mispmm_*_check_host)
# --------------------------------------------------------------------------
def as_u32(name, a):
    """`a` as a flat uint32 array; a value that is no uint32 is an error, never wrapped."""
    a = np.asarray(a)
    if a.dtype != np.uint32:
        wide = a.astype(np.int64).reshape(-1) if a.dtype.kind in "iub" else None
        if wide is None:
            raise ValueError(f"{name} must be an integer array, not {a.dtype}")
        bad = np.flatnonzero((wide < 0) | (wide > 0xFFFFFFFF))
        if bad.size:
            raise ValueError(f"{name}[{int(bad[0])}] = {int(wide[bad[0]])} is not an index (0 .. 4294967295)")
        a = wide.astype(np.uint32)
    return np.ascontiguousarray(a).reshape(-1)


def _count(who, name, value):
    if not 0 <= int(value) <= 0xFFFFFFFF:
        raise ValueError(f"{who} check: {name} = {int(value)} is not a count (0 .. 4294967295)")
    return int(value)


def _check_length(who, name, have, need_name, need):
    if have != need:
        raise ValueError(f"{who} check: {name} holds {have} entries, {need_name} = {need} are needed")


def _check_row_pointers(who, name, rows_name, rows, ptrs, total_name, total):
    if ptrs.shape[0] != rows + 1:
        raise ValueError(f"{who} check: {name} holds {ptrs.shape[0]} entries, {rows_name} + 1 = {rows + 1} are needed")
    if ptrs[0] != 0:
        raise ValueError(f"{who} check: {name}[0] = {int(ptrs[0])}, must be 0")
    down = np.flatnonzero(ptrs[1:] < ptrs[:-1])
    if down.size:
        r = int(down[0])
        raise ValueError(f"{who} check: {name} decrease at row {r} ({int(ptrs[r])} then {int(ptrs[r + 1])})")
    if ptrs[rows] != total:
        raise ValueError(f"{who} check: {name}[{rows_name} = {rows}] = {int(ptrs[rows])}, {total_name} = {total}")


def _check_below(who, name, idxs, bound_name, bound, live=None, note=""):
    bad = idxs >= bound if live is None else live & (idxs >= bound)
    at = np.flatnonzero(bad)
    if at.size:
        raise ValueError(f"{who} check: {name}[{int(at[0])}] = {int(idxs[at[0]])} is not below {bound_name} = {bound}{note}")


def check_csr(csr):
    m, k, nnz = _count("csr", "M", csr.num_rows), _count("csr", "K", csr.num_cols), _count("csr", "nnz", csr.nnz)
    ptrs, cols = as_u32("rowPtrs", csr.row_ptrs), as_u32("colIdxs", csr.col_idxs)
    _check_row_pointers("csr", "rowPtrs", "M", m, ptrs, "nnz", nnz)
    _check_length("csr", "colIdxs", cols.shape[0], "nnz", nnz)
    _check_length("csr", "data", np.asarray(csr.data).size, "nnz", nnz)
    _check_below("csr", "colIdxs", cols, "K", k)


def check_coo(coo):
    m, k, nnz = _count("coo", "M", coo.num_rows), _count("coo", "K", coo.num_cols), _count("coo", "nnz", coo.nnz)
    rows, cols = as_u32("rowIdxs", coo.row_idxs), as_u32("colIdxs", coo.col_idxs)
    _check_length("coo", "rowIdxs", rows.shape[0], "nnz", nnz)
    _check_length("coo", "colIdxs", cols.shape[0], "nnz", nnz)
    _check_below("coo", "rowIdxs", rows, "M", m)
    _check_below("coo", "colIdxs", cols, "K", k)


def check_ell(ell):
    """ELLColMajor: a row index with the sign bit set is padding; ELLRowMajor: 0xFFFFFFFF alone is."""
    m, k = _count("ell", "M", ell.num_rows), _count("ell", "K", ell.num_cols)
    if isinstance(ell, ELLColMajor):
        w, idxs = _count("ell", "maxColNnz", ell.max_col_nnz), as_u32("rowIdxs", ell.row_idxs)
        _check_length("ell", "rowIdxs", idxs.shape[0], "K * maxColNnz", k * w)
        _check_length("ell", "data", np.asarray(ell.data).size, "K * maxColNnz", k * w)
        _check_below("ell", "rowIdxs", idxs, "M", m, live=idxs < 0x80000000)
    else:
        w, idxs = _count("ell", "width", ell.width), as_u32("colIdxs", ell.col_idxs)
        _check_length("ell", "colIdxs", idxs.shape[0], "M * width", m * w)
        _check_length("ell", "data", np.asarray(ell.data).size, "M * width", m * w)
        _check_below("ell", "colIdxs", idxs, "K", k, live=idxs != ELL_PAD, note=" (padding is 4294967295 alone)")


def check_bsr(bsr):
    m, k = _count("bsr", "M", bsr.num_rows), _count("bsr", "K", bsr.num_cols)
    br, bc = _count("bsr", "bR", bsr.block_row_size), _count("bsr", "bC", bsr.block_col_size)
    nb = _count("bsr", "numBlocks", bsr.num_blocks)
    if br == 0 or bc == 0:
        raise ValueError(f"bsr check: block shape {br} x {bc} must be positive")
    if m % br:
        raise ValueError(f"bsr check: M = {m} is not a multiple of bR = {br}")
    if k % bc:
        raise ValueError(f"bsr check: K = {k} is not a multiple of bC = {bc}")
    ptrs, cols = as_u32("blockRowPtrs", bsr.block_row_ptrs), as_u32("blockColIdxs", bsr.block_col_idxs)
    _check_row_pointers("bsr", "blockRowPtrs", "M / bR", m // br, ptrs, "numBlocks", nb)
    _check_length("bsr", "blockColIdxs", cols.shape[0], "numBlocks", nb)
    _check_below("bsr", "blockColIdxs", cols, "K / bC", k // bc)
    _check_length("bsr", "data", np.asarray(bsr.data).size, "numBlocks * bR * bC", nb * br * bc)


# --------------------------------------------------------------------------
# text readers (the formats the reference's C++ constructors parse)
# --------------------------------------------------------------------------
class _Text:
    """The whitespace-separated tokens of one text file, read in order.  Every refusal is a ValueError
    `<path>: malformed <kind> file: <what>`; an index token is range-checked as a signed 64-bit number
    before it becomes a uint32, so "-1" never wraps silently."""

    def __init__(self, path, kind):
        self.path, self.kind = path, kind
        with open(path, "r") as f:
            self.text = f.read()
        self.tokens = self.text.split()
        self.at = 0

    def bad(self, what):
        raise ValueError(f"{self.path}: malformed {self.kind} file: {what}")

    def promise(self, tokens):
        """A token needs at least two bytes (itself and a separator): refuse a header that promises more than the
        file can hold before anything is allocated."""
        if tokens * 2 > len(self.text) + 1:
            self.bad(f"header promises {tokens} tokens, the file has {len(self.text)} bytes")

    def take(self, name, count):
        got = self.tokens[self.at:self.at + count]
        if len(got) != count:
            self.bad(f"truncated: {name} holds {len(got)} tokens, {count} are needed")
        self.at += count
        return got

    def numbers(self, toks, dtype, label):
        try:
            return np.array(toks, dtype=dtype)
        except (ValueError, OverflowError):
            for i, t in enumerate(toks):
                try:
                    dtype(t)
                except (ValueError, OverflowError):
                    self.bad(f"{label(i)}: not a number: '{t}'")
            raise

    def header(self, names):
        vals = self.numbers(self.take("header", len(names)), np.int64, lambda i: names[i])
        for n, v in zip(names, vals):
            if not 0 <= v <= 0xFFFFFFFF:
                self.bad(f"header: {n} = {int(v)} is not a count (0 .. 4294967295)")
        return [int(v) for v in vals]

    def indices(self, name, toks, lowest=0):
        vals = self.numbers(toks, np.int64, lambda i: f"{name}[{i}]")
        bad = np.flatnonzero((vals < lowest) | (vals > 0xFFFFFFFF))
        if bad.size:
            self.bad(f"{name}[{int(bad[0])}] = {int(vals[bad[0]])} is not an index")
        return (vals & 0xFFFFFFFF).astype(np.uint32)

    def values(self, name, toks):
        return self.numbers(toks, np.float64, lambda i: f"{name}[{i}]")

    def checked(self, matrix, check):
        try:
            check(matrix)
        except ValueError as e:
            self.bad(str(e))
        return matrix


def read_dense(path, dtype=np.float32):
    """`rows cols [nnz]` header (rest of the line ignored, dense.cu:23-24) then one text line per row, each
    of exactly `cols` numbers."""
    t = _Text(path, "dense")
    lines = t.text.split("\n")
    head = lines[0].split()
    try:
        rows, cols = int(head[0]), int(head[1])
    except (IndexError, ValueError):
        t.bad(f"header is not two numbers: '{lines[0].strip()}'")
    if not (0 <= rows <= 0xFFFFFFFF and 0 <= cols <= 0xFFFFFFFF):
        t.bad(f"header is not two counts: '{lines[0].strip()}'")
    t.promise(2 + rows * cols)
    data = np.empty((rows, cols), dtype=np.float64)
    for i in range(rows):
        toks = lines[1 + i].split() if 1 + i < len(lines) else None
        if toks is None:
            t.bad(f"fewer rows than the header says: row {i} is missing")
        if len(toks) != cols:
            t.bad(f"row {i} holds {len(toks)} tokens, {cols} are needed")
        data[i] = t.numbers(toks, np.float64, lambda j: f"row {i}, token {j}")
    return Dense(data.astype(dtype))


def read_csr(path, dtype=np.float32):
    t = _Text(path, ".csr")
    rows, cols, nnz = t.header(("numRows", "numCols", "numNonZero"))
    t.promise(3 + rows + 1 + 2 * nnz)
    row_ptrs = t.indices("rowPtrs", t.take("rowPtrs", rows + 1))
    col_idxs, data = t.indices("colIdxs", t.take("colIdxs", nnz)), t.values("data", t.take("data", nnz))
    return t.checked(CSR(rows, cols, row_ptrs, col_idxs, data.astype(dtype)), check_csr)


def read_coo(path, dtype=np.float32):
    t = _Text(path, ".coo")
    rows, cols, nnz = t.header(("numRows", "numCols", "numNonZero"))
    t.promise(3 + 3 * nnz)
    toks = t.take("entries", 3 * nnz)                      # "row col value" per entry
    r, c, v = t.indices("rowIdxs", toks[0::3]), t.indices("colIdxs", toks[1::3]), t.values("data", toks[2::3])
    return t.checked(COO(rows, cols, r, c, v.astype(dtype)), check_coo)


def read_bsr(path, dtype=np.float32):
    t = _Text(path, ".bsr")
    rows, cols, nnz, br, bc, nblocks = t.header(("numRows", "numCols", "numNonZero", "blockRowSize", "blockColSize", "numBlocks"))
    if br == 0 or bc == 0:
        t.bad(f"bsr check: block shape {br} x {bc} must be positive")
    if rows % br:
        t.bad(f"bsr check: M = {rows} is not a multiple of bR = {br}")
    t.promise(6 + rows // br + 1 + nblocks + nblocks * br * bc)
    ptrs = t.indices("blockRowPtrs", t.take("blockRowPtrs", rows // br + 1))
    idxs = t.indices("blockColIdxs", t.take("blockColIdxs", nblocks))
    vals = t.values("data", t.take("data", nblocks * br * bc))
    return t.checked(BSR(rows, cols, nnz, br, bc, ptrs, idxs, vals.reshape(nblocks, br, bc).astype(dtype)), check_bsr)


def _read_ell_pair(index_path, values_path, lines_from_cols, dtype):
    t = _Text(index_path, "ELL")
    rows, cols, nnz, width = t.header(("numRows", "numCols", "numNonZero", "width"))
    n = cols if lines_from_cols else rows
    t.promise(4 + n * width)
    # "-1" -> 0xFFFFFFFF exactly as `istream >> uint32_t` wraps it (sparse_ell.cu:38-43); what a wrapped negative
    # means (padding or not) is the layout's business: check_ell
    name = "rowIdxs" if lines_from_cols else "colIdxs"
    idx = t.indices(name, t.take(name, n * width), lowest=-0x80000000)
    tv = _Text(values_path, "ELL")
    tv.promise(n * width)
    val = tv.values("data", tv.take("data", n * width))
    return t, rows, cols, nnz, width, idx.reshape(n, width), val.reshape(n, width).astype(dtype)


def read_ell_colmajor(rowind_path, values_path, dtype=np.float32):
    t, rows, cols, nnz, w, idx, val = _read_ell_pair(rowind_path, values_path, True, dtype)
    return t.checked(ELLColMajor(rows, cols, nnz, w, idx, val), check_ell)


def read_ell_rowmajor(colind_path, values_path, dtype=np.float32):
    t, rows, cols, nnz, w, idx, val = _read_ell_pair(colind_path, values_path, False, dtype)
    return t.checked(ELLRowMajor(rows, cols, nnz, w, idx, val), check_ell)


# --------------------------------------------------------------------------
# text writers (what utils/python_utils/convert_mtx.py emits)
# --------------------------------------------------------------------------
def _fmt(values, integer):
    if integer:
        return " ".join(str(int(v)) for v in values)
    return " ".join(repr(float(v)) for v in values)


def write_dense(path, dense, integer=False):
    d = np.asarray(dense.data if isinstance(dense, Dense) else dense)
    with open(path, "w") as f:
        f.write(f"{d.shape[0]} {d.shape[1]} {int(np.count_nonzero(d))}\n")
        for row in d:
            f.write(_fmt(row, integer) + "\n")


def write_csr(path, csr, integer=False):
    with open(path, "w") as f:
        f.write(f"{csr.num_rows} {csr.num_cols} {csr.nnz}\n")
        f.write(" ".join(map(str, csr.row_ptrs.tolist())) + "\n")
        f.write(" ".join(map(str, csr.col_idxs.tolist())) + "\n")
        f.write(_fmt(csr.data, integer) + "\n")


def write_coo(path, coo, integer=False):
    order = np.lexsort((coo.col_idxs, coo.row_idxs))
    with open(path, "w") as f:
        f.write(f"{coo.num_rows} {coo.num_cols} {coo.nnz}\n")
        for i in order:
            f.write(f"{int(coo.row_idxs[i])} {int(coo.col_idxs[i])} {_fmt([coo.data[i]], integer)}\n")


def write_bsr(path, bsr, integer=False):
    with open(path, "w") as f:
        f.write(f"{bsr.num_rows} {bsr.num_cols} {bsr.nnz} {bsr.block_row_size} {bsr.block_col_size} "
                f"{bsr.num_blocks}\n")
        f.write(" ".join(map(str, bsr.block_row_ptrs.tolist())) + "\n")
        f.write(" ".join(map(str, bsr.block_col_idxs.tolist())) + "\n")
        for block in bsr.data:
            f.write(_fmt(block.reshape(-1), integer) + "\n")


def _write_ell(index_path, values_path, header, idx, val, integer):
    with open(index_path, "w") as f:
        f.write(header + "\n")
        for line in idx.astype(np.int32):   # 0xFFFFFFFF -> "-1"
            f.write(" ".join(map(str, line.tolist())) + "\n")
    with open(values_path, "w") as f:
        pad = idx == ELL_PAD
        for line, p in zip(val, pad):
            # the reference pads values with the int literal 0 (convert_mtx.py:210,255)
            f.write(" ".join("0" if pp else _fmt([v], integer) for v, pp in zip(line, p)) + "\n")


def write_ell_colmajor(rowind_path, values_path, ell, integer=False):
    _write_ell(rowind_path, values_path, f"{ell.num_rows} {ell.num_cols} {ell.nnz} {ell.max_col_nnz}",
               ell.row_idxs, ell.data, integer)


def write_ell_rowmajor(colind_path, values_path, ell, integer=False):
    _write_ell(colind_path, values_path, f"{ell.num_rows} {ell.num_cols} {ell.nnz} {ell.width}",
               ell.col_idxs, ell.data, integer)
