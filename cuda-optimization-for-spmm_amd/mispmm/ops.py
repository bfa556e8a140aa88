"""SpMM entry points on torch tensors: thin plumbing from torch device memory and
streams to the C ABI (data_ptr() in, data_ptr() out).  PyTorch is used for
allocation and stream handles only -- all arithmetic happens in libmispmm.so."""
import ctypes
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import capi, formats


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _dev_u32(a, device):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to(device)


def _dev_f32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _dev_f64(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def _check_dtype(dtype, what=None):
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what + ': ' if what else ''}dtype must be torch.float32 or torch.float64, not {dtype}")
    return dtype == torch.float64


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise ValueError("mispmm ops take device tensors; there is no CPU path")


def check_host(m):
    """The validity contract of include/mispmm.h on a host container, by the library's own checker (mispmm_csr_check_host /
    _coo_ / _ell_ / _bsr_): raises capi.MispmmError naming the first defect.  Every from_host runs it before anything is
    built or uploaded; an index array that is not uint32 is range-checked first (ValueError), never wrapped."""
    l, u32 = capi.lib(), formats.as_u32
    if isinstance(m, formats.CSR):
        rp, ci = u32("rowPtrs", m.row_ptrs), u32("colIdxs", m.col_idxs)
        st = l.mispmm_csr_check_host(m.num_rows, m.num_cols, m.nnz, rp.ctypes.data, rp.size, ci.ctypes.data, ci.size)
        values, want = m.data, m.nnz
    elif isinstance(m, formats.COO):
        ri, ci = u32("rowIdxs", m.row_idxs), u32("colIdxs", m.col_idxs)
        st = l.mispmm_coo_check_host(m.num_rows, m.num_cols, m.nnz, ri.ctypes.data, ri.size, ci.ctypes.data, ci.size)
        values, want = m.data, m.nnz
    elif isinstance(m, formats.ELLColMajor):
        ri = u32("rowIdxs", m.row_idxs)
        st = l.mispmm_ell_check_host(capi.ELL_COLUMN_MAJOR, m.num_rows, m.num_cols, m.max_col_nnz, ri.ctypes.data, ri.size)
        values, want = m.data, ri.size
    elif isinstance(m, formats.ELLRowMajor):
        ci = u32("colIdxs", m.col_idxs)
        st = l.mispmm_ell_check_host(capi.ELL_ROW_MAJOR, m.num_rows, m.num_cols, m.width, ci.ctypes.data, ci.size)
        values, want = m.data, ci.size
    elif isinstance(m, formats.BSR):
        rp, ci = u32("blockRowPtrs", m.block_row_ptrs), u32("blockColIdxs", m.block_col_idxs)
        st = l.mispmm_bsr_check_host(m.num_rows, m.num_cols, m.block_row_size, m.block_col_size, m.num_blocks, rp.ctypes.data, rp.size,
                                     ci.ctypes.data, ci.size, np.asarray(m.data).size)
        values, want = m.data, np.asarray(m.data).size
    else:
        raise TypeError(f"no structure check for {type(m).__name__}")
    capi.check(st)
    if np.asarray(values).size != want:
        raise ValueError(f"{type(m).__name__}: data holds {np.asarray(values).size} values, {want} are needed")


# ---- the operand contract: what the C ABI cannot see (a dtype, the extent of an allocation, the length of a list) is checked
# here, once, before any call into a library.  The checks read attributes only: no synchronisation, no allocation, no copy.
_DENSE_WORDS = {torch.float32: "{what}: dense operands must be 2-D float32 with unit column stride",
                torch.float64: "{what}: with a float64 A, dense operands must be 2-D float64 with unit column stride",
                torch.int16: "{what} must be a 2-D int16 tensor of bf16 bits with unit column stride"}


def _acc_mode(acc):
    """The library's number of an accumulation mode given by name."""
    if acc not in capi.ACC_MODES:
        raise ValueError(f"acc must be one of {sorted(capi.ACC_MODES)}, not {acc!r}")
    return capi.ACC_MODES[acc]


def _dense(t, what, dtype=torch.float32, rows=None, of="A has {} columns"):
    """Row stride of a 2-D dense operand of `dtype` with unit column stride, of `rows` rows where given, whose rows do not
    overlap one another (an expanded tensor's do).  A single row may have any stride."""
    if t.dim() != 2 or t.dtype != dtype or t.stride(1) != 1 and t.shape[1] > 1:
        raise ValueError(_DENSE_WORDS[dtype].format(what=what) + f", not {t.dtype} {tuple(t.shape)} with strides {tuple(t.stride())}")
    if rows is not None and t.shape[0] != rows:
        raise ValueError(f"{what} has {t.shape[0]} rows, {of.format(rows)}")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))
    if ld < t.shape[1]:
        raise ValueError(f"{what} must not overlap its own rows (row stride {ld} < {t.shape[1]} columns), e.g. an expanded tensor")
    return ld


def _dense_out(out, m, n, like, dtype=torch.float32, what="out"):
    """(out, its row stride): `out` checked as an [m, n] result of `dtype`, or a fresh one on like's device."""
    if out is None:
        return torch.empty((m, n), dtype=dtype, device=like.device), n
    _require_gpu(out)
    if tuple(out.shape) != (m, n):
        raise ValueError(f"{what} has shape {tuple(out.shape)}, expected {(m, n)}")
    return out, _dense(out, what, dtype)


def _dense_list(ts, what, dtype, rows, of, count=None, cols=None):
    """Row stride shared by a list of dense operands: EVERY member checked like _dense and against the first one's shape and
    row stride; `count` members where given, of `cols` columns where given."""
    if not isinstance(ts, (list, tuple)):
        raise ValueError(f"{what} must be a list of tensors, not {type(ts).__name__}")
    if count is not None and len(ts) != count:
        raise ValueError(f"{what} holds {len(ts)} tensors, {count} are needed: one per operand")
    ld0 = None
    for i, t in enumerate(ts):
        _require_gpu(t)
        ld = _dense(t, f"{what}[{i}]", dtype, rows, of)
        if ld0 is None:
            ld0 = ld
        if t.shape != ts[0].shape or ld != ld0:
            raise ValueError(f"{what}[{i}]: batched operands must share one shape and row stride")
        if cols is not None and t.shape[1] != cols:
            raise ValueError(f"{what}[{i}] has {t.shape[1]} columns, expected {cols}")
    return ld0


def _flat(t, what, dtype, count, exact=True):
    """t as a contiguous array of `count` elements of `dtype` (at least `count` with exact=False), whatever its shape."""
    if t.dtype != dtype or not t.is_contiguous() or (t.numel() != count if exact else t.numel() < count):
        raise ValueError(f"{what} must be a contiguous {dtype} tensor of {'' if exact else 'at least '}{count} elements, not {t.dtype} "
                         f"{tuple(t.shape)} with strides {tuple(t.stride())}")


def uniform_row_nnz(row_ptrs):
    """w if every row holds exactly w entries (rowPtrs[r] == r * w), else 0.  O(M) host scan."""
    rp = np.asarray(row_ptrs, dtype=np.int64)
    if rp.shape[0] < 2 or rp[0] != 0:
        return 0
    w = int(rp[1])
    return w if w > 0 and np.array_equal(rp, np.arange(rp.shape[0], dtype=np.int64) * w) else 0


def csr_spans_by_length(row_ptrs, share_len=0):
    """The span list mispmm_csr_split_f32 walks (mispmm_csr_spans_by_length_host): [count, 4] uint32, the rows as
    (row, start, end, 0) longest first, preceded by the rows of more than share_len entries (0 = 128) as 4 chunks
    (row, start, end, 1) each."""
    rp = np.ascontiguousarray(row_ptrs, dtype=np.uint32)
    m = max(rp.shape[0] - 1, 0)
    count = ctypes.c_uint32(0)
    capi.check(capi.lib().mispmm_csr_spans_by_length_host(m, rp.ctypes.data, int(share_len), ctypes.byref(count), None))
    spans = np.zeros((count.value, 4), dtype=np.uint32)
    if count.value:
        capi.check(capi.lib().mispmm_csr_spans_by_length_host(m, rp.ctypes.data, int(share_len), ctypes.byref(count), spans.ctypes.data))
    return spans


HYBRID_ROW_LEN = 32   # rows of more entries go to the split body of mispmm_csr_hybrid_f32, the others to its row-gather body
LONGEST_ROW_FOR_SPANS = 64   # a matrix of short rows with a row this long (tols4000: mean 2.2, longest 90) gets a span list too


def wants_spans(row_ptrs):
    """(build a span list, for the two-body launch only): long rows on average (24 entries or more: the split kernel's
    domain), or short rows on average with a few long ones -- a lane group walks a row of L entries in L / 8 memory round
    trips whatever the rest of the GPU does, so those few rows decide the launch; the two-body launch gives them to the
    split kernel's body.  Without such a launch for the shape the second kind keeps its format's own kernel."""
    rp = np.asarray(row_ptrs, dtype=np.int64)
    m = rp.shape[0] - 1
    if m <= 0 or rp[-1] == 0:
        return False, False
    if int(rp[-1]) // m >= 24:
        return True, False
    build = int(np.diff(rp).max()) >= LONGEST_ROW_FOR_SPANS
    return build, build


def spans_long_count(spans, threshold=HYBRID_ROW_LEN):
    """How many leading positions of a span list hold the long rows (mispmm_csr_spans_long_count_host)."""
    sp = np.ascontiguousarray(spans, dtype=np.uint32).reshape(-1, 4)
    n = ctypes.c_uint32(0)
    capi.check(capi.lib().mispmm_csr_spans_long_count_host(sp.shape[0], sp.ctypes.data, int(threshold), ctypes.byref(n)))
    return n.value


def cluster_rows(csr, parts=4):
    """Greedy row clustering (mispmm_csr_cluster_rows_host): (order, natural_distinct, clustered_distinct) -- order[i] = the
    original row at position i; the two counts are the distinct columns summed over `parts` equal row parts before / after."""
    rp = np.ascontiguousarray(csr.row_ptrs, dtype=np.uint32)
    ci = np.ascontiguousarray(csr.col_idxs, dtype=np.uint32)
    order = np.empty(csr.num_rows, dtype=np.uint32)
    nat, clu = ctypes.c_uint64(0), ctypes.c_uint64(0)
    capi.check(capi.lib().mispmm_csr_cluster_rows_host(csr.num_rows, csr.num_cols, rp.ctypes.data, ci.ctypes.data, int(parts),
                                                        order.ctypes.data, ctypes.byref(nat), ctypes.byref(clu)))
    return order, nat.value, clu.value


def permute_rows(csr, order):
    """The CSR whose row i is row order[i] of `csr` (mispmm_csr_permute_rows_host)."""
    rp = np.ascontiguousarray(csr.row_ptrs, dtype=np.uint32)
    ci = np.ascontiguousarray(csr.col_idxs, dtype=np.uint32)
    va = np.ascontiguousarray(csr.data, dtype=np.float32)
    od = np.ascontiguousarray(order, dtype=np.uint32)
    rp2, ci2, va2 = np.empty_like(rp), np.empty_like(ci), np.empty_like(va)
    capi.check(capi.lib().mispmm_csr_permute_rows_host(csr.num_rows, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, od.ctypes.data,
                                                        rp2.ctypes.data, ci2.ctypes.data, va2.ctypes.data))
    return formats.CSR(csr.num_rows, csr.num_cols, rp2, ci2, va2)


@dataclass
class CsrPlan:
    """The rows of a CSR in a clustered order (rows that read the same B rows together), for mispmm_csr_plan_f32."""
    row_ptrs: torch.Tensor
    col_idxs: torch.Tensor
    data: torch.Tensor
    row_map: torch.Tensor        # row_map[i] = the C row array row i produces
    parts: int
    natural_distinct: int        # distinct columns summed over the parts, storage order ...
    clustered_distinct: int      # ... and plan order


PLAN_PARTS = 8                   # clusters: K=512 in-process A/B (profiles/r3/plan_order.log): 4 clusters -3.3 %, 8 -4.5 %, 16 -3.0 %, 64 -0.6 %
PLAN_MIN_GAIN = 0.10             # keep a plan only if it cuts the per-part distinct columns by this much
# When the plan is USED.  Measured on MI355X, in-process A/B on one set of operands (profiles/r3/plan_order.log): the
# clustered order pays where the slice of B an XCD reads -- every B row x the XCD's column part -- does not fit its 4 MiB
# L2 (n4c6-b13 x K=512: 6.5 MB per XCD, 13.60 -> 12.99 us) and LOSES elsewhere (K=128 3.47 -> 3.69 us, K=256 with 3.3 MB
# per XCD 5.75 -> 6.51: the scattered C rows cost more than the order saves).  MISPMM_PLAN_MIN_N=<n> (measurement aid) replaces
# the rule by "from n columns on".
PLAN_MIN_N = int(os.environ["MISPMM_PLAN_MIN_N"]) if "MISPMM_PLAN_MIN_N" in os.environ else None
L2_BYTES = 4 << 20


def plan_pays(num_cols, n):
    """The footprint RULE (the prior, used when the choice cannot be measured): True where the B slice one XCD reads (num_cols
    rows x its column part of n / 8 columns, fp32) exceeds the L2."""
    if PLAN_MIN_N is not None:
        return n >= PLAN_MIN_N
    return n % 512 == 0 and num_cols * (n // 8) * 4 > L2_BYTES


AUTOTUNE = os.environ.get("MISPMM_AUTOTUNE", "1") != "0"   # MISPMM_AUTOTUNE=0: the footprint rule alone (measurement aid)


def autotune_pick(times_us, min_gain=0.02):
    """mispmm_autotune_pick: index of the candidate to take given its timings -- a pure function (candidate 0 = the default
    is kept unless another is at least min_gain faster)."""
    arr = (ctypes.c_float * len(times_us))(*[float(t) for t in times_us])
    return int(capi.lib().mispmm_autotune_pick(arr, len(times_us), ctypes.c_float(min_gain)))


def use_plan(a, n, acc="reference", stream=None):
    """Plan order or storage order for a product of `a` with a dense operand of n columns: MEASURED on the first product of that
    width (mispmm_csr_autotune_plan_f32: both candidates timed on scratch operands, ~1-2 ms) and remembered in a.tuned; the
    footprint rule where it cannot be measured (stream being captured, autotune switched off, MISPMM_PLAN_MIN_N given).
    a: a float32 DeviceCSR; acc: "reference" or "fast"."""
    mode = _acc_mode(acc)
    if a.plan is None:
        return False
    if PLAN_MIN_N is not None or not AUTOTUNE:
        return plan_pays(a.num_cols, n)
    key = (int(n), acc)
    if key not in a.tuned:
        p = a.plan
        use, times = ctypes.c_int(0), (ctypes.c_float * 2)()
        st = capi.lib().mispmm_csr_autotune_plan_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs), _p(a.data),
                                                     a.uniform_row_nnz, _p(p.row_ptrs), _p(p.col_idxs), _p(p.data), _p(p.row_map), int(n),
                                                     mode, 0, ctypes.byref(use), times)
        if st != capi.OK:                       # e.g. the stream is being captured: nothing measured, nothing remembered
            return plan_pays(a.num_cols, n)
        a.tuned[key] = (bool(use.value), (float(times[0]), float(times[1])))
    return a.tuned[key][0]


@dataclass
class DeviceCSR:
    num_rows: int
    num_cols: int
    nnz: int
    row_ptrs: torch.Tensor
    col_idxs: torch.Tensor
    data: torch.Tensor
    uniform_row_nnz: int = 0     # > 0: structure hint checked on the host when A was uploaded
    spans: torch.Tensor = None   # rows longest first, for the split kernel; built at upload for long-row matrices
    plan: CsrPlan = None         # rows in a clustered order, kept when the clustering cuts the B rows an XCD must fetch
    long_spans: int = 0          # leading positions of `spans` that hold the long rows (the split body of the two-body launch)
    spans_hybrid_only: bool = False   # short rows on average: the list is for the two-body launch only, never the split kernel
    tuned: dict = field(default_factory=dict)   # (n, acc) -> (use the plan?, (storage-order us, plan-order us)) as measured by use_plan

    @staticmethod
    def from_host(csr, device="cuda", spans=None, share_len=0, plan=None, dtype=torch.float32, check=True):
        """spans: True / False to build the span list of the split kernel or not; None = when the mean row holds 24 entries
        or more (where the library's kernel 0 takes the split kernel).  share_len: rows longer than this are dealt to the 4
        waves of a workgroup (0 = the library's default, 128).  plan: True / False to keep a clustered row order or not;
        None = when the matrix has short rows (no span list), at least 1024 rows, and the clustering cuts the distinct
        columns per row part by PLAN_MIN_GAIN or more (a once-per-upload analysis like the two above).
        dtype=torch.float64: the host array's own values in double, for mispmm_csr_f64; no span list, no plan.
        check: run check_host first (one pass over the index arrays); False only for arrays already checked."""
        if check:
            check_host(csr)
        if _check_dtype(dtype):
            return DeviceCSR(csr.num_rows, csr.num_cols, csr.nnz, _dev_u32(csr.row_ptrs, device), _dev_u32(csr.col_idxs, device),
                             _dev_f64(csr.data, device))
        hybrid_only = False
        if spans is None:
            spans, hybrid_only = wants_spans(csr.row_ptrs)
        sp_host = csr_spans_by_length(csr.row_ptrs, share_len) if spans else None
        sp = _dev_u32(sp_host.reshape(-1), device) if spans else None
        n_long = spans_long_count(sp_host) if spans else 0
        pl = None
        if plan or (plan is None and not spans and csr.num_rows >= 1024 and csr.nnz > 0):
            order, nat, clu = cluster_rows(csr, PLAN_PARTS)
            if plan or clu <= (1.0 - PLAN_MIN_GAIN) * nat:
                pc = permute_rows(csr, order)
                pl = CsrPlan(_dev_u32(pc.row_ptrs, device), _dev_u32(pc.col_idxs, device), _dev_f32(pc.data, device),
                             _dev_u32(order, device), PLAN_PARTS, nat, clu)
        return DeviceCSR(csr.num_rows, csr.num_cols, csr.nnz, _dev_u32(csr.row_ptrs, device),
                         _dev_u32(csr.col_idxs, device), _dev_f32(csr.data, device), uniform_row_nnz(csr.row_ptrs), sp, pl, n_long, hybrid_only)


@dataclass
class DeviceELL:
    num_rows: int
    num_cols: int
    width: int
    col_idxs: torch.Tensor
    data: torch.Tensor
    compact: tuple = None     # (nnz, rowPtrs, colIdxs, vals) of the occupied slots, when most of the ELL is padding

    @staticmethod
    def from_host(ell, device="cuda", compact=None, dtype=torch.float32, check=True):
        """compact: True / False to list the occupied slots (mispmm_ell_compact_host) or not; None = when more than half of
        the slots are padding.  dtype=torch.float64: the occupied slots as a row list of doubles in spmmELLCpu's order of
        addition (compact = that list, col_idxs / data its arrays), for mispmm_csr_f64.  check: run check_host first."""
        if check:
            check_host(ell)
        if _check_dtype(dtype):
            rp, ci, va = ell_rows_f64(ell)
            listed = (int(rp[-1]), _dev_u32(rp, device), _dev_u32(ci, device), _dev_f64(va, device), None)
            return DeviceELL(ell.num_rows, ell.num_cols, int(np.diff(rp.astype(np.int64)).max(initial=0)), listed[2], listed[3], listed)
        if isinstance(ell, formats.ELLColMajor):
            ell = colmajor_ell_to_rowmajor(ell)
        cols = np.ascontiguousarray(ell.col_idxs, dtype=np.uint32).reshape(-1)
        vals = np.ascontiguousarray(ell.data, dtype=np.float32).reshape(-1)
        listed = None
        if compact is None:
            compact = cols.size > 0 and int(np.count_nonzero(cols == 0xFFFFFFFF)) * 2 > cols.size
        if compact:
            nnz = ctypes.c_uint32(0)
            head = (ell.num_rows, ell.width, cols.ctypes.data, vals.ctypes.data, ctypes.byref(nnz))
            capi.check(capi.lib().mispmm_ell_compact_host(*head, None, None, None))
            rp = np.zeros(ell.num_rows + 1, np.uint32)
            ci, va = np.zeros(max(nnz.value, 1), np.uint32), np.zeros(max(nnz.value, 1), np.float32)
            capi.check(capi.lib().mispmm_ell_compact_host(*head, rp.ctypes.data, ci.ctypes.data, va.ctypes.data))
            listed = (nnz.value, _dev_u32(rp, device), _dev_u32(ci, device), _dev_f32(va, device), _row_spans(rp, device))
        return DeviceELL(ell.num_rows, ell.num_cols, ell.width, _dev_u32(ell.col_idxs, device),
                         _dev_f32(ell.data, device), listed)


@dataclass
class DeviceBSR:
    num_rows: int
    num_cols: int
    block_row_size: int
    block_col_size: int
    num_blocks: int
    block_row_ptrs: torch.Tensor
    block_col_idxs: torch.Tensor
    data: torch.Tensor       # float32 blocks, or int16-viewed bf16 bit patterns

    @staticmethod
    def from_host(bsr, device="cuda", check=True):
        if check:
            check_host(bsr)
        return DeviceBSR(bsr.num_rows, bsr.num_cols, bsr.block_row_size, bsr.block_col_size, bsr.num_blocks,
                         _dev_u32(bsr.block_row_ptrs, device), _dev_u32(bsr.block_col_idxs, device),
                         _dev_f32(bsr.data.reshape(-1), device))


@dataclass
class RowSpans:
    """One span per row of a COO / ELL / BSR list, longest first, on the device (mispmm_rows_split_f32 / mispmm_rows_hybrid_f32)."""
    spans: torch.Tensor
    long_spans: int      # leading positions that hold rows of more than HYBRID_ROW_LEN entries: the split shape's share of the two-body launch
    hybrid_only: bool    # short rows on average with a few long ones: the two-body launch or the format's own kernel, never the split kernel


def _row_spans(row_ptrs, device):
    """One span per row, longest first (the fp32 arithmetic of COO / ELL / BSR cannot deal a row to several waves), for a
    list of 24 entries per row or more; else None."""
    build, hybrid_only = wants_spans(row_ptrs)
    if not build:
        return None
    host = csr_spans_by_length(row_ptrs, 0xFFFFFFFF)
    return RowSpans(_dev_u32(host.reshape(-1), device), spans_long_count(host), hybrid_only)


def _rows_split(rs, num_rows, num_cols, nnz, col_idxs, data, b, c, acc, stream):
    """rs: RowSpans or None.  The two-body launch (mispmm_rows_hybrid_f32), else mispmm_rows_split_f32, if list and operands
    allow it; False = take the format's own entry point."""
    if rs is None:
        return False
    mode = _acc_mode(acc)
    ldb = _dense(b, "b", rows=num_cols)
    _, ldc = _dense_out(c, num_rows, b.shape[1], b)
    if 0 < rs.long_spans < num_rows and os.environ.get("MISPMM_NO_HYBRID") != "1":
        st = capi.lib().mispmm_rows_hybrid_f32(_stream_ptr(stream), num_rows, num_cols, nnz, _p(col_idxs), _p(data), _p(rs.spans), num_rows,
                                               rs.long_spans, _p(b), b.shape[1], ldb, _p(c), ldc, mode)
        if st != capi.ERR_UNSUPPORTED:
            capi.check(st)
            return True
    if rs.hybrid_only:
        return False
    st = capi.lib().mispmm_rows_split_f32(_stream_ptr(stream), num_rows, num_cols, nnz, _p(col_idxs), _p(data), _p(rs.spans), num_rows,
                                          _p(b), b.shape[1], ldb, _p(c), ldc, mode)
    if st == capi.ERR_UNSUPPORTED:
        return False
    capi.check(st)
    return True


@dataclass
class DeviceCOO:
    num_rows: int
    num_cols: int
    nnz: int
    row_idxs: torch.Tensor
    col_idxs: torch.Tensor
    data: torch.Tensor
    spans: "RowSpans" = None     # long rows: (row, start, end, 0) per row, longest first -- carries the row boundaries
    row_bounds: torch.Tensor = None   # float64 only: the (M+1) row boundaries of the sorted entries (mispmm_coo_row_bounds)

    @staticmethod
    def from_host(coo, device="cuda", dtype=torch.float32, check=True):
        """Entries sorted by row only, a row's entries in storage order: the reference (spmm_coo.cpp) adds them into the row
        in that order, so sorting them by column as well would change the fp32 sums.  dtype=torch.float64: the values in
        double and the row boundaries built once here, for mispmm_csr_f64; no span list.  check: run check_host first."""
        if check:
            check_host(coo)
        f64 = _check_dtype(dtype)
        order = np.argsort(np.asarray(coo.row_idxs), kind="stable")
        rows = np.asarray(coo.row_idxs)[order]
        if f64:
            a = DeviceCOO(coo.num_rows, coo.num_cols, coo.nnz, _dev_u32(rows, device), _dev_u32(np.asarray(coo.col_idxs)[order], device),
                          _dev_f64(np.asarray(coo.data)[order], device))
            a.row_bounds = coo_row_bounds(a)
            return a
        row_ptrs = np.searchsorted(rows, np.arange(coo.num_rows + 1)).astype(np.uint32)
        return DeviceCOO(coo.num_rows, coo.num_cols, coo.nnz, _dev_u32(rows, device),
                         _dev_u32(coo.col_idxs[order], device), _dev_f32(coo.data[order], device), _row_spans(row_ptrs, device))


def _b_and_out(b, out, num_rows, num_cols, acc, dtype=torch.float32):
    """(N, ldb, C, ldc, mode) of C = A @ B for an A of num_rows x num_cols: b and out checked as the dense operands of
    `dtype` every product takes, acc by name."""
    mode = _acc_mode(acc)
    ldb = _dense(b, "b", dtype, num_cols)
    n = b.shape[1]
    c, ldc = _dense_out(out, num_rows, n, b, dtype)
    return n, ldb, c, ldc, mode


def _spmm_rows_f64(num_rows, num_cols, nnz, row_ptrs, col_idxs, data, b, out, kernel, acc, stream):
    """fp64, every format: C = A @ B from A's row list through mispmm_csr_f64 (REFERENCE: fp64 product, fp64 add in list
    order, bit-exact against the reference's CPU functions with DT = double)."""
    if int(kernel) != 0:
        raise ValueError("float64 operands have one kernel: kernel must be 0")
    n, ldb, c, ldc, mode = _b_and_out(b, out, num_rows, num_cols, acc, torch.float64)
    capi.check(capi.lib().mispmm_csr_f64(_stream_ptr(stream), num_rows, num_cols, nnz, _p(row_ptrs), _p(col_idxs), _p(data), _p(b), n, ldb,
                                         _p(c), ldc, mode))
    return c


def spmm_csr(a, b, out=None, kernel=0, acc="reference", stream=None, use_hint=True):
    """C = A @ B.  a: DeviceCSR, b: [K, N] float32 device tensor, out: [M, N] float32 where given -- both row-major with unit
    column stride and any row stride of at least N (the corner of a larger buffer; a single row may have any stride).
    acc: "reference" or "fast".
    With the default kernel (0 / 5) a CSR whose rows all have the same length goes through
    mispmm_csr_uniform_f32 (no row-pointer fetch), one that carries `spans` (long rows) through mispmm_csr_split_f32 with
    its rows longest first; use_hint=False forces the general entry point.
    A float64 A (DeviceCSR.from_host(..., dtype=torch.float64)) takes mispmm_csr_f64: B and out float64, kernel 0."""
    _require_gpu(a.row_ptrs, b, out)
    if a.data.dtype == torch.float64:
        return _spmm_rows_f64(a.num_rows, a.num_cols, a.nnz, a.row_ptrs, a.col_idxs, a.data, b, out, kernel, acc, stream)
    n, ldb, c, ldc, mode = _b_and_out(b, out, a.num_rows, a.num_cols, acc)
    hints = use_hint and os.environ.get("MISPMM_NO_HINT") != "1"
    if hints and a.plan is not None and int(kernel) in (0, 5) and use_plan(a, n, acc, stream):
        # rows in the clustered order of the plan (same bits: every row keeps its entries in storage order)
        if _csr_plan_launch(a, [b], [c], n, ldb, ldc, mode, stream):
            return c
    if hints and a.uniform_row_nnz and int(kernel) in (0, 5) and a.num_cols * ldb * 4 <= 0x7FFFFFFF:
        capi.check(capi.lib().mispmm_csr_uniform_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.uniform_row_nnz,
                                                     _p(a.col_idxs), _p(a.data), _p(b), n, ldb, _p(c), ldc, mode))
        return c
    # the split kernel with the rows longest first: kernel 6 always, kernel 0 / 5 where the library itself would split
    # (REFERENCE mode: up to 383 columns)
    wants_split = int(kernel) == 6 or (int(kernel) in (0, 5) and (acc == "fast" or n < 384))
    if hints and a.spans is not None and wants_split:
        # kernel 0 / 5: the long rows by the split body and the short rows by the row-gather body of ONE launch, where the
        # shape has such a launch (else, and for kernel 6 by name, the split kernel on the whole list)
        if int(kernel) != 6 and 0 < a.long_spans < a.spans.numel() // 4 and os.environ.get("MISPMM_NO_HYBRID") != "1":
            st = capi.lib().mispmm_csr_hybrid_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(a.col_idxs), _p(a.data),
                                                  _p(a.spans), a.spans.numel() // 4, a.long_spans, _p(b), n, ldb, _p(c), ldc, mode)
            if st != capi.ERR_UNSUPPORTED:
                capi.check(st)
                return c
        if a.spans_hybrid_only and int(kernel) != 6:
            st = capi.ERR_UNSUPPORTED        # short rows on average: the wave-per-row split kernel is not for this matrix
        else:
            st = capi.lib().mispmm_csr_split_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs),
                                                 _p(a.data), _p(a.spans), a.spans.numel() // 4, _p(b), n, ldb, _p(c), ldc, mode)
        if st != capi.ERR_UNSUPPORTED:  # operands that are not 16-byte vectors take the general entry point below
            capi.check(st)
            return c
    capi.check(capi.lib().mispmm_csr_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs),
                                         _p(a.col_idxs), _p(a.data), _p(b), n, ldb, _p(c), ldc, int(kernel), mode))
    return c


def _batch_operands(a, bs, cs, acc, what):
    """(N, ldb, ldc, mode) of cs[i] = A @ bs[i]: both lists checked member by member (float32, A's rows or columns, unit column
    stride, no overlapping rows, one shape and one row stride per list, on the device) and of one length."""
    mode = _acc_mode(acc)
    ldb = _dense_list(bs, "bs", torch.float32, a.num_cols, "A has {} columns")
    n = bs[0].shape[1]
    ldc = _dense_list(cs, what, torch.float32, a.num_rows, "A has {} rows", count=len(bs), cols=n)
    return n, ldb, ldc, mode


def _csr_plan_launch(a, bs, cs, n, ldb, ldc, mode, stream):
    p = a.plan
    blist = (ctypes.c_void_p * len(bs))(*[b.data_ptr() for b in bs])
    clist = (ctypes.c_void_p * len(bs))(*[c.data_ptr() for c in cs])
    st = capi.lib().mispmm_csr_plan_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(p.row_ptrs), _p(p.col_idxs), _p(p.data),
                                        a.uniform_row_nnz, _p(p.row_map), len(bs), blist, n, ldb, clist, ldc, mode)
    if st == capi.ERR_UNSUPPORTED:
        return False
    capi.check(st)
    return True


def _csr_plan(a, bs, cs, acc, stream):
    """mispmm_csr_plan_f32 over the plan's arrays; False = the shape is not taken (B of 2 GiB or more).  a: a DeviceCSR that
    carries a plan; bs: a non-empty list of [K, N] float32 device tensors of one shape and row stride; cs: as many [M, N]
    ones."""
    _require_gpu(a.row_ptrs)
    if a.plan is None or not bs:
        raise ValueError("_csr_plan takes a DeviceCSR with a plan and at least one operand in bs")
    return _csr_plan_launch(a, bs, cs, *_batch_operands(a, bs, cs, acc, "cs"), stream)


def spmm_csr_batch(a, bs, outs=None, acc="reference", stream=None):
    """outs[i] = A @ bs[i] for a list of equally shaped dense operands, ONE launch per 16 of them
    (mispmm_csr_batch_f32).  Returns the list of results.  a: a float32 DeviceCSR; bs: a list of [K, N] float32 device
    tensors that share one shape and one row stride (unit column stride, rows that do not overlap); outs, where given: a list
    of as many [M, N] float32 tensors, again of one row stride."""
    if not bs:
        return []
    _require_gpu(a.row_ptrs)
    if a.data.dtype == torch.float64:
        raise ValueError("spmm_csr_batch multiplies float32 operands only; multiply a float64 A with spmm_csr")
    if outs is None:
        mode, ldb = _acc_mode(acc), _dense_list(bs, "bs", torch.float32, a.num_cols, "A has {} columns")
        n = ldc = bs[0].shape[1]
        outs = [torch.empty((a.num_rows, n), dtype=torch.float32, device=bs[0].device) for _ in bs]
    else:
        n, ldb, ldc, mode = _batch_operands(a, bs, outs, acc, "outs")
    if a.spans is not None:
        # long rows: the library issues one launch per operand anyway (there is no batched split kernel); go through the
        # span list like spmm_csr does, so that both give the same bits in FAST mode as well
        for b, c in zip(bs, outs):
            spmm_csr(a, b, out=c, acc=acc, stream=stream)
        return outs
    if a.plan is not None and os.environ.get("MISPMM_NO_HINT") != "1" and use_plan(a, n, acc, stream):
        if _csr_plan_launch(a, bs, outs, n, ldb, ldc, mode, stream):
            return outs
    blist = (ctypes.c_void_p * len(bs))(*[b.data_ptr() for b in bs])
    clist = (ctypes.c_void_p * len(bs))(*[c.data_ptr() for c in outs])
    capi.check(capi.lib().mispmm_csr_batch_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs),
                                               _p(a.data), a.uniform_row_nnz, len(bs), blist, n, ldb, clist, ldc, mode))
    return outs


def csr_transpose(csr):
    """(formats.CSR of A^T, perm) on the host (mispmm_csr_transpose_host): a stable counting sort of A's entries by column.
    Entry t of A^T is entry perm[t] of A (its data is csr.data[perm]); a row of A^T lists its entries by ascending row of A,
    a column repeated in one row of A in storage order.  perm is uint32."""
    rp = np.ascontiguousarray(csr.row_ptrs, dtype=np.uint32)
    ci = np.ascontiguousarray(csr.col_idxs, dtype=np.uint32)
    nnz = int(ci.shape[0])
    trp = np.zeros(csr.num_cols + 1, dtype=np.uint32)
    tci, perm = np.zeros(nnz, dtype=np.uint32), np.zeros(nnz, dtype=np.uint32)
    capi.check(capi.lib().mispmm_csr_transpose_host(csr.num_rows, csr.num_cols, nnz, rp.ctypes.data, ci.ctypes.data, trp.ctypes.data,
                                                     tci.ctypes.data, perm.ctypes.data))
    return formats.CSR(csr.num_cols, csr.num_rows, trp, tci, np.asarray(csr.data)[perm.astype(np.int64)]), perm


def sddmm_csr(a, x, y, out=None, acc="reference", stream=None):
    """out[e] = <x[row(e), :], y[col(e), :]> for every stored entry e of a (mispmm_sddmm_csr_f32 / _f64): the sampled
    dense-dense product on A's pattern, A's values unread.  a: DeviceCSR [M x K]; x: [M, N], y: [K, N] device tensors of one
    dtype (float32 or float64; row-major, any row stride); returns a tensor of nnz elements in A's storage order."""
    _require_gpu(a.row_ptrs, x, y, out)
    f64 = _check_dtype(x.dtype, "x")
    mode = _acc_mode(acc)
    if y.dtype != x.dtype:
        raise ValueError(f"x and y must be of one dtype, not {x.dtype} and {y.dtype}")
    ldx, ldy = _dense(x, "x", x.dtype), _dense(y, "y", x.dtype)
    if x.shape[0] != a.num_rows or y.shape[0] != a.num_cols or x.shape[1] != y.shape[1]:
        raise ValueError(f"A is {a.num_rows} x {a.num_cols}: x must be [{a.num_rows}, N] and y [{a.num_cols}, N], not "
                         f"{tuple(x.shape)} and {tuple(y.shape)}")
    if out is None:
        out = torch.empty(a.nnz, dtype=x.dtype, device=x.device)
    if out.dtype != x.dtype or out.dim() != 1 or out.shape[0] != a.nnz or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {x.dtype} tensor of {a.nnz} elements")
    fn = capi.lib().mispmm_sddmm_csr_f64 if f64 else capi.lib().mispmm_sddmm_csr_f32
    capi.check(fn(_stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs), _p(x), ldx, _p(y), ldy,
                  x.shape[1], _p(out), mode))
    return out


def _entries(a, t, what):
    """t as an array over A's entries: a contiguous 1-D float32 / float64 device tensor of nnz elements."""
    if t.dim() != 1 or t.shape[0] != a.nnz or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous 1-D tensor of the {a.nnz} entries of A, not {tuple(t.shape)} with strides {tuple(t.stride())}")


def softmax_csr(a, scores, out=None, acc="reference", stream=None):
    """out[e] = exp(scores[e] - m_r) / sum over row r of exp(scores[e'] - m_r), m_r the row's largest score
    (mispmm_softmax_csr_f32 / _f64): the softmax of every row of a's pattern over its stored entries.  a: DeviceCSR, of which
    only row_ptrs, num_rows and nnz are used; scores: nnz elements in A's storage order, float32 or float64.  A -Inf score is
    a masked entry (+0); a row with a NaN, a +Inf or nothing but -Inf is NaN throughout.  out may be scores itself."""
    _require_gpu(a.row_ptrs, scores, out)
    f64 = _check_dtype(scores.dtype, "scores")
    mode = _acc_mode(acc)
    _entries(a, scores, "scores")
    if out is None:
        out = torch.empty_like(scores)
    if out.dtype != scores.dtype:
        raise ValueError(f"out must be {scores.dtype}, like scores")
    _entries(a, out, "out")
    fn = capi.lib().mispmm_softmax_csr_f64 if f64 else capi.lib().mispmm_softmax_csr_f32
    capi.check(fn(_stream_ptr(stream), a.num_rows, a.nnz, _p(a.row_ptrs), _p(scores), _p(out), mode))
    return out


def softmax_csr_bwd(a, p, dp, out=None, acc="reference", stream=None):
    """ds[e] = p[e] * (dp[e] - sum over row r of p[e'] * dp[e']) (mispmm_softmax_csr_bwd_f32 / _f64): the gradient of
    softmax_csr with respect to the scores, given its result p and the gradient dp of that result.  out may be dp itself."""
    _require_gpu(a.row_ptrs, p, dp, out)
    f64 = _check_dtype(p.dtype, "p")
    mode = _acc_mode(acc)
    if dp.dtype != p.dtype:
        raise ValueError(f"dp must be {p.dtype}, like p")
    _entries(a, p, "p")
    _entries(a, dp, "dp")
    if out is None:
        out = torch.empty_like(dp)
    if out.dtype != p.dtype:
        raise ValueError(f"out must be {p.dtype}, like p")
    _entries(a, out, "out")
    fn = capi.lib().mispmm_softmax_csr_bwd_f64 if f64 else capi.lib().mispmm_softmax_csr_bwd_f32
    capi.check(fn(_stream_ptr(stream), a.num_rows, a.nnz, _p(a.row_ptrs), _p(p), _p(dp), _p(out), mode))
    return out


ATTN_CSR_MAX_WIDTH = 256     # D and Dv of the fused CSR attention kernel: 1 up to this (mispmm_attn_csr.h)


def attention_csr(a, q, k, v, scale=None, bias=None, return_lse=False, out=None, lse=None, stream=None):
    """Fused attention on a CSR pattern (mispmm_attn_csr_f32, libmispmm_attn_csr.so): for every head, out = softmax over each
    row's stored entries of (scale * <q_r, k_c> + bias), times v -- one launch for all heads, neither the scores nor the
    weights written.  a: a float32 DeviceCSR [M x K] (index arrays used, values unread); q: [M, D], k: [K, D], v: [K, Dv]
    float32, or [H, ...] with any head and row strides and unit column stride (a permuted [M, H, D]; k, v expanded over the
    heads for multi-query attention); D and Dv from 1 to 256.  scale defaults to D ** -0.5.  bias: float32 [nnz], shared by
    the heads, or [H, nnz], in A's entry order, added to the scaled scores, -Inf = masked.  Returns out, [M, Dv] or
    [H, M, Dv]; with return_lse (out, lse), lse the [M] or [H, M] log-sum-exp of each row.  out= and lse= take the results
    where given: out of the result's shape with unit column stride, lse contiguous."""
    from . import _attn_csr
    _require_gpu(a.row_ptrs, q, k, v, bias, out, lse)
    return _attn_csr.forward("attention_csr", _attn_csr.F32, a, q, k, v, scale, bias, False, return_lse, out, lse, stream)


def attention_csr_bwd(a, at, perm, q, k, v, out, lse, grad_out, scale=None, bias=None, need=(True, True, True), dq=None, dk=None, dv=None,
                      delta=None, stream=None):
    """Fused backward of attention_csr (mispmm_attn_csr_bwd_f32, libmispmm_attn_csr_bwd.so): (dq, dk, dv) for every head in at
    most two launches, the scores, the weights and their gradients never written.  a: the forward's DeviceCSR; at, perm: A^T's
    pattern and the permutation of its entries (csr_transpose; TrainableCSR.tpattern / .perm32()), perm an integer device
    tensor (int64 is converted to 32 bits here: hand in int32 to avoid the copy), read only with a bias.  q, k, v, scale, bias:
    as in the forward; out, lse: what the forward returned; grad_out: float32 of out's shape.  2-D or [H, ...] operands with
    any head and row strides and unit column stride.  need: which of (dq, dk, dv) to compute; the others come back None and
    their work is skipped.  dk and dv are [H, K, ...] also where k and v are one head expanded over all.  dq= / dk= / dv= take
    the gradients where given.  delta: a contiguous float32 workspace of lse's shape, allocated here unless given; needed
    for dq and dk."""
    from . import _attn_csr
    _require_gpu(a.row_ptrs, at.row_ptrs, perm, q, k, v, out, lse, grad_out, bias, dq, dk, dv, delta)
    return _attn_csr.backward("attention_csr_bwd", _attn_csr.F32, a, at, perm, q, k, v, out, lse, grad_out, scale, bias, need, False, dq, dk, dv,
                              delta, stream)


@dataclass
class DeviceCSRTiles:
    """A CSR with rows of one width grouped into LDS tiles (mispmm_csr_tiles_host): rows that share B rows sit in one tile of
    <= 16 rows / <= 128 distinct columns, an entry names its column by its position in the tile's list."""
    num_rows: int
    num_cols: int
    nnz: int
    row_nnz: int
    num_tiles: int
    num_listed: int              # sum of the tiles' column lists = B-row slices staged per column part (nnz without sharing)
    max_tile_cols: int           # the longest column list of a tile (the kernel declines lists longer than its LDS image)
    tile_row_ptrs: torch.Tensor
    tile_col_ptrs: torch.Tensor
    tile_cols: torch.Tensor
    slots: torch.Tensor          # uint8 per entry, plan order
    data: torch.Tensor           # values, plan order
    row_map: torch.Tensor        # plan position -> C row

    @staticmethod
    def from_host(csr, device="cuda", max_rows=16, max_cols=128, check=True):
        if check:
            check_host(csr)
        w = uniform_row_nnz(csr.row_ptrs)
        if w == 0 or w > 16:
            raise ValueError("LDS tiles take rows of one width of 1..16 entries")
        l = capi.lib()
        rp = np.ascontiguousarray(csr.row_ptrs, dtype=np.uint32)
        ci = np.ascontiguousarray(csr.col_idxs, dtype=np.uint32)
        nt, nl = ctypes.c_uint32(0), ctypes.c_uint32(0)
        head = (csr.num_rows, csr.num_cols, rp.ctypes.data, ci.ctypes.data, int(max_rows), int(max_cols), ctypes.byref(nt), ctypes.byref(nl))
        capi.check(l.mispmm_csr_tiles_host(*head, None, None, None, None, None))
        trp, tcp = np.zeros(nt.value + 1, np.uint32), np.zeros(nt.value + 1, np.uint32)
        tc, order, slots = np.zeros(max(nl.value, 1), np.uint32), np.zeros(csr.num_rows, np.uint32), np.zeros(max(csr.nnz, 1), np.uint8)
        capi.check(l.mispmm_csr_tiles_host(*head, trp.ctypes.data, tcp.ctypes.data, tc.ctypes.data, order.ctypes.data, slots.ctypes.data))
        planned = permute_rows(csr, order)
        widest = int(np.diff(tcp.astype(np.int64)).max()) if nt.value else 0
        return DeviceCSRTiles(csr.num_rows, csr.num_cols, csr.nnz, w, nt.value, nl.value, widest, _dev_u32(trp, device), _dev_u32(tcp, device),
                              _dev_u32(tc, device), torch.from_numpy(slots).to(device), _dev_f32(planned.data, device), _dev_u32(order, device))


def spmm_csr_tiles(a, b, out=None, acc="reference", stream=None):
    """C = A @ B with the B rows of every tile staged in LDS (mispmm_csr_lds_tile_f32): a: DeviceCSRTiles; b, out and
    acc as spmm_csr takes them (float32, unit column stride, any row stride of at least N)."""
    _require_gpu(a.tile_row_ptrs, b)
    n, ldb, c, ldc, mode = _b_and_out(b, out, a.num_rows, a.num_cols, acc)
    capi.check(capi.lib().mispmm_csr_lds_tile_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.row_nnz, a.num_tiles, a.max_tile_cols,
                                                  _p(a.tile_row_ptrs), _p(a.tile_col_ptrs), _p(a.tile_cols), _p(a.slots), _p(a.data),
                                                  _p(a.row_map), _p(b), n, ldb, _p(c), ldc, mode))
    return c


@dataclass
class DeviceCSRPanels:
    """A CSR plus, per row, where its entries of each panel of `panel_rows` consecutive B rows start (mispmm_csr_panels_host):
    what mispmm_csr_panel_f32 walks.  The entries stay in the matrix's own order; rows must ascend in column."""
    num_rows: int
    num_cols: int
    nnz: int
    panel_rows: int
    num_panels: int
    row_ptrs: torch.Tensor
    col_idxs: torch.Tensor
    data: torch.Tensor
    panel_ptrs: torch.Tensor     # num_rows x (num_panels + 1) offsets into col_idxs / data, row-major

    @staticmethod
    def from_host(csr, device="cuda", panel_rows=None, check=True):
        """Raises capi.MispmmError for a matrix the builder declines (a row whose columns do not ascend: ERR_UNSUPPORTED)."""
        if check:
            check_host(csr)
        l = capi.lib()
        depth = int(panel_rows) if panel_rows is not None else l.mispmm_csr_panel_rows()
        rp = np.ascontiguousarray(csr.row_ptrs, dtype=np.uint32)
        ci = np.ascontiguousarray(csr.col_idxs, dtype=np.uint32)
        npan, noff = ctypes.c_uint32(0), ctypes.c_uint64(0)
        head = (csr.num_rows, csr.num_cols, rp.ctypes.data, ci.ctypes.data, depth, ctypes.byref(npan), ctypes.byref(noff))
        capi.check(l.mispmm_csr_panels_host(*head, None, 0))
        pp = np.zeros(max(noff.value, 1), np.uint32)
        capi.check(l.mispmm_csr_panels_host(*head, pp.ctypes.data, pp.shape[0]))
        return DeviceCSRPanels(csr.num_rows, csr.num_cols, csr.nnz, depth, npan.value, _dev_u32(rp, device), _dev_u32(ci, device),
                               _dev_f32(csr.data, device), _dev_u32(pp, device))


def spmm_csr_panels(a, b, out=None, acc="reference", stream=None):
    """C = A @ B with B staged panel by panel in LDS (mispmm_csr_panel_f32, for dense-regime A): a: DeviceCSRPanels; b, out
    and acc as spmm_csr takes them (float32, unit column stride, any row stride of at least N)."""
    _require_gpu(a.panel_ptrs, b)
    n, ldb, c, ldc, mode = _b_and_out(b, out, a.num_rows, a.num_cols, acc)
    capi.check(capi.lib().mispmm_csr_panel_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(a.row_ptrs), _p(a.col_idxs),
                                               _p(a.data), _p(a.panel_ptrs), a.panel_rows, _p(b), n, ldb, _p(c), ldc,
                                               mode))
    return c


def spmm_ell(a, b, out=None, kernel=0, acc="reference", stream=None):
    """C = A @ B for a DeviceELL (mispmm_ell_f32; the list of occupied slots where the upload made one).  b, out and acc as
    spmm_csr takes them: [K, N] and [M, N] float32, unit column stride, any row stride of at least N.  A float64 A takes
    mispmm_csr_f64: B and out float64, kernel 0."""
    _require_gpu(a.col_idxs, b)
    if a.data.dtype == torch.float64:
        nnz, rp, ci, va, _ = a.compact
        return _spmm_rows_f64(a.num_rows, a.num_cols, nnz, rp, ci, va, b, out, kernel, acc, stream)
    n, ldb, c, ldc, mode = _b_and_out(b, out, a.num_rows, a.num_cols, acc)
    if a.compact is not None and int(kernel) in (0, 1):   # mostly padding: multiply from the list of occupied slots
        nnz, rp, ci, va, spans = a.compact
        if _rows_split(spans, a.num_rows, a.num_cols, nnz, ci, va, b, c, acc, stream):
            return c
        st = capi.lib().mispmm_ell_compact_f32(_stream_ptr(stream), a.num_rows, a.num_cols, nnz, _p(rp), _p(ci), _p(va), _p(b), n,
                                               ldb, _p(c), ldc, mode)
        if st != capi.ERR_UNSUPPORTED:
            capi.check(st)
            return c
    capi.check(capi.lib().mispmm_ell_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.width, _p(a.col_idxs),
                                         _p(a.data), _p(b), n, ldb, _p(c), ldc, int(kernel),
                                         mode))
    return c


def spmm_bsr(a, b, out=None, kernel=0, acc="reference", stream=None):
    """C = A @ B for a DeviceBSR of float32 blocks (mispmm_bsr_f32).  b, out and acc as spmm_csr takes them: [K, N] and [M, N]
    float32, unit column stride, any row stride of at least N."""
    _require_gpu(a.block_row_ptrs, b)
    n, ldb, c, ldc, mode = _b_and_out(b, out, a.num_rows, a.num_cols, acc)
    capi.check(capi.lib().mispmm_bsr_f32(_stream_ptr(stream), a.num_rows // a.block_row_size, a.num_cols,
                                         a.block_row_size, a.block_col_size, a.num_blocks, _p(a.block_row_ptrs),
                                         _p(a.block_col_idxs), _p(a.data), _p(b), n, ldb, _p(c), ldc,
                                         int(kernel), mode))
    return c


def bsr_nonzeros(bsr, device="cuda", dtype=torch.float32, check=True):
    """The non-zero block entries of a host BSR as a DeviceCSR in the reference's order of addition
    (mispmm_bsr_nonzeros_host) -- the once-per-upload analysis step of the zero-skipping BSR path.  dtype=torch.float64:
    the values in double (mispmm_bsr_nonzeros_f64_host), for mispmm_csr_f64; no span list.  check: run check_host first -- the
    builders themselves cannot (their signatures carry no K)."""
    if check:
        check_host(bsr)
    if _check_dtype(dtype):
        rp, ci, va = bsr_nonzeros_f64_host(bsr)
        return DeviceCSR(bsr.num_rows, bsr.num_cols, int(rp[-1]), _dev_u32(rp, device), _dev_u32(ci, device), _dev_f64(va, device))
    l = capi.lib()
    ptrs = np.ascontiguousarray(bsr.block_row_ptrs, dtype=np.uint32)
    cols = np.ascontiguousarray(bsr.block_col_idxs, dtype=np.uint32)
    data = np.ascontiguousarray(bsr.data, dtype=np.float32).reshape(-1)
    nnz = ctypes.c_uint32(0)
    args = (bsr.num_block_rows, bsr.block_row_size, bsr.block_col_size, bsr.num_blocks, ptrs.ctypes.data, cols.ctypes.data,
            data.ctypes.data, ctypes.byref(nnz))
    capi.check(l.mispmm_bsr_nonzeros_host(*args, None, None, None))
    rp = np.empty(bsr.num_rows + 1, dtype=np.uint32)
    ci = np.empty(max(1, nnz.value), dtype=np.uint32)
    va = np.empty(max(1, nnz.value), dtype=np.float32)
    capi.check(l.mispmm_bsr_nonzeros_host(*args, rp.ctypes.data, ci.ctypes.data, va.ctypes.data))
    return DeviceCSR(bsr.num_rows, bsr.num_cols, nnz.value, _dev_u32(rp, device), _dev_u32(ci[:nnz.value], device),
                     _dev_f32(va[:nnz.value], device), 0, _row_spans(rp, device))


def spmm_bsr_nonzeros(nz, b, out=None, acc="reference", stream=None):
    """C = A @ B from the non-zero list of a BSR (bsr_nonzeros): fp32 product, fp32 add in the reference's order.  A float64
    list takes mispmm_csr_f64: B and out float64.  b, out and acc as spmm_csr takes them."""
    _require_gpu(nz.row_ptrs, b)
    if nz.data.dtype == torch.float64:
        return _spmm_rows_f64(nz.num_rows, nz.num_cols, nz.nnz, nz.row_ptrs, nz.col_idxs, nz.data, b, out, 0, acc, stream)
    n, ldb, c, ldc, mode = _b_and_out(b, out, nz.num_rows, nz.num_cols, acc)
    if _rows_split(nz.spans, nz.num_rows, nz.num_cols, nz.nnz, nz.col_idxs, nz.data, b, c, acc, stream):
        return c
    capi.check(capi.lib().mispmm_bsr_nonzeros_f32(_stream_ptr(stream), nz.num_rows, nz.num_cols, nz.nnz, _p(nz.row_ptrs),
                                                  _p(nz.col_idxs), _p(nz.data), _p(b), n, ldb, _p(c), ldc,
                                                  mode))
    return c


def coo_row_bounds(a, stream=None):
    """The (M+1)-entry row-boundary array of a row-sorted device COO (the once-per-upload analysis step)."""
    _require_gpu(a.row_idxs)
    ws = torch.empty(a.num_rows + 1, dtype=torch.int32, device=a.row_idxs.device)
    capi.check(capi.lib().mispmm_coo_row_bounds(_stream_ptr(stream), a.num_rows, a.nnz, _p(a.row_idxs), _p(ws)))
    return ws


def spmm_coo(a, b, out=None, kernel=0, acc="reference", stream=None, workspace=True):
    """workspace=True allocates the (M+1)-entry row-boundary scratch; False uses binary search; a tensor from
    coo_row_bounds() is used as is (pass kernel=2 to skip rebuilding it): a contiguous int32 device tensor of at least M + 1
    elements, which the kernel writes.  b, out, acc: as in spmm_csr.  A float64 A takes mispmm_csr_f64 over its row
    boundaries: B and out float64, kernel 0."""
    _require_gpu(a.row_idxs, b, out)
    if a.data.dtype == torch.float64:
        return _spmm_rows_f64(a.num_rows, a.num_cols, a.nnz, a.row_bounds, a.col_idxs, a.data, b, out, kernel, acc, stream)
    n, ldb, c, ldc, mode = _b_and_out(b, out, a.num_rows, a.num_cols, acc)
    if isinstance(workspace, torch.Tensor):
        _require_gpu(workspace)
        _flat(workspace, "workspace", torch.int32, a.num_rows + 1, exact=False)
        ws = workspace
    else:
        ws = torch.empty(a.num_rows + 1, dtype=torch.int32, device=b.device) if workspace else None
    if workspace is not False and int(kernel) in (0, 1, 2) and _rows_split(a.spans, a.num_rows, a.num_cols, a.nnz, a.col_idxs, a.data, b, c, acc, stream):
        return c
    capi.check(capi.lib().mispmm_coo_f32(_stream_ptr(stream), a.num_rows, a.num_cols, a.nnz, _p(a.row_idxs),
                                         _p(a.col_idxs), _p(a.data), _p(b), n, ldb, _p(c), ldc,
                                         _p(ws), int(kernel), mode))
    return c


def f32_to_bf16(x, stream=None):
    """Device fp32 tensor -> int16 tensor of bf16 bit patterns (round to nearest even).  x: float32 of any shape; a view that
    is not contiguous is copied first."""
    _require_gpu(x)
    if x.dtype != torch.float32:
        raise ValueError(f"x must be a float32 tensor, not {x.dtype}")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    capi.check(capi.lib().mispmm_f32_to_bf16(_stream_ptr(stream), x.numel(), _p(x), _p(out)))
    return out


def bf16_to_f32(x, stream=None):
    """Device int16 tensor of bf16 bit patterns -> fp32 tensor.  x: int16 of any shape; a view that is not contiguous is
    copied first."""
    _require_gpu(x)
    if x.dtype != torch.int16:
        raise ValueError(f"x must be an int16 tensor of bf16 bits, not {x.dtype}")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    capi.check(capi.lib().mispmm_bf16_to_f32(_stream_ptr(stream), x.numel(), _p(x), _p(out)))
    return out


def spmm_bsr_bf16(a, blocks_bf16, b_bf16, out_bf16=False, out=None, stream=None):
    """C = A @ B on MFMA (mispmm_bsr_bf16).  a: DeviceBSR [M x K] (index arrays used); blocks_bf16: A's blocks as a contiguous
    int16 tensor of bf16 bits, num_blocks * bS * bS elements in A's block order; b_bf16: [K, N] int16 tensor of bf16 bits, unit
    column stride, any row stride of at least N.  Returns [M, N] float32, or int16 bf16 bits with out_bf16; out= takes the
    result where given: that shape and dtype, unit column stride, any row stride of at least N."""
    _require_gpu(a.block_row_ptrs, blocks_bf16, b_bf16, out)
    _flat(blocks_bf16, "blocks_bf16", torch.int16, a.num_blocks * a.block_row_size * a.block_col_size)
    n, ldb, out, ldc = _bf16_b_and_out(b_bf16, out_bf16, out, a.num_rows, a.num_cols)
    capi.check(capi.lib().mispmm_bsr_bf16(_stream_ptr(stream), a.num_rows // a.block_row_size, a.num_cols,
                                          a.block_row_size, a.block_col_size, a.num_blocks, _p(a.block_row_ptrs),
                                          _p(a.block_col_idxs), _p(blocks_bf16), _p(b_bf16), n, ldb, _p(out), ldc, int(bool(out_bf16))))
    return out


def _bf16_ld(t, what):
    return _dense(t, what, torch.int16)


def _bf16_b_and_out(b_bf16, out_bf16, out, num_rows, num_cols):
    """(N, ldb, C, ldc) of C = A @ B with B in bf16 bits for an A of num_rows x num_cols; C float32, or int16 with out_bf16."""
    ldb = _dense(b_bf16, "b_bf16", torch.int16, num_cols)
    n = b_bf16.shape[1]
    c, ldc = _dense_out(out, num_rows, n, b_bf16, torch.int16 if out_bf16 else torch.float32)
    return n, ldb, c, ldc


def sddmm_bsr_bf16(a, x_bf16, y_bf16, out_bf16=False, out=None, stream=None):
    """out[e][i][j] = <x[R * bS + i, :], y[c * bS + j, :]> for every stored block e of a, R its block row and c its block column
    (mispmm_sddmm_bsr_bf16): the sampled dense-dense product on A's block pattern, A's values unread.  a: DeviceBSR
    [M x K] of 16 x 16 or 32 x 32 blocks (index arrays used); x_bf16: [M, N], y_bf16: [K, N] int16 tensors of bf16 bits
    (row-major, any row stride); returns [num_blocks, bS, bS] in A's block order, float32, or int16 bf16 bits with out_bf16."""
    _require_gpu(a.block_row_ptrs, x_bf16, y_bf16, out)
    ldx, ldy = _bf16_ld(x_bf16, "x_bf16"), _bf16_ld(y_bf16, "y_bf16")
    bs = a.block_row_size
    if a.block_col_size != bs:
        raise ValueError(f"blocks must be square, not {bs} x {a.block_col_size}")
    if x_bf16.shape[0] != a.num_rows or y_bf16.shape[0] != a.num_cols or x_bf16.shape[1] != y_bf16.shape[1]:
        raise ValueError(f"A is {a.num_rows} x {a.num_cols}: x_bf16 must be [{a.num_rows}, N] and y_bf16 [{a.num_cols}, N], not "
                         f"{tuple(x_bf16.shape)} and {tuple(y_bf16.shape)}")
    dtype = torch.int16 if out_bf16 else torch.float32
    if out is None:
        out = torch.empty((a.num_blocks, bs, bs), dtype=dtype, device=x_bf16.device)
    if out.dtype != dtype or tuple(out.shape) != (a.num_blocks, bs, bs) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {dtype} tensor of shape {(a.num_blocks, bs, bs)}")
    capi.check(capi.lib().mispmm_sddmm_bsr_bf16(_stream_ptr(stream), a.num_rows // bs, a.num_cols, bs, a.num_blocks,
                                                _p(a.block_row_ptrs), _p(a.block_col_idxs), _p(x_bf16), ldx, _p(y_bf16), ldy,
                                                x_bf16.shape[1], _p(out), int(bool(out_bf16))))
    return out


def _block_array(a, t, dtypes, what):
    """t as an array over A's block elements: a contiguous [num_blocks, bS, bS] device tensor of one of `dtypes`."""
    bs = a.block_row_size
    if t.dtype not in dtypes or tuple(t.shape) != (a.num_blocks, bs, bs) or not t.is_contiguous():
        names = " or ".join(str(d) for d in dtypes)
        raise ValueError(f"{what} must be a contiguous {names} tensor of shape {(a.num_blocks, bs, bs)}, not {t.dtype} {tuple(t.shape)} "
                         f"with strides {tuple(t.stride())}")


def _square_blocks(a):
    if a.block_col_size != a.block_row_size:
        raise ValueError(f"blocks must be square, not {a.block_row_size} x {a.block_col_size}")


def softmax_bsr(a, scores, scale=1.0, mask=None, out_bf16=False, out=None, stream=None):
    """out = softmax over every matrix row of z = scale * scores + mask (one fp32 fma; without a mask the product), a row
    being element row i of all blocks of a block row (mispmm_softmax_bsr_f32).  a: DeviceBSR of 16 x 16 or 32 x 32 blocks, of
    which only block_row_ptrs and the sizes are used; scores and mask: float32 [num_blocks, bS, bS] in A's block order, as
    sddmm_bsr_bf16 writes them; a -Inf in mask is a masked position (+0).  Returns [num_blocks, bS, bS] float32, or int16 bf16
    bits with out_bf16 -- the blocks spmm_bsr_bf16 takes.  out must not overlap scores or mask."""
    _require_gpu(a.block_row_ptrs, scores, mask, out)
    _square_blocks(a)
    _block_array(a, scores, (torch.float32,), "scores")
    if mask is not None:
        _block_array(a, mask, (torch.float32,), "mask")
    dtype = torch.int16 if out_bf16 else torch.float32
    if out is None:
        out = torch.empty(scores.shape, dtype=dtype, device=scores.device)
    _block_array(a, out, (dtype,), "out")
    bs = a.block_row_size
    capi.check(capi.lib().mispmm_softmax_bsr_f32(_stream_ptr(stream), a.num_rows // bs, bs, a.num_blocks, _p(a.block_row_ptrs),
                                                 _p(scores), _p(mask), float(scale), _p(out), int(bool(out_bf16))))
    return out


def softmax_bsr_bwd(a, p, dp, scale=1.0, out_bf16=False, out=None, stream=None):
    """ds = scale * p * (dp - sum over the matrix row of p * dp) (mispmm_softmax_bsr_bwd_f32): the gradient of softmax_bsr
    with respect to the scores, given its result p (float32, or int16 bf16 bits: the dtype says which) and the float32
    gradient dp of that result.  Returns float32, or int16 bf16 bits with out_bf16.  out must not overlap p or dp."""
    _require_gpu(a.block_row_ptrs, p, dp, out)
    _square_blocks(a)
    _block_array(a, p, (torch.float32, torch.int16), "p")
    _block_array(a, dp, (torch.float32,), "dp")
    dtype = torch.int16 if out_bf16 else torch.float32
    if out is None:
        out = torch.empty(dp.shape, dtype=dtype, device=dp.device)
    _block_array(a, out, (dtype,), "out")
    bs = a.block_row_size
    capi.check(capi.lib().mispmm_softmax_bsr_bwd_f32(_stream_ptr(stream), a.num_rows // bs, bs, a.num_blocks, _p(a.block_row_ptrs),
                                                     _p(p), int(p.dtype == torch.int16), _p(dp), float(scale), _p(out), int(bool(out_bf16))))
    return out


ATTN_MAX_WIDTH = 128     # D and Dv of the fused attention kernel: multiples of 8 up to this (mispmm_attn.h)


def _attn_operand(t, rows, heads, what):
    """(t as [H, rows, width], row stride, head stride) of a bf16-bits operand given as [rows, width] or [H, rows, width]."""
    if t.dtype != torch.int16 or t.dim() not in (2, 3):
        raise ValueError(f"{what} must be an int16 tensor of bf16 bits, [{rows}, width] or [H, {rows}, width], not {t.dtype} {tuple(t.shape)}")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.shape[1] != rows or (heads is not None and t.shape[0] != heads):
        raise ValueError(f"{what} must be [{rows}, width] or [{'H' if heads is None else heads}, {rows}, width], not {tuple(t.shape)}")
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError(f"{what} must have a contiguous last dimension")
    width = t.shape[2]
    ld = t.stride(1) if rows > 1 else max(width, t.stride(1))
    if ld < width or any(s < 0 for s in t.stride()):
        raise ValueError(f"{what} must not overlap its own rows (row stride {ld} < {width} columns), e.g. an expanded tensor")
    return t, ld, (t.stride(0) if t.shape[0] > 1 else 0)


def attention_bsr_bf16(a, q, k, v, scale=None, mask=None, out_bf16=False, return_lse=False, out=None, lse=None, stream=None):
    """Fused block-sparse attention forward (mispmm_attn_bsr_bf16, libmispmm_attn.so): for every head, out = softmax over each
    matrix row of (scale * q k^T + mask) on A's stored blocks, times v -- one launch for all heads, the scores and the weights
    never written.  a: DeviceBSR [M x K] of 16 x 16 or 32 x 32 blocks (index arrays used); q: [M, D], k: [K, D], v: [K, Dv]
    int16 tensors of bf16 bits, or [H, ...] with any head and row strides whose last dimension is contiguous (e.g. a permuted
    [M, H, D]); D and Dv multiples of 8 up to 128.  scale defaults to D ** -0.5; mask: float32 [num_blocks, bS, bS], added to
    the scaled scores, -Inf = masked, shared by the heads.  Returns out, [M, Dv] or [H, M, Dv], float32 or int16 bf16 bits
    with out_bf16; with return_lse (out, lse), lse the float32 [M] or [H, M] log-sum-exp of each row.  out= and lse= take
    the results where given: out of the result's shape with a contiguous last dimension, lse contiguous."""
    from . import capi_attn
    _require_gpu(a.block_row_ptrs, q, k, v, mask, out, lse)
    _square_blocks(a)
    bs = a.block_row_size
    if q.dim() != k.dim() or q.dim() != v.dim():
        raise ValueError(f"q, k and v must all be 2-D or all [H, ...], not {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    batched = q.dim() == 3
    q3, ldq, q_head = _attn_operand(q, a.num_rows, None, "q")
    heads = q3.shape[0]
    k3, ldk, k_head = _attn_operand(k, a.num_cols, heads, "k")
    v3, ldv, v_head = _attn_operand(v, a.num_cols, heads, "v")
    d, dv = q3.shape[2], v3.shape[2]
    if k3.shape[2] != d:
        raise ValueError(f"q and k must have the same number of columns, not {d} and {k3.shape[2]}")
    for width, what in ((d, "D"), (dv, "Dv")):
        if width == 0 or width % 8 != 0 or width > ATTN_MAX_WIDTH:
            raise ValueError(f"the fused attention kernel takes {what} in multiples of 8 up to {ATTN_MAX_WIDTH}, not {width}")
    if mask is not None:
        _block_array(a, mask, (torch.float32,), "mask")
    if scale is None:
        scale = d ** -0.5
    dtype = torch.int16 if out_bf16 else torch.float32
    shape = (heads, a.num_rows, dv)
    if out is None:
        out3 = torch.empty(shape, dtype=dtype, device=q.device)
    else:
        out3 = out if batched else out.unsqueeze(0)
        if out.dtype != dtype or tuple(out3.shape) != shape or (dv > 1 and out3.stride(2) != 1) or out3.stride(1) < dv:
            raise ValueError(f"out must be a {dtype} tensor of shape {shape if batched else shape[1:]} with a contiguous last dimension")
    want_lse = return_lse or lse is not None
    if lse is None and want_lse:
        lse = torch.empty((heads, a.num_rows) if batched else (a.num_rows,), dtype=torch.float32, device=q.device)
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != ((heads, a.num_rows) if batched else (a.num_rows,))
                            or not lse.is_contiguous()):
        raise ValueError(f"lse must be a contiguous float32 tensor of shape {(heads, a.num_rows) if batched else (a.num_rows,)}")
    o_head = out3.stride(0) if heads > 1 else 0
    capi_attn.check(capi_attn.lib().mispmm_attn_bsr_bf16(
        _stream_ptr(stream), heads, a.num_rows // bs, a.num_cols, bs, a.num_blocks, _p(a.block_row_ptrs), _p(a.block_col_idxs),
        _p(q3), ldq, q_head, _p(k3), ldk, k_head, _p(v3), ldv, v_head, d, dv, _p(mask), float(scale), _p(out3), out3.stride(1), o_head,
        int(bool(out_bf16)), _p(lse)))
    result = out if out is not None else (out3 if batched else out3[0])
    return (result, lse) if return_lse else result


def _attn_result(t, shape, batched, bf16, what):
    """(t as [H, rows, width], row stride, head stride) of a float32 / bf16-bits tensor the backward reads or writes."""
    dtype = torch.int16 if bf16 else torch.float32
    t3 = t if batched else t.unsqueeze(0)
    if t.dtype != dtype or t.dim() != (3 if batched else 2) or tuple(t3.shape) != shape or (shape[2] > 1 and t3.stride(2) != 1) \
            or (shape[1] > 1 and t3.stride(1) < shape[2]):
        raise ValueError(f"{what} must be a {dtype} tensor of shape {shape if batched else shape[1:]} with a contiguous last dimension, "
                         f"not {t.dtype} {tuple(t.shape)} with strides {tuple(t.stride())}")
    return t3, (t3.stride(1) if shape[1] > 1 else max(shape[2], t3.stride(1))), (t3.stride(0) if shape[0] > 1 else 0)


def attention_bsr_bwd_bf16(a, at, perm, q, k, v, out, lse, grad_out, scale=None, mask=None, grads_bf16=True, need=(True, True, True),
                           dq=None, dk=None, dv=None, delta=None, stream=None):
    """Fused backward of attention_bsr_bf16 (mispmm_attn_bsr_bwd_bf16, libmispmm_attn_bwd.so): (dq, dk, dv) for every head in
    at most two launches, the scores, the weights and their gradients never written.  a: the forward's DeviceBSR; at, perm:
    A^T's pattern and the permutation of its blocks (bsr_transpose; TrainableBSR.tpattern / .perm), perm an integer device
    tensor (int64 is converted to 32 bits here: hand in int32 to avoid the copy), read only with a mask.  q, k, v: as in the
    forward; out, lse: what the forward returned (out float32 or int16 bf16 bits, lse float32 contiguous); grad_out: int16
    bf16 bits of out's shape.  2-D or [H, ...] operands with any strides whose last dimension is contiguous.  need: which of
    (dq, dk, dv) to compute; the others come back None and their work is skipped.  The gradients are int16 bf16 bits
    (grads_bf16, the fp32 sums rounded once) or float32; dq= / dk= / dv= take them where given.  delta: a contiguous float32
    workspace of lse's shape, allocated here unless given."""
    from . import capi_attn_bwd
    _require_gpu(a.block_row_ptrs, at.block_row_ptrs, perm, q, k, v, out, lse, grad_out, mask, dq, dk, dv, delta)
    _square_blocks(a)
    bs = a.block_row_size
    if (at.block_row_size, at.block_col_size, at.num_rows, at.num_cols, at.num_blocks) != (bs, bs, a.num_cols, a.num_rows, a.num_blocks):
        raise ValueError(f"at must be the pattern of A^T: {a.num_cols} x {a.num_rows} of {a.num_blocks} {bs} x {bs} blocks")
    if len({q.dim(), k.dim(), v.dim(), out.dim(), grad_out.dim()}) != 1:
        raise ValueError("q, k, v, out and grad_out must all be 2-D or all [H, ...]")
    batched = q.dim() == 3
    q3, ldq, q_head = _attn_operand(q, a.num_rows, None, "q")
    heads = q3.shape[0]
    k3, ldk, k_head = _attn_operand(k, a.num_cols, heads, "k")
    v3, ldv, v_head = _attn_operand(v, a.num_cols, heads, "v")
    g3, ldg, g_head = _attn_operand(grad_out, a.num_rows, heads, "grad_out")
    d, dvw = q3.shape[2], v3.shape[2]
    if k3.shape[2] != d:
        raise ValueError(f"q and k must have the same number of columns, not {d} and {k3.shape[2]}")
    if g3.shape[2] != dvw:
        raise ValueError(f"grad_out must have v's {dvw} columns, not {g3.shape[2]}")
    for width, what in ((d, "D"), (dvw, "Dv")):
        if width == 0 or width % 8 != 0 or width > ATTN_MAX_WIDTH:
            raise ValueError(f"the fused attention kernel takes {what} in multiples of 8 up to {ATTN_MAX_WIDTH}, not {width}")
    if out.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"out must be the forward's result, float32 or int16 bf16 bits, not {out.dtype}")
    out_bf16 = out.dtype == torch.int16
    o3, ldo, o_head = _attn_result(out, (heads, a.num_rows, dvw), batched, out_bf16, "out")
    rows_shape = (heads, a.num_rows) if batched else (a.num_rows,)
    if lse.dtype != torch.float32 or tuple(lse.shape) != rows_shape or not lse.is_contiguous():
        raise ValueError(f"lse must be a contiguous float32 tensor of shape {rows_shape}")
    if mask is not None:
        _block_array(a, mask, (torch.float32,), "mask")
    if len(need) != 3:
        raise ValueError("need holds three flags: (dq, dk, dv)")
    if perm is not None:
        if perm.dtype not in (torch.int32, torch.int64) or perm.numel() != a.num_blocks:
            raise ValueError(f"perm must hold {a.num_blocks} int32 or int64 block numbers")
        if perm.dtype == torch.int64:
            perm = perm.to(torch.int32)
        perm = perm.contiguous()
    elif mask is not None and (need[1] or need[2]):
        raise ValueError("with a mask, dk and dv need perm")
    if scale is None:
        scale = d ** -0.5
    grads = []
    for wanted, given, rows, width, what in ((need[0], dq, a.num_rows, d, "dq"), (need[1], dk, a.num_cols, d, "dk"), (need[2], dv, a.num_cols, dvw, "dv")):
        if not wanted:
            grads.append((None, None, 0, 0))
            continue
        shape = (heads, rows, width)
        if given is None:
            given = torch.empty(shape if batched else shape[1:], dtype=torch.int16 if grads_bf16 else torch.float32, device=q.device)
        t3, ld, head = _attn_result(given, shape, batched, grads_bf16, what)
        grads.append((given, t3, ld, head))
    if need[0] or need[1]:
        if delta is None:
            delta = torch.empty(rows_shape, dtype=torch.float32, device=q.device)
        elif delta.dtype != torch.float32 or tuple(delta.shape) != rows_shape or not delta.is_contiguous():
            raise ValueError(f"delta must be a contiguous float32 tensor of shape {rows_shape}")
    (rq, q_out, lddq, dq_head), (rk, k_out, lddk, dk_head), (rv, v_out, lddv, dv_head) = grads
    capi_attn_bwd.check(capi_attn_bwd.lib().mispmm_attn_bsr_bwd_bf16(
        _stream_ptr(stream), heads, a.num_rows // bs, a.num_cols, bs, a.num_blocks, _p(a.block_row_ptrs), _p(a.block_col_idxs),
        _p(at.block_row_ptrs), _p(at.block_col_idxs), _p(perm), _p(q3), ldq, q_head, _p(k3), ldk, k_head, _p(v3), ldv, v_head,
        _p(g3), ldg, g_head, _p(o3), ldo, o_head, int(out_bf16), _p(lse), _p(delta), d, dvw, _p(mask), float(scale),
        _p(q_out), lddq, dq_head, _p(k_out), lddk, dk_head, _p(v_out), lddv, dv_head, int(bool(grads_bf16))))
    return rq, rk, rv


def bsr_transpose(bsr):
    """(formats.BSR of A^T, perm) on the host: mispmm_csr_transpose_host on the block arrays, a stable counting sort of A's
    blocks by block column.  Block t of A^T is block perm[t] of A with its two inner axes swapped; a block row of A^T lists its
    blocks by ascending block row of A.  perm is uint32."""
    br, bc = bsr.block_row_size, bsr.block_col_size
    blocks = np.asarray(bsr.data).reshape(bsr.num_blocks, br, bc)
    t, perm = csr_transpose(formats.CSR(bsr.num_rows // br, bsr.num_cols // bc, bsr.block_row_ptrs, bsr.block_col_idxs, blocks))
    return formats.BSR(bsr.num_cols, bsr.num_rows, bsr.nnz, bc, br, t.row_ptrs, t.col_idxs,
                       np.ascontiguousarray(t.data.transpose(0, 2, 1))), perm


@dataclass
class DeviceBSRC:
    """Column-compacted block rows of a 16-row BSR (mispmm_bsr_compact_bf16_host)."""
    num_rows: int
    num_cols: int
    num_steps: int
    step_ptrs: torch.Tensor
    cols: torch.Tensor
    tiles: torch.Tensor      # int16 view of bf16 bits, [num_steps, 16, 32]

    @staticmethod
    def from_host(bsr, device="cuda", check=True):
        if check:
            check_host(bsr)
        l = capi.lib()
        ptrs = np.ascontiguousarray(bsr.block_row_ptrs, dtype=np.uint32)
        cols = np.ascontiguousarray(bsr.block_col_idxs, dtype=np.uint32)
        data = np.ascontiguousarray(bsr.data, dtype=np.float32).reshape(-1)
        n = ctypes.c_uint32(0)
        head = (bsr.num_block_rows, bsr.block_row_size, bsr.block_col_size, bsr.num_blocks, ptrs.ctypes.data, cols.ctypes.data,
                data.ctypes.data, ctypes.byref(n))
        capi.check(l.mispmm_bsr_compact_bf16_host(*head, None, None, None))
        sp = np.empty(bsr.num_block_rows + 1, dtype=np.uint32)
        cl = np.empty(max(1, n.value) * 32, dtype=np.uint32)
        tl = np.empty(max(1, n.value) * 512, dtype=np.uint16)
        capi.check(l.mispmm_bsr_compact_bf16_host(*head, sp.ctypes.data, cl.ctypes.data, tl.ctypes.data))
        return DeviceBSRC(bsr.num_rows, bsr.num_cols, n.value, _dev_u32(sp, device), _dev_u32(cl, device),
                          torch.from_numpy(tl.view(np.int16).copy()).to(device))


def spmm_bsrc_bf16(a, b_bf16, out_bf16=False, out=None, stream=None):
    """a: DeviceBSRC [M x K]; b_bf16: [K, N] int16 tensor of bf16 bits, unit column stride, any row stride of at least N.
    Returns [M, N] float32, or int16 bf16 bits with out_bf16; out= takes the result where given: that shape and dtype, unit
    column stride, any row stride of at least N."""
    _require_gpu(a.step_ptrs, b_bf16, out)
    n, ldb, out, ldc = _bf16_b_and_out(b_bf16, out_bf16, out, a.num_rows, a.num_cols)
    capi.check(capi.lib().mispmm_bsrc_bf16(_stream_ptr(stream), a.num_rows // 16, a.num_cols, a.num_steps, _p(a.step_ptrs),
                                           _p(a.cols), _p(a.tiles), _p(b_bf16), n, ldb, _p(out), ldc,
                                           int(bool(out_bf16))))
    return out


@dataclass
class DeviceBSRCSlots:
    """Column-compacted block rows of a 16-row BSR in fixed step slots, one workgroup per block row
    (mispmm_bsr_compact_slots_bf16_host)."""
    num_rows: int
    num_cols: int
    num_steps: int           # extent of cols / tiles: 4 slots per block row + extra steps
    used_steps: int          # steps that hold values (MFMA K steps executed)
    extra_ptrs: torch.Tensor
    cols: torch.Tensor
    tiles: torch.Tensor      # int16 view of bf16 bits, [num_steps, 16, 32]

    @staticmethod
    def from_host(bsr, device="cuda", check=True):
        if check:
            check_host(bsr)
        l = capi.lib()
        ptrs = np.ascontiguousarray(bsr.block_row_ptrs, dtype=np.uint32)
        cols = np.ascontiguousarray(bsr.block_col_idxs, dtype=np.uint32)
        data = np.ascontiguousarray(bsr.data, dtype=np.float32).reshape(-1)
        n, used = ctypes.c_uint32(0), ctypes.c_uint32(0)
        head = (bsr.num_block_rows, bsr.block_row_size, bsr.block_col_size, bsr.num_blocks, ptrs.ctypes.data, cols.ctypes.data,
                data.ctypes.data, ctypes.byref(n), ctypes.byref(used))
        capi.check(l.mispmm_bsr_compact_slots_bf16_host(*head, None, None, None))
        ep = np.empty(bsr.num_block_rows + 1, dtype=np.uint32)
        cl = np.empty(max(1, n.value) * 32, dtype=np.uint32)
        tl = np.empty(max(1, n.value) * 512, dtype=np.uint16)
        capi.check(l.mispmm_bsr_compact_slots_bf16_host(*head, ep.ctypes.data, cl.ctypes.data, tl.ctypes.data))
        return DeviceBSRCSlots(bsr.num_rows, bsr.num_cols, n.value, used.value, _dev_u32(ep, device), _dev_u32(cl, device),
                               torch.from_numpy(tl.view(np.int16).copy()).to(device))

    def operand_bytes(self):
        """Bytes of A one product must read: every slot's column list, the tiles of the used steps, the extra pointers."""
        return self.num_steps * 128 + self.used_steps * 1024 + (self.num_rows // 16 + 1) * 4


def spmm_bsrc_slots_bf16(a, b_bf16, out_bf16=False, out=None, stream=None):
    """a: DeviceBSRCSlots [M x K]; b_bf16, out_bf16 and out as spmm_bsrc_bf16 takes them."""
    _require_gpu(a.extra_ptrs, b_bf16, out)
    n, ldb, out, ldc = _bf16_b_and_out(b_bf16, out_bf16, out, a.num_rows, a.num_cols)
    capi.check(capi.lib().mispmm_bsrc_slots_bf16(_stream_ptr(stream), a.num_rows // 16, a.num_cols, a.num_steps, _p(a.extra_ptrs),
                                                 _p(a.cols), _p(a.tiles), _p(b_bf16), n, ldb, _p(out), ldc,
                                                 int(bool(out_bf16))))
    return out


def dense_transpose(x, stream=None):
    """x^T of a 2-D float32 device tensor (mispmm_dense_transpose_f32); a view that is not contiguous is copied first."""
    _require_gpu(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"x must be a 2-D float32 tensor, not {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    out = torch.empty((x.shape[1], x.shape[0]), dtype=torch.float32, device=x.device)
    capi.check(capi.lib().mispmm_dense_transpose_f32(_stream_ptr(stream), x.shape[0], x.shape[1], _p(x), _p(out)))
    return out


def colmajor_ell_to_rowmajor(ell):
    """Host conversion through the library's own helper (the path the C++ host uses)."""
    ridx = np.ascontiguousarray(ell.row_idxs, dtype=np.uint32)
    vals = np.ascontiguousarray(ell.data, dtype=np.float32)
    width = ctypes.c_uint32(0)
    l = capi.lib()
    capi.check(l.mispmm_ell_colmajor_to_rowmajor_host(ell.num_rows, ell.num_cols, ell.max_col_nnz, ridx.ctypes.data,
                                                      vals.ctypes.data, ctypes.byref(width), None, None))
    w = width.value
    cols = np.empty((ell.num_rows, w), dtype=np.uint32)
    out = np.empty((ell.num_rows, w), dtype=np.float32)
    capi.check(l.mispmm_ell_colmajor_to_rowmajor_host(ell.num_rows, ell.num_cols, ell.max_col_nnz, ridx.ctypes.data,
                                                      vals.ctypes.data, ctypes.byref(width), cols.ctypes.data,
                                                      out.ctypes.data))
    return formats.ELLRowMajor(ell.num_rows, ell.num_cols, ell.nnz, w, cols, out)


def ell_rows_f64(ell):
    """(rowPtrs, colIdxs, vals float64) of a column-major ELL's occupied slots, every row in spmmELLCpu's order of addition
    (mispmm_ell_colmajor_to_rows_f64_host).  A row-major ELL keeps its slot order, padding dropped."""
    if isinstance(ell, formats.ELLRowMajor):
        cols = np.ascontiguousarray(ell.col_idxs, dtype=np.uint32).reshape(ell.num_rows, -1)
        vals = np.ascontiguousarray(ell.data, dtype=np.float64).reshape(ell.num_rows, -1)
        live = cols != formats.ELL_PAD
        rp = np.concatenate([[0], np.cumsum(live.sum(axis=1))]).astype(np.uint32)
        return rp, cols[live], vals[live]
    ridx = np.ascontiguousarray(ell.row_idxs, dtype=np.uint32)
    vals = np.ascontiguousarray(ell.data, dtype=np.float64)
    nnz = ctypes.c_uint32(0)
    head = (ell.num_rows, ell.num_cols, ell.max_col_nnz, ridx.ctypes.data, vals.ctypes.data, ctypes.byref(nnz))
    l = capi.lib()
    capi.check(l.mispmm_ell_colmajor_to_rows_f64_host(*head, None, None, None))
    rp = np.zeros(ell.num_rows + 1, np.uint32)
    ci, va = np.zeros(max(nnz.value, 1), np.uint32), np.zeros(max(nnz.value, 1), np.float64)
    capi.check(l.mispmm_ell_colmajor_to_rows_f64_host(*head, rp.ctypes.data, ci.ctypes.data, va.ctypes.data))
    return rp, ci[:nnz.value], va[:nnz.value]


def bsr_nonzeros_f64_host(bsr):
    """(rowPtrs, colIdxs, vals float64) of a BSR's non-zero block entries in spmmBSRCpu's order (mispmm_bsr_nonzeros_f64_host)."""
    ptrs = np.ascontiguousarray(bsr.block_row_ptrs, dtype=np.uint32)
    cols = np.ascontiguousarray(bsr.block_col_idxs, dtype=np.uint32)
    data = np.ascontiguousarray(bsr.data, dtype=np.float64).reshape(-1)
    nnz = ctypes.c_uint32(0)
    args = (bsr.num_block_rows, bsr.block_row_size, bsr.block_col_size, bsr.num_blocks, ptrs.ctypes.data, cols.ctypes.data,
            data.ctypes.data, ctypes.byref(nnz))
    l = capi.lib()
    capi.check(l.mispmm_bsr_nonzeros_f64_host(*args, None, None, None))
    rp = np.empty(bsr.num_rows + 1, dtype=np.uint32)
    ci, va = np.empty(max(1, nnz.value), dtype=np.uint32), np.empty(max(1, nnz.value), dtype=np.float64)
    capi.check(l.mispmm_bsr_nonzeros_f64_host(*args, rp.ctypes.data, ci.ctypes.data, va.ctypes.data))
    return rp, ci[:nnz.value], va[:nnz.value]


def shard_rows_by_nnz(row_ptrs, parts):
    rp = np.ascontiguousarray(row_ptrs, dtype=np.uint32)
    bounds = np.zeros(parts + 1, dtype=np.uint32)
    capi.check(capi.lib().mispmm_shard_rows_by_nnz_host(rp.shape[0] - 1, rp.ctypes.data, parts, bounds.ctypes.data))
    return bounds


# ---- the row-list product with B in bf16 (libmispmm_bf16.so, include/mispmm_bf16.h)
def _spmm_rows_bf16(what, num_rows, num_cols, nnz, row_ptrs, row_nnz, col_idxs, data, b_bf16, out_bf16, out, acc, sum_f32, stream):
    """C = A @ B from A's row list through mispmm_rows_bf16: A's values fp32, B int16 bf16 bits, C float32 or int16 bf16
    bits.  row_ptrs=None: every row holds row_nnz entries (0xFFFFFFFF = padding).  Exact contracts, see the header."""
    from . import capi_bf16
    _require_gpu(col_idxs, data, b_bf16, out)
    if data.dtype != torch.float32:
        raise ValueError(f"{what} takes a float32 matrix, not {data.dtype}")
    mode = _acc_mode(acc)
    n, ldb, out, ldc = _bf16_b_and_out(b_bf16, out_bf16, out, num_rows, num_cols)
    capi_bf16.check(capi_bf16.lib().mispmm_rows_bf16(_stream_ptr(stream), num_rows, num_cols, nnz, _p(row_ptrs), int(row_nnz), _p(col_idxs),
                                                     _p(data), _p(b_bf16), n, ldb, _p(out), ldc, int(bool(out_bf16)), mode,
                                                     int(bool(sum_f32))))
    return out


def spmm_csr_bf16(a, b_bf16, out_bf16=False, out=None, acc="reference", ref_sum="f64", stream=None):
    """C = A @ B with B in bf16 (mispmm_rows_bf16).  a: any float32 DeviceCSR -- a CSR, or the list of bsr_nonzeros (pass
    ref_sum="f32" for that one: the fp32 sum of the BSR reference); b_bf16: [K, N] int16 tensor of bf16 bits, unit column
    stride, any row stride; returns [M, N] float32, or int16 bf16 bits with out_bf16.  acc="reference": the fp32 product
    summed in a double (ref_sum="f64", the CSR rule) or in fp32 (ref_sum="f32"); acc="fast": one fma per entry.  Plan and
    span list are not used; a matrix of uniform rows is walked without its row pointers (MISPMM_NO_HINT=1: with them)."""
    if ref_sum not in ("f64", "f32"):
        raise ValueError(f"ref_sum must be 'f64' or 'f32', not {ref_sum!r}")
    _require_gpu(a.row_ptrs)
    uniform = a.uniform_row_nnz and os.environ.get("MISPMM_NO_HINT") != "1"
    return _spmm_rows_bf16("spmm_csr_bf16", a.num_rows, a.num_cols, a.nnz, None if uniform else a.row_ptrs, a.uniform_row_nnz if uniform else 0,
                           a.col_idxs, a.data, b_bf16, out_bf16, out, acc, ref_sum == "f32", stream)


def spmm_coo_bf16(a, b_bf16, out_bf16=False, out=None, acc="reference", stream=None):
    """C = A @ B with B in bf16 for a float32 DeviceCOO (entries stable-sorted by row at upload): fp32 product, fp32 sum in
    list order (the COO reference's rule), or acc="fast".  The row boundaries are built by coo_row_bounds on first use and
    kept in a.row_bounds.  Operands as spmm_csr_bf16."""
    _require_gpu(a.row_idxs)
    if a.data.dtype != torch.float32:
        raise ValueError(f"spmm_coo_bf16 takes a float32 matrix, not {a.data.dtype}")
    if a.row_bounds is None:
        _require_gpu(b_bf16, out)            # the first product launches twice: refuse a bad operand before the first launch
        _acc_mode(acc)
        out = _bf16_b_and_out(b_bf16, out_bf16, out, a.num_rows, a.num_cols)[2]
        a.row_bounds = coo_row_bounds(a, stream)
    return _spmm_rows_bf16("spmm_coo_bf16", a.num_rows, a.num_cols, a.nnz, a.row_bounds, 0, a.col_idxs, a.data, b_bf16, out_bf16, out, acc, True,
                           stream)


def spmm_ell_bf16(a, b_bf16, out_bf16=False, out=None, acc="reference", stream=None):
    """C = A @ B with B in bf16 for a float32 DeviceELL: the list of occupied slots where the upload made one (`compact`),
    else the padded row-major arrays as a uniform list of `width` entries per row, the padding skipped by its column index.
    fp32 product, fp32 sum in slot order (the ELL reference's rule), or acc="fast".  Operands as spmm_csr_bf16."""
    _require_gpu(a.col_idxs)
    if a.data.dtype != torch.float32:
        raise ValueError(f"spmm_ell_bf16 takes a float32 matrix, not {a.data.dtype}")
    if a.compact is not None:
        nnz, rp, ci, va = a.compact[:4]
        return _spmm_rows_bf16("spmm_ell_bf16", a.num_rows, a.num_cols, nnz, rp, 0, ci, va, b_bf16, out_bf16, out, acc, True, stream)
    return _spmm_rows_bf16("spmm_ell_bf16", a.num_rows, a.num_cols, a.num_rows * a.width, None, a.width, a.col_idxs, a.data, b_bf16, out_bf16, out,
                           acc, True, stream)
