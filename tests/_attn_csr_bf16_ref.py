"""The fused bf16 CSR attention contract (include/mispmm_attn_csr_bf16.h) for the tests: the cases and operands the CPU and GPU
tests share, the checks, the bf16-specific faults, and the table of kernel tags.

bf16 widens to fp32 exactly, so the contract IS the ALGORITHM of include/mispmm_attn_csr.h on the widened operands and every
reference is one the project already owns, evaluated on them: the float64 attention with both tolerances (_attn_csr_ref), the
derived tight check (_attn_csr_tight), the restatement `_attn_csr_ref.fused_f32`.  Nothing here is measured on a kernel.

OPERANDS, built the way _attn_csr_ref.operands builds them: q and k from its `_grid` (n / 256 with 64 <= |n| <= 192: eight
significant bits, so they ARE bf16 values and every score is exact in fp32 in any order, asserted per case), the power-of-two
scale, `make_bias`; v has full mantissas ROUNDED TO bf16 (synth.bf16_round), and every reference reads the rounded v.
LAYOUT on the device (`padded_bits`): every operand is the [:, :width] corner of a buffer 8 columns wider whose pad columns hold
NaN bits, so a multiple of 8 stays one and a kernel that strays by a column meets a NaN.
A bf16 out is the fp32 out rounded once to nearest even (`_spmm_bf16_ref.bf16_bits`: the project's rounding reference for
mispmm_rows_bf16's bf16 C)."""
import functools

import numpy as np

import _attn_csr_ref as ref
import _attn_csr_tight as tight
from _softmax_ref import full_mantissa, matrix
from _spmm_bf16_ref import bf16_bits, same_bits, widen  # noqa: F401  (re-exported for the tests)

from mispmm import synth

PATTERNS = ("edges", "ragged")
#          V8 ....................................................  V1 ..........................................
WIDTHS = ((8, 64), (64, 8), (40, 72), (128, 128), (256, 256), (3, 5), (1, 1), (100, 36), (1, 129))
BIASES = ("none", "finite", "masked")
HEADS = (1, 3)
PAD = 8                      # pad columns of every device buffer
NAN_BITS = 0x7FC1            # what the pad columns of the inputs hold
OUT_SENTINEL_BF16 = 0x7FDE   # what the pad columns of a bf16 out hold before the call, and after

Case = ref.Case
CASES = tuple(Case(n, d, dv, b, h) for n in PATTERNS for (d, dv) in WIDTHS for b in BIASES for h in HEADS)

# deliberate bf16-specific faults of the restatement: name -> the words of mispmm_attn_csr_bf16.h it breaks
FAULTS = {
    "k_pair_swapped": "S: `columns ascending` of the widened k -- the halves of every 32-bit pair of a K row exchanged (columns 2j, 2j + 1).",
    "v_pair_swapped": "product: `O = fma(w_i, v[c_i], O)` per column -- the halves of every 32-bit pair of a V row exchanged.",
    "out_truncated": "OPERANDS: a bf16 out is `rounded once to nearest even` -- the low 16 bits are cut off instead.",
    "v_at_k_offset": "OPERANDS: `row strides ldq / ldk / ldv / ldo` -- V's rows are read at ldk's stride (ldk != ldv in the case).",
}


def is_bf16(x):
    """True where every element of the float32 array is a bf16 value: the low 16 bits are clear."""
    return not np.any(np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF))


def to_bits(x):
    """float32 holding bf16 values -> their int16 bit patterns (the upper halves)."""
    assert is_bf16(x)
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16).view(np.int16)


def padded_bits(x, pad=PAD):
    """[..., n, w] float32 of bf16 values -> int16 [..., n, w + pad]: the bits in the [:, :w] corner, NaN bits in the pad."""
    buf = np.full(x.shape[:-1] + (x.shape[-1] + pad,), NAN_BITS, np.uint16).view(np.int16)
    buf[..., :x.shape[-1]] = to_bits(x)
    return buf


@functools.lru_cache(maxsize=None)
def operands(case):
    """dict(q [H, M, D], k [1, K, D], v [1, K, Dv], bias None | [nnz] | [H, nnz], scale), float32 arrays of bf16 values: k and v
    are shared by the heads (head stride 0), `finite` with H > 1 has a bias per head and `masked` a shared one.  Read-only."""
    csr = matrix(case.name)
    rng = np.random.default_rng(19000 + 7 * case.d + case.dv + 100 * case.heads + len(case.bias))
    q = ref._grid(rng, (case.heads, csr.num_rows, case.d))
    k = ref._grid(rng, (1, csr.num_cols, case.d))
    v = synth.bf16_round(full_mantissa(rng, (1, csr.num_cols, case.dv), np.float32).reshape(-1)).reshape(1, csr.num_cols, case.dv).astype(np.float32)
    per_head = case.heads if case.bias == "finite" else 1
    bias = ref.make_bias(csr, case.bias, per_head, rng)
    if bias is not None and per_head == 1:
        bias = bias[0]
    res = dict(q=q, k=k, v=v, bias=bias, scale=ref.scale_of(case.d))
    for x in res.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return res


# ---- the checks, functions of (got, case) as those of _attn_csr_mutants, on THESE operands
@functools.lru_cache(maxsize=None)
def expected(case):
    """(out, lse, out tolerance, lse tolerance) of a case in float64; read-only."""
    op, csr = operands(case), matrix(case.name)
    out, lse = ref.attention_f64(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"])
    return (out, lse, ref.out_tolerance(csr, op["q"], op["k"], op["v"], op["scale"], op["bias"]),
            ref.lse_tolerance(csr, op["q"], op["k"], op["scale"], op["bias"]))


@functools.lru_cache(maxsize=None)
def tight_reference(case):
    op = operands(case)
    return tight.forward_reference(matrix(case.name), op["q"], op["k"], op["v"], op["scale"], op["bias"])


def out_composed(got, case):
    """out against float64 inside the composed tolerance of the four-launch chain: (ok, worst |err| / tolerance)."""
    want, _, tol, _ = expected(case)
    with np.errstate(invalid="ignore"):
        err = np.abs(got["out"].astype(np.float64) - want)
        return bool(np.all(err <= tol)), float(np.max(np.where(np.isnan(err), np.inf, err / tol)))


def lse_bound(got, case):
    """lse against float64 inside the header's bound; -Inf exactly on the rows without entries."""
    _, want, _, tol = expected(case)
    stored = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got["lse"][stored].astype(np.float64) - want[stored])
        ok = bool(np.all(err <= tol[stored])) and bool(np.array_equal(np.isneginf(got["lse"]), ~stored))
        return ok, float(np.max(np.where(np.isnan(err), np.inf, err / tol[stored]), initial=0.0))


def tight_forward(got, case):
    """out and lse against the derived reference of _attn_csr_tight, every element: (ok, worst ratio)."""
    out, tol, lse, ltol = tight_reference(case)
    ok_out, worst_out = tight._worst(got["out"], out, tol)
    stored = np.isfinite(lse)
    ok_lse, worst_lse = tight._worst(got["lse"][stored], lse[stored], ltol[stored])
    return ok_out and ok_lse and bool(np.array_equal(np.isneginf(got["lse"]), ~stored)), max(worst_out, worst_lse)


def rounded_once(got, case=None):
    """The bf16 out is the fp32 out rounded once to nearest even, bit for bit, NaN for NaN: (ok, elements that differ)."""
    want = bf16_bits(got["out"])
    bits = np.ascontiguousarray(got["out_bf16"]).view(np.uint16)
    nan = np.isnan(widen(want))
    wrong = int((nan != np.isnan(widen(bits))).sum() + (bits[~nan] != want[~nan]).sum())
    return wrong == 0, float(wrong)


CHECKS = {"out_composed": out_composed, "lse_bound": lse_bound, "tight_forward": tight_forward, "rounded_once": rounded_once}


# ---- the restatement and its bf16-specific faults
def _swap_pairs(x):
    """Columns 2j and 2j + 1 exchanged, as far as whole pairs go."""
    y = x.copy()
    n = x.shape[-1] // 2 * 2
    y[..., 0:n:2], y[..., 1:n:2] = x[..., 1:n:2], x[..., 0:n:2]
    return y


def _rows_at_stride(x, ld_own, ld_used):
    """Rows of x [1, K, W], stored with row stride ld_own (zeros between rows), read at row stride ld_used; a read past the
    buffer's end returns zeros, as a buffer load does."""
    rows, width = x.shape[1], x.shape[2]
    flat = np.zeros(rows * max(ld_own, ld_used) + width, np.float32)
    at = (np.arange(rows)[:, None] * ld_own + np.arange(width)[None, :]).ravel()
    flat[at] = x[0].ravel()
    end = (rows - 1) * ld_own + width                       # the span of the descriptor
    want = np.arange(rows)[:, None] * ld_used + np.arange(width)[None, :]
    return np.where(want < end, flat[np.minimum(want, flat.shape[0] - 1)], np.float32(0))[None].astype(np.float32)


@functools.lru_cache(maxsize=8)
def restated(case, fault=None):
    """dict(out, lse, out_bf16): _attn_csr_ref.fused_f32 on the case's operands, the bf16 out its rounding; fault: None or one
    of FAULTS."""
    if fault is not None and fault not in FAULTS:
        raise ValueError(f"unknown fault {fault!r}")
    op, csr = operands(case), matrix(case.name)
    k, v = op["k"], op["v"]
    if fault == "k_pair_swapped":
        k = _swap_pairs(k)
    if fault == "v_pair_swapped":
        v = _swap_pairs(v)
    if fault == "v_at_k_offset":
        v = _rows_at_stride(v, case.dv + PAD, case.d + PAD)
    out, lse = ref.fused_f32(csr, op["q"], k, v, op["scale"], op["bias"])
    if fault == "out_truncated":
        out_bf16 = (np.ascontiguousarray(out).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    else:
        out_bf16 = bf16_bits(out)
    return dict(out=out, lse=lse, out_bf16=out_bf16)


# ---- the kernel tags
def tag_of(d, dv, aligned):
    """mispmm_last_kernel() for (D, Dv, operands 16-byte aligned with strides in multiples of 8): the host's choice restated."""
    vec = 8 if aligned and d % 8 == 0 and dv % 8 == 0 else 1
    need = -(-max(d, dv) // vec)
    g = next((x for x in (8, 16, 32, 64) if x >= need), 64)
    chunks = 1 if g < 64 else -(-max(d, dv) // (64 * vec))
    return f"attn_csr_bf16<G{g},V{vec},C{1 if chunks <= 1 else 2 if chunks == 2 else 4}>"


# tag -> the smallest (D, Dv, aligned) that reaches it
TAGS = {
    "attn_csr_bf16<G8,V8,C1>": (8, 8, True), "attn_csr_bf16<G16,V8,C1>": (8, 72, True), "attn_csr_bf16<G32,V8,C1>": (8, 136, True),
    "attn_csr_bf16<G8,V1,C1>": (1, 1, False), "attn_csr_bf16<G16,V1,C1>": (1, 9, False), "attn_csr_bf16<G32,V1,C1>": (1, 17, False),
    "attn_csr_bf16<G64,V1,C1>": (1, 33, False), "attn_csr_bf16<G64,V1,C2>": (1, 65, False), "attn_csr_bf16<G64,V1,C4>": (1, 129, False),
}


def with_one_bf16_rounding(reference, tol):
    """A tolerance on an fp32 result, widened by the one rounding that makes it bf16: tol + 2^-8 (|reference| + tol).  2^-8 is
    the rounding unit of bf16 (to nearest: half of it on a normal result); the value rounded lies within tol of the reference."""
    return tol + 2.0 ** -8 * (np.abs(reference) + tol)
