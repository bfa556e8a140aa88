"""Fused bf16 attention on a CSR pattern (mispmm_attn_csr_bf16 through attn_csr_bf16.attention_csr_bf16 and
autograd.sparse_attention_bf16) on the GPU.  bf16 widens to fp32 exactly, so every reference is one the project owns, on the
widened operands: float64 inside the composed tolerance and the header's lse bound, the derived tight check on every element,
the fp32 kernel BIT FOR BIT where the scores are exact, the fp32 out rounded once for a bf16 out, the exact tie rows, special
values, strides and alignment, every kernel tag, determinism and graph replay, and autograd against the composition that
defines its backward.  The checks are the functions tests/test_attn_csr_bf16_cpu.py runs the faulty restatements through."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, capi_attn_csr, capi_attn_csr_bf16, capi_attn_csr_bwd, formats, ops, synth  # noqa: E402
from mispmm.attn_csr_bf16 import attention_csr_bf16  # noqa: E402

import _attn_csr_bf16_ref as bref  # noqa: E402
import _attn_csr_bwd_ref as bwd  # noqa: E402
import _attn_csr_ref as ref  # noqa: E402
import _attn_csr_tight as tight  # noqa: E402
from _bits import SENTINEL_BITS, assert_same_bits  # noqa: E402
from _softmax_ref import full_mantissa, matrix  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = bref.PAD


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the shared operands are read-only


def bf16_values(rng, shape):
    """Full-mantissa values rounded to bf16, as float32."""
    return synth.bf16_round(full_mantissa(rng, shape, np.float32).reshape(-1)).reshape(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def device_csr(name):
    return ops.DeviceCSR.from_host(matrix(name), plan=False)


def layout(op):
    """(q, k, v, bias) on the device as the suite lays them out: int16 bf16 bits, every operand the [:, :width] corner of a
    buffer PAD columns wider whose pad holds NaN bits; q a view of [M, H, D + PAD] storage; k and v given as one head are
    expanded over all (head stride 0); one head: plain 2-D tensors."""
    heads, d, dv = op["q"].shape[0], op["q"].shape[2], op["v"].shape[2]
    bias = None if op["bias"] is None else dev(op["bias"])
    if heads == 1:
        return dev(bref.padded_bits(op["q"][0]))[:, :d], dev(bref.padded_bits(op["k"][0]))[:, :d], dev(bref.padded_bits(op["v"][0]))[:, :dv], bias
    q = dev(np.ascontiguousarray(bref.padded_bits(op["q"]).transpose(1, 0, 2))).permute(1, 0, 2)[:, :, :d]
    assert q.stride() == (d + PAD, heads * (d + PAD), 1)
    kv = []
    for x, w in ((op["k"], d), (op["v"], dv)):
        if x.shape[0] == 1:
            kv.append(dev(bref.padded_bits(x[0]))[:, :w].unsqueeze(0).expand(heads, -1, -1))
            assert kv[-1].stride(0) == 0
        else:
            kv.append(dev(bref.padded_bits(x))[:, :, :w])
    return q, kv[0], kv[1], bias


def run(a, op, out_bf16=False, lay=None):
    """dict(out [H, M, Dv] float32 or uint16 bits, lse [H, M], tag).  out is the corner of a buffer PAD columns wider whose
    pad holds a sentinel that must survive."""
    q, k, v, bias = lay if lay is not None else layout(op)
    heads, dv = op["q"].shape[0], op["v"].shape[2]
    m = a.num_rows
    if out_bf16:
        store = torch.full((heads, m, dv + PAD), bref.OUT_SENTINEL_BF16, dtype=torch.int16, device="cuda")
    else:
        store = torch.empty((heads, m, dv + PAD), dtype=torch.float32, device="cuda")
        store.view(torch.int32).fill_(SENTINEL_BITS)
    lse = torch.full((heads, m) if heads > 1 else (m,), -5.0, device="cuda")
    got = attention_csr_bf16(a, q, k, v, scale=op["scale"], bias=bias, out_bf16=out_bf16, out=store[:, :, :dv] if heads > 1 else store[0, :, :dv], lse=lse)
    assert got.data_ptr() == store.data_ptr()
    tag = capi_attn_csr_bf16.last_kernel()
    host = store.cpu().numpy()
    raw = host.view(np.uint16 if out_bf16 else np.uint32)
    assert np.all(raw[:, :, dv:] == (bref.OUT_SENTINEL_BF16 if out_bf16 else SENTINEL_BITS)), "the pad columns of out must keep their sentinel"
    out = np.ascontiguousarray(raw[:, :, :dv] if out_bf16 else host[:, :, :dv])
    return dict(out=out, lse=lse.cpu().numpy().reshape(heads, m), tag=tag)


def run_f32(a, op):
    """ops.attention_csr on the widened operands (the float32 arrays of the case ARE the widened values)."""
    heads = op["q"].shape[0]
    bias = None if op["bias"] is None else dev(op["bias"])
    if heads == 1:
        q, k, v = dev(op["q"][0]), dev(op["k"][0]), dev(op["v"][0])
    else:
        q = dev(op["q"])
        k, v = (dev(op[n][0]).unsqueeze(0).expand(heads, -1, -1) if op[n].shape[0] == 1 else dev(op[n]) for n in ("k", "v"))
    out, lse = ops.attention_csr(a, q, k, v, scale=op["scale"], bias=bias, return_lse=True)
    return dict(out=out.cpu().numpy().reshape(heads, a.num_rows, -1), lse=lse.cpu().numpy().reshape(heads, a.num_rows))


@functools.lru_cache(maxsize=None)
def results(case):
    """The three runs of a case, made once: the new kernel with fp32 out and lse, with bf16 out, and the fp32 kernel."""
    op, a = bref.operands(case), device_csr(case.name)
    lay = layout(op)
    return run(a, op, lay=lay), run(a, op, out_bf16=True, lay=lay), run_f32(a, op)


CASE_PARAMS = [pytest.param(c, id=c.id) for c in bref.CASES]


def test_the_device_widening_is_the_hosts():
    case = bref.Case("ragged", 40, 72, "none", 3)
    op = bref.operands(case)
    for n in ("q", "k", "v"):
        assert_same_bits(ops.bf16_to_f32(dev(bref.to_bits(op[n]))).cpu().numpy(), op[n], n)


@pytest.mark.parametrize("case", CASE_PARAMS)
def test_fp32_out_and_lse_against_float64_the_tight_check_and_the_fp32_kernel_bit_for_bit(case):
    got, _, f32 = results(case)
    assert got["tag"] == bref.tag_of(case.d, case.dv, True), got["tag"]
    checks = {what: bref.CHECKS[what](got, case) for what in ("out_composed", "lse_bound", "tight_forward")}
    print(f"attn_csr_bf16 {case.id} {got['tag']}: worst |err| / tolerance: " + ", ".join(f"{what} {worst:.3g}" for what, (_, worst) in checks.items()))
    for what, (ok, worst) in checks.items():
        assert ok, f"{case.id}: {what} fails, worst {worst:.3g} x"
    assert_same_bits(got["out"], f32["out"], f"{case.id}: out against ops.attention_csr on the widened operands")
    assert_same_bits(got["lse"], f32["lse"], f"{case.id}: lse against ops.attention_csr on the widened operands")
    empty = np.diff(matrix(case.name).row_ptrs.astype(np.int64)) == 0
    assert not got["out"][:, empty].view(np.uint32).any(), "an empty row must be +0"
    assert np.all(np.isneginf(got["lse"][:, empty]))


@pytest.mark.parametrize("case", CASE_PARAMS)
def test_bf16_out_is_the_fp32_out_rounded_once(case):
    got, got16, _ = results(case)
    assert got16["tag"] == got["tag"]
    ok, wrong = bref.rounded_once(dict(out=got["out"], out_bf16=got16["out"]))
    assert ok, f"{case.id}: {int(wrong)} elements of the bf16 out are not the fp32 out rounded to nearest even"
    assert_same_bits(got16["lse"], got["lse"], "lse does not depend on the out type")
    empty = np.diff(matrix(case.name).row_ptrs.astype(np.int64)) == 0
    assert not got16["out"][:, empty].any(), "an empty row must be +0"
    assert np.all(np.isneginf(got16["lse"][:, empty]))


@pytest.mark.parametrize("through_bias", [False, True])
@pytest.mark.parametrize("t", tight.TIES)
def test_tie_rows_bit_for_bit(t, through_bias):
    seen = tight.tie_coverage(t)
    assert seen["slots"] == set(range(8)) and seen["first_batch"] and seen["last_batch"] and seen["partial_last"], seen
    csr = tight.tie_pattern(t)[0]
    op = tight.tie_operands(t, through_bias)
    assert all(bref.is_bf16(op[n]) for n in ("q", "k", "v"))
    a = ops.DeviceCSR.from_host(csr, plan=False)
    lay = layout(op)
    got = run(a, op, lay=lay)
    ok, wrong = tight.tie_check(got, t, through_bias)
    assert ok, f"t={t} through_bias={through_bias}: {wrong} elements differ from the exact answers"
    want = tight.tie_expected(t, through_bias)[0].astype(np.float32)
    assert bref.is_bf16(want)
    got16 = run(a, op, out_bf16=True, lay=lay)
    assert np.array_equal(got16["out"], bref.to_bits(want).view(np.uint16)), "the bf16 out must be the expected integers, bit for bit"


@pytest.mark.parametrize("d,dv", [(64, 64), (40, 72)])
def test_scores_that_round_lie_inside_the_composed_tolerances(d, dv):
    csr, heads = matrix("ragged"), 2
    rng = np.random.default_rng(171 + d)
    # eight significant bits in [0.5, 2) alone would still sum exactly in fp32 (products of 16 bits, 64 of them below 2^8): the
    # elements also get exponents of their own, 2^-6 .. 2^0, so a row's products span 12 binades more and the sums round
    spread = lambda shape: bf16_values(rng, shape) * np.exp2(rng.integers(-6, 1, shape)).astype(np.float32)      # noqa: E731
    op = dict(q=spread((heads, csr.num_rows, d)), k=spread((heads, csr.num_cols, d)), v=bf16_values(rng, (heads, csr.num_cols, dv)),
              bias=None, scale=d ** -0.5)
    assert bref.is_bf16(op["q"]) and bref.is_bf16(op["k"]) and not tight.exact_scores(csr, op["q"], op["k"], 0.125, None)
    rows, cols = ref.entry_rows(csr.row_ptrs), csr.col_idxs.astype(np.int64)
    s64 = (op["q"][0].astype(np.float64)[rows] * op["k"][0].astype(np.float64)[cols]).sum(axis=1)
    assert np.mean(s64.astype(np.float32).astype(np.float64) != s64) > 0.5, "most scores must not be fp32 numbers"
    got = run(device_csr("ragged"), op)
    assert got["tag"] == bref.tag_of(d, dv, True)
    want_out, want_lse = ref.attention_f64(csr, op["q"], op["k"], op["v"], op["scale"])
    err = np.abs(got["out"] - want_out) / ref.out_tolerance(csr, op["q"], op["k"], op["v"], op["scale"])
    stored = np.isfinite(want_lse)
    lerr = np.abs(got["lse"][stored] - want_lse[stored]) / ref.lse_tolerance(csr, op["q"], op["k"], op["scale"])[stored]
    print(f"attn_csr_bf16 rounding scores D={d} Dv={dv}: worst |err| / tolerance: out {float(err.max()):.3g}, lse {float(lerr.max()):.3g}")
    assert np.all(err <= 1.0) and np.all(lerr <= 1.0) and np.array_equal(np.isneginf(got["lse"]), ~stored)


def _shifted_edges():
    """`edges` with every column moved up by one on K + 2 columns: no entry names column 0 or the last one."""
    csr = matrix("edges")
    return formats.CSR(csr.num_rows, csr.num_cols + 2, csr.row_ptrs, (csr.col_idxs + 1).astype(np.uint32), csr.data)


def test_special_values_are_torchs_and_stay_in_their_rows():
    csr = matrix("edges")
    a = device_csr("edges")
    op = dict(bref.operands(bref.Case("edges", 8, 8, "finite", 1)))
    ptrs = csr.row_ptrs.astype(np.int64)
    lens = np.diff(ptrs)
    clean, clean16 = run(a, op), run(a, op, out_bf16=True)
    rows = {"nan": int(np.argwhere(lens == 33)[0, 0]), "+inf": int(np.argwhere(lens == 17)[0, 0]), "all -inf": int(np.argwhere(lens == 9)[0, 0]),
            "both": int(np.argwhere(lens == 300)[0, 0])}
    bias = op["bias"].copy()
    bias[ptrs[rows["nan"]] + 20] = np.nan
    bias[ptrs[rows["+inf"]] + 3] = np.inf
    bias[ptrs[rows["all -inf"]]:ptrs[rows["all -inf"] + 1]] = -np.inf
    bias[ptrs[rows["both"]] + 5], bias[ptrs[rows["both"]] + 250] = np.inf, np.nan
    op["bias"] = bias
    hit = np.zeros(csr.num_rows, bool)
    hit[list(rows.values())] = True
    want = torch.logsumexp(torch.tensor([[np.nan, 0.0], [np.inf, 0.0], [-np.inf, -np.inf], [np.inf, np.nan]]), dim=1).numpy()
    for out_bf16 in (False, True):
        got = run(a, op, out_bf16=out_bf16)
        out = bref.widen(got["out"]) if out_bf16 else got["out"]
        base = (clean16 if out_bf16 else clean)["out"]
        assert np.array_equal(np.isnan(out[0]), np.broadcast_to(hit[:, None], out[0].shape))
        assert np.array_equal(got["out"][0][~hit].view(np.uint16 if out_bf16 else np.uint32), base[0][~hit].view(np.uint16 if out_bf16 else np.uint32))
        assert_same_bits(got["lse"][0][~hit], clean["lse"][0][~hit], "lse of rows without a special value")
        for (what, r), w in zip(rows.items(), want):
            assert np.array_equal(got["lse"][0][r:r + 1], w[None], equal_nan=True), (what, got["lse"][0][r], w)
    # a NaN SCORE through the operands: NaN bits in a row of K that one entry of one row names
    named = int(csr.col_idxs[ptrs[rows["nan"]] + 20])
    k = op["k"].copy()
    k[0, named, 3] = np.nan
    got = run(a, dict(op, bias=None, k=k))
    poisoned = np.array([named in csr.col_idxs[lo:hi] for lo, hi in zip(ptrs[:-1], ptrs[1:])])
    assert poisoned[rows["nan"]] and not poisoned.all()
    assert np.array_equal(np.isnan(got["out"][0]), np.broadcast_to(poisoned[:, None], got["out"][0].shape)) and np.array_equal(np.isnan(got["lse"][0]), poisoned)
    # an empty row: +0 and -Inf; a row of one finite entry: that row of V (w = 1, l = 1)
    assert np.array_equal(np.isneginf(clean["lse"][0]), lens == 0)
    for r in np.argwhere(lens == 1).ravel():
        assert_same_bits(clean["out"][0][r], op["v"][0][csr.col_idxs[ptrs[r]]] + np.float32(0), f"row {r} of one entry")


@pytest.mark.parametrize("d,dv", [(8, 8), (3, 5), (40, 72), (1, 129)])
def test_nan_bits_in_rows_of_k_and_v_that_no_entry_names_reach_no_output(d, dv):
    csr = _shifted_edges()
    a = ops.DeviceCSR.from_host(csr, plan=False)
    rng = np.random.default_rng(178)
    op = dict(q=bf16_values(rng, (1, csr.num_rows, d)), k=bf16_values(rng, (1, csr.num_cols, d)), v=bf16_values(rng, (1, csr.num_cols, dv)),
              bias=None, scale=d ** -0.5)
    clean, clean16 = run(a, op), run(a, op, out_bf16=True)
    assert not np.isnan(clean["out"]).any() and clean["tag"] == bref.tag_of(d, dv, True)
    q, k, v, _ = layout(op)
    for x in (k, v):                                  # row 0 (where a wrapped offset would land) and a row nobody names
        x[0] = bref.NAN_BITS
        x[-1] = bref.NAN_BITS
    for out_bf16, base in ((False, clean), (True, clean16)):
        got = run(a, op, out_bf16=out_bf16, lay=(q, k, v, None))
        assert np.array_equal(got["out"].view(np.uint16 if out_bf16 else np.uint32), base["out"].view(np.uint16 if out_bf16 else np.uint32)), "out with NaN rows planted"
        assert_same_bits(got["lse"], base["lse"], "lse with NaN rows planted")


def test_an_empty_pattern_and_k_with_one_row():
    rng = np.random.default_rng(179)
    empty = formats.CSR(5, 7, np.zeros(6, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    op = dict(q=bf16_values(rng, (2, 5, 16)), k=bf16_values(rng, (2, 7, 16)), v=bf16_values(rng, (2, 7, 24)), bias=None, scale=0.25)
    for out_bf16 in (False, True):
        got = run(ops.DeviceCSR.from_host(empty, plan=False), op, out_bf16=out_bf16)
        assert not got["out"].view(np.uint16 if out_bf16 else np.uint32).any() and np.all(np.isneginf(got["lse"]))
    one = formats.CSR(4, 1, np.array([0, 1, 1, 3, 4], np.uint32), np.zeros(4, np.uint32), np.ones(4, np.float32))
    op = dict(q=bf16_values(rng, (1, 4, 8)), k=bf16_values(rng, (1, 1, 8)), v=bf16_values(rng, (1, 1, 8)), bias=None, scale=0.5)
    got = run(ops.DeviceCSR.from_host(one, plan=False), op)
    for r in (0, 2, 3):                               # every weight is 1 / L of the same row of V; two entries: (v + v) / 2
        assert_same_bits(got["out"][0][r], op["v"][0][0] + np.float32(0), f"row {r}")
    assert not got["out"][0][1].view(np.uint32).any() and np.isneginf(got["lse"][0][1])


def test_strides_and_alignment_give_the_same_bits():
    case = bref.Case("edges", 40, 72, "finite", 3)
    op, a = bref.operands(case), device_csr("edges")
    base, base16, _ = results(case)
    heads, m, kk, d, dv = 3, a.num_rows, a.num_cols, 40, 72
    q, k, v, bias = layout(op)
    assert k.stride(0) == 0 and v.stride(0) == 0 and q.stride(0) < q.stride(1)      # the suite's layout: [M, H, D] q, shared k and v
    # out permuted too: [M, H, Dv] storage viewed as [H, M, Dv]
    for out_bf16, want in ((False, base), (True, base16)):
        store = torch.zeros((m, heads, dv + PAD), dtype=torch.int16 if out_bf16 else torch.float32, device="cuda")
        out = attention_csr_bf16(a, q, k, v, scale=op["scale"], bias=bias, out_bf16=out_bf16, out=store.permute(1, 0, 2)[:, :, :dv])
        assert capi_attn_csr_bf16.last_kernel() == "attn_csr_bf16<G16,V8,C1>" and out.stride() == (dv + PAD, heads * (dv + PAD), 1)
        assert np.array_equal(out.contiguous().cpu().numpy().view(want["out"].dtype), want["out"]), "a permuted out"
        assert not store[:, :, dv:].any()
    # every operand one element off a 16-byte base: element lanes, the same bits
    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        flat[1:] = t.contiguous().reshape(-1)
        s = flat[1:].view(t.shape)
        assert s.data_ptr() % 16 == 2
        return s
    plain = [dev(bref.to_bits(op[n]) if op[n].shape[0] > 1 else bref.to_bits(op[n][0])) for n in ("q", "k", "v")]
    moved = {"q": (shifted(plain[0]), plain[1], plain[2]), "k": (plain[0], shifted(plain[1]), plain[2]), "v": (plain[0], plain[1], shifted(plain[2]))}
    for which, (q2, k2, v2) in moved.items():
        k3, v3 = (x.unsqueeze(0).expand(heads, -1, -1) for x in (k2, v2))
        out, lse = attention_csr_bf16(a, q2, k3, v3, scale=op["scale"], bias=bias, return_lse=True)
        assert capi_attn_csr_bf16.last_kernel() == bref.tag_of(d, dv, False) == "attn_csr_bf16<G64,V1,C2>", which
        assert_same_bits(out.cpu().numpy(), base["out"], f"{which} one element off a 16-byte base")
        assert_same_bits(lse.cpu().numpy(), base["lse"], f"{which} one element off a 16-byte base, lse")
    # a bf16 out one element off: a 2-byte store per element; an fp32 out one element off likewise
    k3, v3 = (x.unsqueeze(0).expand(heads, -1, -1) for x in plain[1:])
    for out_bf16, want in ((True, base16), (False, base)):
        flat = torch.zeros(heads * m * dv + 2, dtype=torch.int16 if out_bf16 else torch.float32, device="cuda")
        out = flat[1:-1].view(heads, m, dv)
        attention_csr_bf16(a, plain[0], k3, v3, scale=op["scale"], bias=bias, out_bf16=out_bf16, out=out)
        assert capi_attn_csr_bf16.last_kernel() == "attn_csr_bf16<G64,V1,C2>"
        assert np.array_equal(out.contiguous().cpu().numpy().view(want["out"].dtype), want["out"]), "out one element off a 16-byte base"
        assert not flat[0].item() and not flat[-1].item()


def test_every_tag_of_the_table_is_reached_and_reported():
    a, csr = device_csr("edges"), matrix("edges")
    rng = np.random.default_rng(180)
    seen = set()
    for tag, (d, dv, aligned) in bref.TAGS.items():
        pad = 0 if aligned else 1                    # an odd leading dimension: element lanes whatever the widths
        op = dict(q=bf16_values(rng, (1, csr.num_rows, d)), k=bf16_values(rng, (1, csr.num_cols, d)), v=bf16_values(rng, (1, csr.num_cols, dv)),
                  bias=None, scale=d ** -0.5)
        q, k, v = (dev(bref.padded_bits(op[n][0], pad))[:, :w] for n, w in (("q", d), ("k", d), ("v", dv)))
        out = attention_csr_bf16(a, q, k, v)
        assert capi_attn_csr_bf16.last_kernel() == tag == bref.tag_of(d, dv, aligned), (capi_attn_csr_bf16.last_kernel(), tag)
        assert capi.last_kernel() == tag             # the tag is left in the library every binding shares
        want = ref.attention_f64(csr, op["q"], op["k"], op["v"], op["scale"])[0]
        assert np.all(np.abs(out.cpu().numpy()[None] - want) <= ref.out_tolerance(csr, op["q"], op["k"], op["v"], op["scale"])), tag
        seen.add(tag)
    assert seen == set(bref.TAGS) and len(seen) == 9
    # multiples of 8 in a buffer with a leading dimension that is none take the element lanes; multiples of 4 always do
    q, k, v = (dev(bref.padded_bits(bf16_values(rng, (n, 8)), 4))[:, :8] for n in (csr.num_rows, csr.num_cols, csr.num_cols))
    attention_csr_bf16(a, q, k, v)
    assert capi_attn_csr_bf16.last_kernel() == "attn_csr_bf16<G8,V1,C1>"


def test_refusals_launch_nothing():
    a, csr = device_csr("edges"), matrix("edges")
    q, k, v = (torch.zeros((n, 8), dtype=torch.int16, device="cuda") for n in (csr.num_rows, csr.num_cols, csr.num_cols))
    sentinel = torch.full((csr.num_rows, 8), 7.0, device="cuda")
    ops.spmm_csr(a, torch.zeros((csr.num_cols, 8), device="cuda"))
    before = capi.last_kernel()
    with pytest.raises(capi.MispmmError, match="scale must be finite"):
        attention_csr_bf16(a, q, k, v, scale=float("inf"), out=sentinel)
    # (torch cannot make an int16 tensor at an odd address: that refusal is run with fake pointers in the CPU suite)
    with pytest.raises(ValueError, match="out must be an int16"):
        attention_csr_bf16(a, q, k, v, out=sentinel, out_bf16=True)
    with pytest.raises(ValueError, match="q must be an int16"):
        attention_csr_bf16(a, q.float(), k, v, out=sentinel)
    torch.cuda.synchronize()
    assert capi.last_kernel() == before and bool((sentinel == 7.0).all()), "a refused call must launch nothing"


def test_deterministic_replays_from_a_graph_and_a_head_does_not_depend_on_h():
    case = bref.Case("edges", 40, 72, "masked", 3)
    op, a = bref.operands(case), device_csr("edges")
    base, base16, _ = results(case)
    q, k, v, bias = layout(op)
    for out_bf16, want in ((False, base), (True, base16)):
        again = run(a, op, out_bf16=out_bf16, lay=(q, k, v, bias))
        assert np.array_equal(again["out"].view(want["out"].dtype), want["out"]) and np.array_equal(again["lse"].view(np.uint32), want["lse"].view(np.uint32))
        out2 = torch.empty((3, a.num_rows, 72), dtype=torch.int16 if out_bf16 else torch.float32, device="cuda")
        lse2 = torch.empty((3, a.num_rows), device="cuda")
        kw = dict(scale=op["scale"], bias=bias, out_bf16=out_bf16, out=out2, lse=lse2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                   # warm-up outside the capture
            attention_csr_bf16(a, q, k, v, **kw)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            attention_csr_bf16(a, q, k, v, **kw)
        out2.zero_()
        lse2.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out2.cpu().numpy().view(want["out"].dtype), want["out"]), "graph replay"
        assert_same_bits(lse2.cpu().numpy(), want["lse"], "graph replay, lse")
    # the result of a head does not depend on H: head 1 alone, head 1 among 2 (per-head bias rows of the finite case)
    fin = bref.Case("edges", 40, 72, "finite", 3)
    fop, (fbase, _, _) = bref.operands(fin), results(fin)
    for pick in ([1], [1, 2], [2, 0]):
        sub = dict(fop, q=fop["q"][pick], bias=fop["bias"][pick] if len(pick) > 1 else fop["bias"][pick[0]])
        got = run(a, sub)
        assert_same_bits(got["out"], fbase["out"][pick], f"heads {pick} of 3")
        assert_same_bits(got["lse"], fbase["lse"][pick], f"heads {pick} of 3, lse")


# ---- autograd
GRADS = ("dq", "dk", "dv")


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["g32", "g16"])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("heads", [1, 2])
def test_sparse_attention_bf16_forward_and_gradients(heads, with_bias, grad_dtype):
    name, d = "long", 8
    csr = matrix(name)
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(246 + heads)
    q, k, v, g = (bf16_values(rng, (heads, n, d)) for n in (csr.num_rows, csr.num_cols, csr.num_cols, csr.num_rows))
    bias = rng.uniform(-2, 2, (heads, csr.nnz)).astype(np.float32) if with_bias else None
    scale = d ** -0.5
    squeeze = (lambda x: x[0]) if heads == 1 else (lambda x: x)
    bd = None if bias is None else dev(squeeze(bias))
    bits = lambda t: t.detach().view(torch.int16)                                  # noqa: E731
    qd, kd, vd = (dev(squeeze(x)).to(torch.bfloat16).requires_grad_(True) for x in (q, k, v))
    gd = dev(squeeze(g)).to(grad_dtype)
    out_dtype = grad_dtype                                                           # a bf16 result takes a bf16 grad_out
    with torch.autograd.set_multithreading_enabled(False):
        out = autograd.sparse_attention_bf16(a, qd, kd, vd, bias=bd, out_dtype=out_dtype)
        if out_dtype == torch.float32:
            assert capi.last_kernel() == "attn_csr_bf16<G8,V8,C1>"
        out.backward(gd)
        assert capi_attn_csr_bwd.last_kernel().startswith("attn_csr_bwd_col<")
    # the forward is the kernel's fp32 out (and lse), a bf16 result that out rounded once
    out32, lse = attention_csr_bf16(a.fwd, bits(qd), bits(kd), bits(vd), scale=scale, bias=bd, return_lse=True)
    assert capi_attn_csr_bf16.last_kernel() == "attn_csr_bf16<G8,V8,C1>"
    if out_dtype == torch.float32:
        assert out.dtype == torch.float32
        assert_same_bits(out.detach().cpu().numpy(), out32.cpu().numpy(), "forward")
    else:
        assert out.dtype == torch.bfloat16
        assert np.array_equal(bits(out).cpu().numpy().view(np.uint16), bref.bf16_bits(out32.cpu().numpy())), "the fp32 out rounded once"
        assert np.array_equal(bits(out).cpu().numpy(), attention_csr_bf16(a.fwd, bits(qd), bits(kd), bits(vd), scale=scale, bias=bd, out_bf16=True).cpu().numpy())
    # the gradients are the composition that defines them, made by hand, bit for bit
    qf, kf, vf = (ops.bf16_to_f32(bits(t)) for t in (qd, kd, vd))
    gf = ops.bf16_to_f32(bits(gd)) if grad_dtype == torch.bfloat16 else gd
    hand = ops.attention_csr_bwd(a.fwd, a.tpattern, a.perm32(), qf, kf, vf, out32, lse, gf, scale=scale, bias=bd)
    got = []
    for n, t, h in zip(GRADS, (qd, kd, vd), hand):
        assert t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape
        assert np.array_equal(bits(t.grad).cpu().numpy(), ops.f32_to_bf16(h).cpu().numpy()), f"{n} against the composition made by hand"
        got.append(bref.widen(bits(t.grad).cpu().numpy()).reshape(heads, *t.shape[-2:]))
    # ... and lie within the fused fp32 backward's derived tolerances of float64 on the widened operands, plus one bf16 rounding
    want = bwd.backward_f64(csr, q, k, v, g, scale, bias)
    tols = bwd.bwd_tolerances(csr, q, k, v, g, scale, bias)
    for n, x, w, t in zip(GRADS, got, want, tols):
        ok, worst = tight._worst(x, w, bref.with_one_bf16_rounding(w, t))
        print(f"sparse_attention_bf16 H={heads} bias={with_bias} g={grad_dtype} {n}: max |err| / tolerance = {worst:.3g}")
        assert ok, n


def test_frozen_inputs_get_none_and_their_pass_is_skipped():
    csr = matrix("long")
    a = autograd.TrainableCSR.from_host(csr)
    rng = np.random.default_rng(247)
    q, k, v = (bf16_values(rng, (n, 8)) for n in (csr.num_rows, csr.num_cols, csr.num_cols))
    seen = []
    real = ops.attention_csr_bwd
    ops.attention_csr_bwd = lambda *args, **kw: seen.append(tuple(kw["need"])) or real(*args, **kw)
    try:
        with torch.autograd.set_multithreading_enabled(False):
            for trainable in ((False, False, True), (True, False, False), (False, True, False), (True, True, True)):
                qd, kd, vd = (dev(x).to(torch.bfloat16).requires_grad_(t) for x, t in zip((q, k, v), trainable))
                autograd.sparse_attention_bf16(a, qd, kd, vd).float().sum().backward()                  # an expanded grad_out
                assert seen[-1] == trainable and [x.grad is not None for x in (qd, kd, vd)] == list(trainable)
                # dq alone ends with the row pass: the column pass on A^T's pattern was not launched
                assert capi_attn_csr_bwd.last_kernel().startswith("attn_csr_bwd_row<" if trainable == (True, False, False) else "attn_csr_bwd_col<")
            count = len(seen)
            out = autograd.sparse_attention_bf16(a, *(dev(x).to(torch.bfloat16) for x in (q, k, v)))
            assert out.grad_fn is None and not out.requires_grad and out.dtype == torch.bfloat16 and len(seen) == count
    finally:
        ops.attention_csr_bwd = real
    qb, kb, vb = (dev(x).to(torch.bfloat16) for x in (q, k, v))
    with pytest.raises(ValueError, match="constant"):
        autograd.sparse_attention_bf16(a, qb, kb, vb, bias=torch.zeros(csr.nnz, device="cuda", requires_grad=True))
    with pytest.raises(ValueError, match="q must be torch.bfloat16"):
        autograd.sparse_attention_bf16(a, qb.float(), kb, vb)
    with pytest.raises(ValueError, match="out_dtype"):
        autograd.sparse_attention_bf16(a, qb, kb, vb, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="float32 matrix"):
        autograd.sparse_attention_bf16(autograd.TrainableCSR.from_host(csr, dtype=torch.float64), qb, kb, vb)
