"""The split-row fused attention forward on a CSR pattern (include/mispmm_attn_csr_split.h) on the GPU, fp32 and bf16 operands, held
to the float64 reference and the two tolerances of the one-launch forward with nothing added (`-s` prints every worst |err| /
tolerance; DESIGN.md section 9 item 31 keeps the worst).  tight.tight_forward is NOT applied to split rows: its reference puts
the roundings of fl(z - mu) at the ONE-LAUNCH kernel's running maxima, and a split row's maximum restarts in every segment.  In
its place, exact: rows of one segment have the one-launch kernel's bits, and the tie rows their exact answers at every split."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import attn_csr_split, autograd, capi, capi_attn_csr_split, ops  # noqa: E402
from mispmm.attn_csr_bf16 import attention_csr_bf16  # noqa: E402

import _attn_csr_bf16_ref as bref  # noqa: E402
import _attn_csr_bwd_ref as bwd  # noqa: E402
import _attn_csr_mutants as mut  # noqa: E402
import _attn_csr_ref as ref  # noqa: E402
import _attn_csr_tight as tight  # noqa: E402
from _attn_csr_ref import Case  # noqa: E402
from _bits import assert_same_bits  # noqa: E402
from _softmax_ref import full_mantissa, matrix  # noqa: E402
from test_gpu_attn_csr import dev, device_csr, device_operands  # noqa: E402
from test_gpu_attn_csr_bf16 import layout as bf16_layout  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ("f32", "bf16")
SPLITS = ((2, 1), (3, 1), (8, 4), (256, 1))
WIDTHS = ((8, 64), (3, 5), (256, 256), (40, 72))
# every instance tag -> the smallest (D, Dv, aligned) that reaches it, as ref.TAGS and bref.TAGS for the one-launch kernels
_V1 = {"G8,V1,C1": (1, 1, False), "G16,V1,C1": (1, 9, False), "G32,V1,C1": (1, 17, False), "G64,V1,C1": (1, 33, False),
       "G64,V1,C2": (1, 65, False), "G64,V1,C4": (1, 129, False)}
TAGS = {"f32": {"G8,V4,C1": (4, 4, True), "G16,V4,C1": (4, 36, True), "G32,V4,C1": (4, 68, True), "G64,V4,C1": (4, 132, True), **_V1},
        "bf16": {"G8,V8,C1": (8, 8, True), "G16,V8,C1": (8, 72, True), "G32,V8,C1": (8, 136, True), **_V1}}
# (out against float64 inside the composed tolerance, lse inside the header's bound) on the kind's own operands: (ok, worst)
CHECKS = {"f32": (mut.out_composed, mut.lse_bound), "bf16": (bref.out_composed, bref.lse_bound)}


def operands(kind, case):
    return (ref if kind == "f32" else bref).operands(case)


def element(kind, x):
    return dev(x if kind == "f32" else bref.to_bits(x))          # float32, or int16 bf16 bits


def layout(kind, op):
    """The sibling suites' layouts: q a view of [M, H, D] storage, k and v one head expanded over all; bf16 with NaN pad columns."""
    return (device_operands if kind == "f32" else bf16_layout)(op)


def split(kind, a, q, k, v, **kw):
    return (attn_csr_split.attention_csr_split if kind == "f32" else attn_csr_split.attention_csr_split_bf16)(a, q, k, v, **kw)


def one_launch(kind, a, q, k, v, **kw):
    return (ops.attention_csr if kind == "f32" else attention_csr_bf16)(a, q, k, v, **kw)


def host(x, heads):
    x = x.cpu().numpy()
    x = bref.widen(x.view(np.uint16)) if x.dtype == np.int16 else x        # a bf16 out widened exactly: the same bits to compare
    return x if heads > 1 else x[None]


def run(fn, kind, a, op, **kw):
    q, k, v, bias = layout(kind, op)
    heads = op["q"].shape[0]
    out, lse = fn(kind, a, q, k, v, scale=op["scale"], bias=bias, return_lse=True, **kw)
    return dict(out=host(out, heads).reshape(heads, a.num_rows, -1), lse=host(lse, heads))


@pytest.mark.parametrize("si", range(len(SPLITS)), ids=[f"S{s}m{b}" for s, b in SPLITS])
@pytest.mark.parametrize("wi", range(len(WIDTHS)), ids=[f"D{d}Dv{dv}" for d, dv in WIDTHS])
@pytest.mark.parametrize("kind", KINDS)
def test_edges_against_float64_inside_both_tolerances(kind, wi, si):
    (d, dv), (s, mb) = WIDTHS[wi], SPLITS[si]
    case = Case("edges", d, dv, ("none", "masked")[(wi + si) % 2], (1, 3)[(wi + si // 2) % 2])      # bias and heads vary along
    got = run(split, kind, device_csr("edges"), operands(kind, case), splits=s, min_batches=mb)
    assert capi_attn_csr_split.last_kernel() == f"attn_csr_combine<f32,S{s}>"
    (ok_out, w_out), (ok_lse, w_lse) = (check(got, case) for check in CHECKS[kind])
    print(f"attn_csr_split {kind} {case.id} S={s} min_batches={mb}: worst |err| / tolerance out {w_out:.3g}, lse {w_lse:.3g}")
    assert ok_out and ok_lse, f"{kind} {case.id} S={s} min_batches={mb}: out {w_out:.3g}, lse {w_lse:.3g} of the tolerance"
    empty = np.diff(matrix("edges").row_ptrs.astype(np.int64)) == 0
    assert empty.any() and not got["out"][:, empty].view(np.uint32).any(), "an empty row must be +0"


@pytest.mark.parametrize("kind", KINDS)
def test_one_segment_is_the_one_launch_kernel_bit_for_bit(kind):
    case = Case("edges", 40, 72, "masked", 3)
    a, op = device_csr("edges"), operands(kind, case)
    lens = np.diff(matrix("edges").row_ptrs.astype(np.int64))
    for narrow in ({},) if kind == "f32" else ({}, dict(out_bf16=True)):
        want = run(one_launch, kind, a, op, **narrow)
        got = run(split, kind, a, op, splits=1, **narrow)
        assert_same_bits(got["out"], want["out"], f"{kind} {narrow}: out of splits=1")
        assert_same_bits(got["lse"], want["lse"], f"{kind} {narrow}: lse of splits=1")
        got = run(split, kind, a, op, splits=8, min_batches=4, **narrow)        # n < 2 * 4 batches: fewer than 57 entries
        short = lens < 57
        assert short.any() and (~short).any()
        assert_same_bits(got["out"][:, short], want["out"][:, short], f"{kind} {narrow}: rows of one segment at (8, 4)")
        assert_same_bits(got["lse"][:, short], want["lse"][:, short], f"{kind} {narrow}: lse of rows of one segment at (8, 4)")


@pytest.mark.parametrize("s", [2, 3, 8])
@pytest.mark.parametrize("t", tight.TIES)
@pytest.mark.parametrize("kind", KINDS)
def test_tie_rows_bit_for_bit(kind, t, s):
    a = ops.DeviceCSR.from_host(tight.tie_pattern(t)[0], plan=False)
    for through_bias in (False, True):
        got = run(split, kind, a, tight.tie_operands(t, through_bias), splits=s, min_batches=1)
        ok, wrong = tight.tie_check(got, t, through_bias)
        assert ok, f"{kind} t={t} through_bias={through_bias} S={s}: {wrong} elements differ from the exact answers"


@pytest.mark.parametrize("d,dv,vec", [(8, 64, 8), (3, 5, 1), (40, 72, 8)])
def test_a_bf16_out_of_split_rows_is_the_fp32_out_rounded_once(d, dv, vec):
    """The bf16 combine kernel: its 8-byte store (16-byte lanes) and its guarded element stores (Dv = 5 of Dvp = 8), sentinels
    beside every row."""
    case = Case("edges", d, dv, "masked", 3)
    a, op, m = device_csr("edges"), bref.operands(case), matrix("edges").num_rows
    q, k, v, bias = layout("bf16", op)
    kw = dict(scale=op["scale"], bias=bias, splits=3, min_batches=1, return_lse=True)
    out32, lse32 = split("bf16", a, q, k, v, **kw)
    store = torch.full((3, m, dv + bref.PAD), bref.OUT_SENTINEL_BF16, dtype=torch.int16, device="cuda")
    _, lse16 = split("bf16", a, q, k, v, out_bf16=True, out=store[:, :, :dv], **kw)
    assert capi_attn_csr_split.last_kernel() == "attn_csr_combine<bf16,S3>"
    assert capi_attn_csr_split.last_partial() == f"attn_csr_split<bf16,G{8 if dv < 72 else 16},V{vec},C1,S3>"
    assert bool((store[:, :, dv:] == bref.OUT_SENTINEL_BF16).all()), "the pad columns of a bf16 out must keep their sentinel"
    ok, wrong = bref.rounded_once(dict(out=out32.cpu().numpy(), out_bf16=store[:, :, :dv].cpu().numpy().view(np.uint16)))
    assert ok, f"D={d} Dv={dv}: {int(wrong)} elements of the bf16 out are not the fp32 out rounded to nearest even"
    assert_same_bits(lse16, lse32, "lse does not depend on the out type")


@pytest.mark.parametrize("kind", KINDS)
def test_special_values_stay_in_their_rows_and_wholly_masked_segments_contribute_nothing(kind):
    """A NaN (row of 33), a +Inf (17), nothing but -Inf (9), +Inf and NaN in different segments (300); then the first two of the
    8 segments of the 1025-entry row (129 batches: batches 0 .. 31) wholly masked."""
    case, csr = Case("edges", 8, 8, "finite", 1), matrix("edges")
    a, op = device_csr("edges"), operands(kind, case)
    ptrs = csr.row_ptrs.astype(np.int64)
    lens = np.diff(ptrs)
    at = {n: int(ptrs[np.argwhere(lens == n)[0, 0]]) for n in (33, 17, 9, 300, 1025)}
    bias = op["bias"].copy()
    bias[at[33] + 20], bias[at[17] + 3], bias[at[9]:at[9] + 9], bias[at[300] + 5], bias[at[300] + 250] = np.nan, np.inf, -np.inf, np.inf, np.nan
    clean = run(split, kind, a, op, splits=8, min_batches=1)
    got, want = run(split, kind, a, dict(op, bias=bias), splits=8, min_batches=1), run(one_launch, kind, a, dict(op, bias=bias))
    hit = np.isin(lens, (33, 17, 9, 300))
    assert np.array_equal(np.isnan(got["out"][0]), np.broadcast_to(hit[:, None], got["out"][0].shape))
    assert np.array_equal(np.isnan(want["out"]), np.isnan(got["out"])) and np.array_equal(got["lse"][0, hit], want["lse"][0, hit], equal_nan=True)
    assert_same_bits(got["out"][0][~hit], clean["out"][0][~hit], "rows without a special value")
    assert_same_bits(got["lse"][0][~hit], clean["lse"][0][~hit], "lse of rows without a special value")
    bias = op["bias"].copy()
    bias[at[1025]:at[1025] + 32 * 8] = -np.inf
    masked = run(split, kind, a, dict(op, bias=bias), splits=8, min_batches=1)
    err = np.abs(masked["out"] - ref.attention_f64(csr, op["q"], op["k"], op["v"], op["scale"], bias)[0])
    assert np.all(err <= ref.out_tolerance(csr, op["q"], op["k"], op["v"], op["scale"], bias)), "two wholly masked segments"


@pytest.mark.parametrize("kind", KINDS)
def test_buffers_refusals_heads_and_graph_replay(kind):
    case, s, pad = Case("edges", 40, 72, "masked", 3), 3, 64
    a, op, m = device_csr("edges"), operands(kind, case), matrix("edges").num_rows
    q, k, v, bias = layout(kind, op)
    kw = dict(scale=op["scale"], bias=bias, splits=s, min_batches=2)
    singles = [split(kind, a, q[h].contiguous(), k[0], v[0], return_lse=True, **kw) for h in range(3)]
    need = attn_csr_split.workspace_bytes(a, 3, 72, s)
    assert need == 4 * 3 * m * s * (72 + 2)
    wbuf = torch.full((pad + need + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    obuf, lbuf = (torch.full((pad + 3 * m * w + pad,), -7.0, device="cuda") for w in (80, 1))
    view, linner = obuf[pad:-pad].view(3, m, 80), lbuf[pad:-pad].view(3, m)
    go = lambda **more: split(kind, a, q, k, v, out=view[:, :, :72], lse=linner, **{**kw, "workspace": wbuf[pad:pad + need], **more})   # noqa: E731
    go()
    for h in range(3):                                          # three strided heads against three calls of one head
        assert_same_bits(view[h, :, :72].contiguous(), singles[h][0], f"head {h} of 3 against a call of its own")
        assert_same_bits(linner[h], singles[h][1], f"lse of head {h}")
    for what, buf, mark in (("out", obuf, -7.0), ("lse", lbuf, -7.0), ("the workspace", wbuf, 0xA5)):
        assert bool((buf[:pad] == mark).all()) and bool((buf[-pad:] == mark).all()), f"a sentinel of {what} was written"
    assert bool((view[:, :, 72:] == -7.0).all()), "a gap of the strided out was written"
    want, want_lse = view[:, :, :72].clone(), linner.clone()
    before = capi.last_kernel()
    view.fill_(-7.0)
    for bad, error, text in ((dict(workspace=wbuf[pad:pad + need - 1]), capi.MispmmError, f"hold {need} bytes"),
                             (dict(workspace=wbuf[pad + 4:pad + 4 + need]), capi.MispmmError, "a misaligned pointer"),
                             (dict(splits=0), ValueError, "splits must be"), (dict(splits=257), ValueError, "splits must be"),
                             (dict(min_batches=0), ValueError, "min_batches must be")):
        with pytest.raises(error, match=text):
            go(**bad)
    torch.cuda.synchronize()
    assert capi.last_kernel() == before and bool((view == -7.0).all()), "a refused call must launch nothing"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                   # two launches in a row: no parallel branches
        go()
    for _ in range(2):
        view.zero_()
        linner.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_same_bits(view[:, :, :72].contiguous(), want, "graph replay")
        assert_same_bits(linner, want_lse, "graph replay, lse")


@pytest.mark.parametrize("kind", KINDS)
def test_every_instance_tag_is_reached_at_its_smallest_shape(kind):
    a, csr = device_csr("edges"), matrix("edges")
    rng = np.random.default_rng(81)
    for tag, (d, dv, aligned) in TAGS[kind].items():
        pad = 0 if aligned else 1                    # an odd leading dimension: element lanes whatever the widths
        full = [bref.widen(bref.bf16_bits(full_mantissa(rng, (n, w + pad), np.float32))) for n, w in ((csr.num_rows, d), (csr.num_cols, d), (csr.num_cols, dv))]
        q, k, v = (element(kind, x)[:, :w] for x, w in zip(full, (d, d, dv)))
        out = split(kind, a, q, k, v, splits=2, min_batches=1)
        assert capi_attn_csr_split.last_partial() == f"attn_csr_split<{kind},{tag},S2>"
        assert capi_attn_csr_split.last_kernel() == capi.last_kernel() == "attn_csr_combine<f32,S2>"
        qh, kh, vh = (x[None, :, :w] for x, w in zip(full, (d, d, dv)))
        want = ref.attention_f64(csr, qh, kh, vh, d ** -0.5)[0]
        assert np.all(np.abs(out.cpu().numpy()[None] - want) <= ref.out_tolerance(csr, qh, kh, vh, d ** -0.5)), tag


def test_autograd_with_splits_has_the_gradients_of_the_one_launch_forward():
    csr, d = matrix("long"), 8                                  # its rows of 77, 129 and 300 entries are split at min_batches = 4
    a, rng = autograd.TrainableCSR.from_host(csr), np.random.default_rng(346)
    q, k, v, g = (bref.widen(bref.bf16_bits(full_mantissa(rng, (2, n, d), np.float32))) for n in (csr.num_rows, csr.num_cols, csr.num_cols, csr.num_rows))
    want, tols = bwd.backward_f64(csr, q, k, v, g, d ** -0.5, None), bwd.bwd_tolerances(csr, q, k, v, g, d ** -0.5, None)

    def grads(fn, dtype, **kw):
        qd, kd, vd = (dev(x).to(dtype).requires_grad_(True) for x in (q, k, v))
        with torch.autograd.set_multithreading_enabled(False):
            out = fn(a, qd, kd, vd, **kw)
            tag = capi.last_kernel()
            out.backward(dev(g).to(out.dtype))
        return tag, [t.grad.float().cpu().numpy() for t in (qd, kd, vd)]

    def inside(gs, what, widen=lambda w, t: t):
        for x, w, t, n in zip(gs, want, tols, "qkv"):
            ok, worst = tight._worst(x, w, widen(w, t))
            print(f"{what} d{n}: max |err| / tolerance = {worst:.3g}")
            assert ok, f"{what}: d{n} outside the tolerance"

    f32, b16 = autograd.sparse_attention, autograd.sparse_attention_bf16
    one, got = grads(f32, torch.float32, fused=True), grads(f32, torch.float32, fused=True, splits=3)
    assert one[0].startswith("attn_csr<") and got[0] == "attn_csr_combine<f32,S3>"
    for x, y, n in zip(got[1], one[1], "qkv"):
        assert_same_bits(x, y, f"d{n}: splits=3 against splits=None, recomputing backward")
    for x, y, n in zip(grads(b16, torch.bfloat16, splits=1)[1], grads(b16, torch.bfloat16)[1], "qkv"):
        assert_same_bits(x, y, f"bf16 d{n}: splits=1 against splits=None")
    for splits in (3, "auto"):
        inside(grads(f32, torch.float32, fused=True, fused_backward=True, splits=splits)[1], f"sparse_attention fused_backward splits={splits}")
    for kw in (dict(splits=3), dict(splits=3, fused_backward=True)):
        inside(grads(b16, torch.bfloat16, **kw)[1], f"sparse_attention_bf16 {kw}", bref.with_one_bf16_rounding)
