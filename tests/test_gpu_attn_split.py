"""The split-row fused attention forward (mispmm_attn_bsr_split_bf16; include/mispmm_attn_split.h) on the GPU, held to the references,
tolerances and checks of the one-wave forward with nothing added.  Worst |err| / tolerance on an MI355X (`-s` prints every one;
DESIGN.md section 9 item 30): out fp32 0.428, bf16 0.483; lse 0.040; a constant V 0.045: the one-wave kernel's, at S = 1."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, capi, capi_attn_split, ops  # noqa: E402
from mispmm.attn_bsr_split import attention_bsr_split_bf16 as split, workspace_bytes  # noqa: E402

import _attn_checks as checks  # noqa: E402
import _attn_fused_ref as ref  # noqa: E402
import _attn_tight as tight  # noqa: E402
from _attn_checks import Case  # noqa: E402
from _softmax_bsr_ref import pattern  # noqa: E402
from test_gpu_attn_fused import dbits, host  # noqa: E402
from test_gpu_attn_fused_bwd import dmask  # noqa: E402
from test_gpu_softmax_bsr import _attention_tolerances, _dense_attention, bf, bits, dev, device_bsr, same_bits, trainable  # noqa: E402

pytestmark = pytest.mark.gpu

SPLITS = [1, 2, 3, 8, 64]
SENTINELS = 64


@pytest.mark.parametrize("s", SPLITS)
@pytest.mark.parametrize("kind", ref.MASKS)
@pytest.mark.parametrize("d,dv", [(8, 64), (128, 128), (40, 72)])
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_out_and_lse_against_float64_dense_masked_attention(name, d, dv, kind, s):
    a = device_bsr(name)
    q, k, v = (dbits(x[0]) for x in ref.operands(name, d, dv))
    empty = checks.empty_block_rows(pattern(name))
    for out_bf16 in (False, True):
        out, lse = split(a, q, k, v, mask=dmask(name, kind), out_bf16=out_bf16, return_lse=True, splits=s)
        assert capi_attn_split.last_kernel() == f"attn_bsr_combine<{'bf16' if out_bf16 else 'f32'},S{s}>"
        case, got = Case(name, d, dv, kind, out_bf16=out_bf16), dict(out=host(out), lse=lse.cpu().numpy())
        (ok_out, w_out), (ok_lse, w_lse) = checks.out_composed(got, case), checks.lse_bound(got, case)
        print(f"split attention {name} D={d} Dv={dv} {kind} S={s} bf16={out_bf16}: max |err| / tolerance out {w_out:.3g}, lse {w_lse:.3g}")
        assert ok_out and ok_lse, f"{case.id} S={s}: out {w_out:.3g}, lse {w_lse:.3g} of the tolerance"
        assert empty.any() and not out.cpu().numpy().view(np.uint16 if out_bf16 else np.uint32)[empty].any()    # +0 bits
        assert np.array_equal(np.isneginf(got["lse"]), empty)


@pytest.mark.parametrize("kind", ["none", "causal"])
@pytest.mark.parametrize("name", ["edges16", "edges32"])
def test_one_split_is_the_one_wave_kernel_bit_for_bit(name, kind):
    a = device_bsr(name)
    q, k, v = (dbits(x[0]) for x in ref.operands(name, 40, 72))
    for out_bf16 in (False, True):
        want = ops.attention_bsr_bf16(a, q, k, v, mask=dmask(name, kind), out_bf16=out_bf16, return_lse=True)
        got = split(a, q, k, v, mask=dmask(name, kind), out_bf16=out_bf16, return_lse=True, splits=1)
        same_bits(got[0], want[0], f"{name} {kind} bf16={out_bf16}: out of splits=1")
        same_bits(got[1], want[1], f"{name} {kind}: lse of splits=1")


@pytest.mark.parametrize("s", [2, 3, 8])
@pytest.mark.parametrize("through_mask", [False, True])
@pytest.mark.parametrize("t", tight.TIES)
def test_tie_rows_bit_for_bit(t, through_mask, s):
    for name in ("edges16", "edges32"):
        op = tight.tie_operands(name, t, through_mask)
        q, k, v = (dbits(op[n]) for n in ("q", "k", "v"))
        mask = None if op["mask"] is None else dev(np.array(op["mask"]))
        for out_bf16 in (False, True):
            out, lse = split(device_bsr(name), q, k, v, scale=op["scale"], mask=mask, out_bf16=out_bf16, return_lse=True, splits=s)
            ok, wrong = tight.tie_forward(dict(out=host(out), lse=lse.cpu().numpy()), name, t, through_mask, out_bf16)
            assert ok, f"tie rows {name} t={t} through_mask={through_mask} S={s} bf16={out_bf16}: {wrong} elements differ from the exact answer"


@pytest.mark.parametrize("s", SPLITS)
@pytest.mark.parametrize("name", ["edges16", "edges32"])
def test_a_constant_v_comes_back_to_fp32_accuracy(name, s):
    a, p = device_bsr(name), pattern(name)
    q, k, _ = (dbits(x[0]) for x in ref.operands(name, 64, 64))
    for dv, value in ((64, 1.0), (128, -0.34765625)):
        out = split(a, q, k, dbits(np.full((p.num_cols, dv), value, np.float32)), mask=dmask(name, "causal"), splits=s).cpu().numpy()
        ok, worst = checks.constant_v(dict(out=out), Case(name, 64, dv, "causal", const_v=value))
        assert ok, f"constant V {name} Dv={dv} S={s}: max rel / ((L + 16) u) = {worst:.3g}"


@functools.lru_cache(maxsize=None)
def special_case(name):
    """(block row r, mask, float64 out, {out_bf16: tolerance}): query row 10 of the longest block row has its first segments masked."""
    p = pattern(name)
    ptrs = p.block_row_ptrs.astype(np.int64)
    r = int(np.argmax(np.diff(ptrs)))
    base = np.zeros((p.num_blocks, p.block_row_size, p.block_row_size), np.float32)
    base[ptrs[r]:ptrs[r] + (ptrs[r + 1] - ptrs[r] + 1) // 2, 10, :] = -np.inf
    q, k, v = (x[0] for x in ref.operands(name, 40, 72))
    g0 = np.zeros((p.num_rows, 72), np.float32)
    return r, base, _dense_attention(p, q, k, v, g0, 0.3, base)[0], {ob: _attention_tolerances(name, q, k, v, g0, 0.3, base, ob)[0] for ob in (False, True)}


@pytest.mark.parametrize("s", [2, 8])
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("name", ["edges16", "edges32"])
def test_special_values_stay_in_their_matrix_row(name, out_bf16, s):
    """In the longest block row: a NaN score, a +Inf score, an all -Inf row, and the half-masked row of special_case()."""
    p, a = pattern(name), device_bsr(name)
    r, base, want, tols = special_case(name)
    lo, hi, bs = int(p.block_row_ptrs[r]), int(p.block_row_ptrs[r + 1]), p.block_row_size
    q, k, v = (dbits(x[0]) for x in ref.operands(name, 40, 72))
    m = base.copy()
    m[(lo + hi) // 2, 1, bs - 1], m[hi - 1, 4, 0], m[lo:hi, 7, :] = np.nan, np.inf, -np.inf
    clean, clean_lse = (host(x) for x in split(a, q, k, v, scale=0.3, mask=dev(base), out_bf16=out_bf16, return_lse=True, splits=s))
    got, lse = (host(x) for x in split(a, q, k, v, scale=0.3, mask=dev(m), out_bf16=out_bf16, return_lse=True, splits=s))
    hit = np.zeros(p.num_rows, bool)
    hit[r * bs + np.array([1, 4, 7])] = True
    assert np.array_equal(np.isnan(got), np.broadcast_to(hit[:, None], got.shape)), "NaN positions differ"
    assert np.array_equal(got[~hit], clean[~hit]) and np.array_equal(lse[~hit], clean_lse[~hit]), "another row changed"
    assert np.array_equal(lse[hit], np.array([np.nan, np.inf, -np.inf], np.float32), equal_nan=True), lse[hit]
    assert np.all(np.abs(clean.astype(np.float64) - want) <= tols[out_bf16]) and np.isfinite(clean_lse[r * bs + 10])


def test_heads_strides_workspace_and_graph():
    """A permuted [M, H, D] q and head-stride-0 k, v against single-head calls; sentinels; an exact workspace; a graph replayed twice."""
    name, d, dv, heads, s = "edges16", 40, 72, 3, 3
    a, p = device_bsr(name), pattern(name)
    qh, kh, vh = ref.operands(name, d, dv, heads)
    mask = dmask(name, "causal")
    q = dbits(np.ascontiguousarray(qh.transpose(1, 0, 2))).permute(1, 0, 2)
    k, v = dbits(kh[0]).unsqueeze(0).expand(heads, -1, -1), dbits(vh[0]).unsqueeze(0).expand(heads, -1, -1)
    assert not q.is_contiguous() and k.stride(0) == 0
    singles = [split(a, dbits(qh[h]), dbits(kh[0]), dbits(vh[0]), mask=mask, return_lse=True, splits=s) for h in range(heads)]
    need = workspace_bytes(a, heads, dv, s)
    assert need == 4 * heads * p.num_rows * s * (dv + 3)
    wbuf = torch.full((SENTINELS + need + SENTINELS,), 0xA5, dtype=torch.uint8, device="cuda")
    obuf = torch.full((SENTINELS + heads * p.num_rows * 80 + SENTINELS,), -7.0, device="cuda")
    view = obuf[SENTINELS:-SENTINELS].view(heads, p.num_rows, 80)
    lbuf = torch.full((SENTINELS + heads * p.num_rows + SENTINELS,), -7.0, device="cuda")
    linner = lbuf[SENTINELS:-SENTINELS].view(heads, p.num_rows)
    run = lambda: split(a, q, k, v, mask=mask, splits=s, out=view[:, :, :dv], lse=linner, workspace=wbuf[SENTINELS:SENTINELS + need])   # noqa: E731
    run()
    for h in range(heads):
        same_bits(view[h, :, :dv].contiguous(), singles[h][0], f"head {h} of 3 against a call of its own")
        same_bits(linner[h], singles[h][1], f"lse of head {h}")
    for what, buf, mark in (("out", obuf, -7.0), ("lse", lbuf, -7.0), ("the workspace", wbuf, 0xA5)):
        assert bool((buf[:SENTINELS] == mark).all()) and bool((buf[-SENTINELS:] == mark).all()), f"a sentinel of {what} was written"
    assert bool((view[:, :, dv:] == -7.0).all()), "a gap of the strided out was written"
    with pytest.raises(capi.MispmmError, match=f"hold {need} bytes"):
        split(a, q, k, v, mask=mask, splits=s, workspace=wbuf[SENTINELS:SENTINELS + need - 1])
    want, want_lse = view[:, :, :dv].clone(), linner.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                   # two launches in a row: no parallel branches
        run()
    for _ in range(2):
        view.zero_()
        linner.zero_()
        g.replay()
        torch.cuda.synchronize()
        same_bits(view[:, :, :dv].contiguous(), want, "graph replay")
        same_bits(linner, want_lse, "graph replay, lse")


def test_autograd_with_splits_has_the_gradients_of_the_one_wave_forward():
    name, d, dv = "ragged16", 64, 64
    case = Case(name, d, dv, "causal", src="bwd", grads_bf16=True)
    qh, kh, vh, gh = case.arrays
    mask = dev(np.array(case.mask))
    grads = {}
    for key, kw in (("one", {}), ("split", dict(splits=3)), ("fused", dict(splits=3, fused_backward=True)), ("auto", dict(splits="auto"))):
        q, k, v = (bf(np.array(x)).requires_grad_(True) for x in (qh, kh, vh))
        out = autograd.block_sparse_attention(trainable(name), q, k, v, mask=mask, fused=True, **kw)
        assert capi_attn_split.last_kernel().startswith("attn_bsr_combine<f32,S3>" if kw.get("splits") == 3 else "attn_bsr<")
        out.backward(dev(np.array(gh)))
        grads[key] = (q.grad, k.grad, v.grad)
    for x, y, z in zip(grads["split"], grads["one"], grads["auto"]):
        same_bits(bits(x), bits(y), "splits=3 against splits=None, recomputing backward")
        same_bits(bits(z), bits(y), "splits='auto' (one wave on this pattern) against splits=None")
    ok, worst = checks.bwd_composed(dict(zip(("dq", "dk", "dv"), (x.float().cpu().numpy() for x in grads["fused"]))), case)
    assert ok, f"splits=3 with the fused backward: max |err| / tolerance dq, dk, dv = {worst}"
