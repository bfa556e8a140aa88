"""The two fused attention kernels on the GPU against the DERIVED tight check and the exact tie rows of tests/_attn_tight.py --
the functions tests/test_attn_mutants_cpu.py shows to catch every fault of tests/_attn_mutants.py, the eight the composed
tolerances let through among them.  Through ops.attention_bsr_bf16, ops.attention_bsr_bwd_bf16 and
block_sparse_attention(fused=True, fused_backward=True); the six small patterns, the four width pairs, the three masks, both out
types, both gradient types.  The backward is checked on the kernel's own stored out and lse, so a failure there is the backward's.

`-s` prints, per case, worst |err| / tight tolerance and the flagged share of the live elements (at most 1 %, asserted).  Worst
printed on an MI355X: forward fp32 out 0.939, lse 0.217; backward fp32 dq 0.988, dk 0.988,
dv 0.987 -- a flagged element that flips uses the whole of its one ulp, so figures just below 1 are what a kernel that keeps the
contract gives; every bf16 output lies between the two rounded ends of its fp32 interval; flagged at most 0.12 %; the tie rows
hold bit for bit in all 60 (pattern, t, way) combinations, every out and gradient type."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mispmm import autograd, ops  # noqa: E402

import _attn_checks as checks  # noqa: E402
import _attn_fused_bwd_ref as ref  # noqa: E402
import _attn_tight as tight  # noqa: E402
from _attn_checks import Case  # noqa: E402
from test_gpu_attn_fused_bwd import backward, dbits, forward, host, trainable  # noqa: E402
from test_gpu_softmax_bsr import bf, dev  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a):
    return dev(np.array(a))                                     # a copy: the shared operands are read-only


def _bf(a):
    return bf(np.array(a))


def _dmask(case):
    return None if case.mask is None else _dev(case.mask)


@pytest.mark.parametrize("kind", ref.MASKS)
@pytest.mark.parametrize("d,dv", ref.WIDTHS)
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_forward_and_backward_inside_the_derived_tight_tolerance(name, d, dv, kind):
    base = Case(name, d, dv, kind, src="bwd")
    q, k, v, g = (dbits(x) for x in base.arrays)
    mask = _dmask(base)
    for out_bf16 in (False, True):
        out, lse = forward(name, q, k, v, mask, out_bf16)
        stored = dict(out=host(out), lse=lse.cpu().numpy())
        ok, (w_out, w_lse, share) = tight.tight_forward(stored, Case(name, d, dv, kind, src="bwd", out_bf16=out_bf16))
        print(f"tight forward {name} D={d} Dv={dv} {kind} out_bf16={out_bf16}: worst |err| / tight tolerance out {w_out:.3g}, lse {w_lse:.3g}; flagged {share:.3%}")
        assert ok, f"{name} D={d} Dv={dv} {kind} out_bf16={out_bf16}: the forward breaks the contract of mispmm_attn.h (out {w_out:.3g}, lse {w_lse:.3g} of the tight tolerance)"
        for grads_bf16 in (False, True):
            dq, dk, dvv = backward(name, q, k, v, out, lse, g, mask, grads_bf16=grads_bf16)
            case = Case(name, d, dv, kind, src="bwd", out_bf16=out_bf16, grads_bf16=grads_bf16)
            ok, worst = tight.tight_backward(dict(stored, dq=host(dq), dk=host(dk), dv=host(dvv)), case)
            print(f"tight backward {name} D={d} Dv={dv} {kind} out_bf16={out_bf16} grads_bf16={grads_bf16}: worst |err| / tight tolerance "
                  f"dq {worst[0]:.3g}, dk {worst[1]:.3g}, dv {worst[2]:.3g}; flagged P {worst[3]:.3%}, dS {worst[4]:.3%}")
            assert ok, f"{case.id}: the backward breaks the contract of mispmm_attn_bwd.h (dq, dk, dv {worst[:3]} of the tight tolerance)"


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["edges16", "edgesT32"])
def test_autograd_with_a_float32_grad_out_inside_the_tight_tolerance(name, out_dtype):
    """block_sparse_attention(fused=True, fused_backward=True) rounds a float32 grad_out to bf16 ONCE before the passes: the
    reference does the same and allows nothing for it."""
    out_bf16 = out_dtype == torch.bfloat16
    case = Case(name, 40, 72, "causal", src="bwd", out_bf16=out_bf16, grads_bf16=True, g32=True)
    qh, kh, vh, g32 = case.arrays
    q, k, v = (_bf(x).requires_grad_(True) for x in (qh, kh, vh))
    out = autograd.block_sparse_attention(trainable(name), q, k, v, mask=_dmask(case), out_dtype=out_dtype, fused=True, fused_backward=True)
    out.backward(_dev(case.g_bf16).to(torch.bfloat16) if out_bf16 else _dev(g32))      # a bf16 out takes a bf16 grad_out: already rounded
    o, lse = forward(name, dbits(qh), dbits(kh), dbits(vh), _dmask(case), out_bf16)
    stored = dict(out=host(o), lse=lse.cpu().numpy())
    assert np.array_equal(out.detach().float().cpu().numpy(), stored["out"])
    ok, (w_out, w_lse, share) = tight.tight_forward(stored, case)
    assert ok, (w_out, w_lse)
    got = dict(stored, dq=q.grad.float().cpu().numpy(), dk=k.grad.float().cpu().numpy(), dv=v.grad.float().cpu().numpy())
    ok, worst = tight.tight_backward(got, case)
    print(f"tight autograd {case.id}: worst dq {worst[0]:.3g}, dk {worst[1]:.3g}, dv {worst[2]:.3g}; flagged P {worst[3]:.3%}, dS {worst[4]:.3%}")
    assert ok, f"{case.id}: autograd's fused backward outside the tight tolerance {worst[:3]}"


@pytest.mark.parametrize("through_mask", [False, True])
@pytest.mark.parametrize("t", tight.TIES)
def test_tie_rows_bit_for_bit(t, through_mask):
    """t keys share a row's exact maximum, the rest lie 2^10 and more below: out, dq, dk, dv are exact numbers and lse = +0 at t = 1.
    No tolerance.  Relies on exp2(0) = 1 and on 1 / t being exact for a power of two."""
    for name in ref.PATTERNS:
        op = tight.tie_operands(name, t, through_mask)
        q, k, v, g = (dbits(op[n]) for n in ("q", "k", "v", "g"))
        mask = None if op["mask"] is None else _dev(op["mask"])
        for out_bf16 in (False, True):
            out, lse = forward(name, q, k, v, mask, out_bf16, scale=op["scale"])
            ok, wrong = tight.tie_forward(dict(out=host(out), lse=lse.cpu().numpy()), name, t, through_mask, out_bf16)
            assert ok, f"tie rows {name} t={t} through_mask={through_mask} out_bf16={out_bf16}: {wrong} elements of out / lse differ from the exact answer"
            for grads_bf16 in (False, True):
                dq, dk, dvv = backward(name, q, k, v, out, lse, g, mask, grads_bf16=grads_bf16, scale=op["scale"])
                ok, wrong = tight.tie_backward(dict(dq=host(dq), dk=host(dk), dv=host(dvv)), name, t, through_mask, grads_bf16)
                assert ok, f"tie rows {name} t={t} through_mask={through_mask} out_bf16={out_bf16} grads_bf16={grads_bf16}: {wrong} gradient elements differ"


def test_tie_rows_through_autograd_bit_for_bit():
    name, t = "edgesT16", 4
    for through_mask in (False, True):
        op = tight.tie_operands(name, t, through_mask)
        q, k, v = (_bf(op[n]).requires_grad_(True) for n in ("q", "k", "v"))
        mask = None if op["mask"] is None else _dev(op["mask"])
        out = autograd.block_sparse_attention(trainable(name), q, k, v, scale=op["scale"], mask=mask, fused=True, fused_backward=True)
        out.backward(_dev(op["g"]))
        want = tight.tie_expected(name, t, through_mask)
        assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), want["out"].astype(np.float32).view(np.uint32))
        got = dict(dq=q.grad.float().cpu().numpy(), dk=k.grad.float().cpu().numpy(), dv=v.grad.float().cpu().numpy())
        assert tight.tie_backward(got, name, t, through_mask, grads_bf16=True) == (True, 0)


@pytest.mark.parametrize("name,kind", [("ragged16", "none"), ("edges32", "leading")])
def test_wide_scores_stay_inside_the_composed_tolerances(name, kind):
    """|z| in the hundreds: exp of a difference against anything but the RUNNING maximum overflows (the fault `stale_max`)."""
    case = Case(name, 64, 64, kind, wide=16, scale=1.0)
    q, k, v, _ = (dbits(x) for x in case.arrays)
    for out_bf16 in (False, True):
        out, lse = ops.attention_bsr_bf16(ops.DeviceBSR.from_host(case.bsr), q, k, v, scale=1.0, mask=_dmask(case), out_bf16=out_bf16, return_lse=True)
        got = dict(out=host(out), lse=lse.cpu().numpy())
        c = Case(name, 64, 64, kind, wide=16, scale=1.0, out_bf16=out_bf16)
        for check in (checks.out_composed, checks.lse_bound, checks.forward_zero_rows):
            ok, worst = check(got, c)
            print(f"wide scores {c.id} {check.__name__}: {worst:.3g}")
            assert ok, f"{c.id}: {check.__name__} fails at {worst:.3g}"
