"""A check of the fused CSR attention backward that is DERIVED from the words of include/mispmm_attn_csr_bwd.h and not measured,
built as tests/_attn_csr_tight.py is.  Functions of (got, case): the CPU harness and the GPU tests call the same code.

WHY IT CAN BE TIGHT.  `bwd_tolerances` (_attn_csr_bwd_ref) allows for the errors of the forward: of z, of the stored lse and of
the stored out.  This check takes the kernel's OWN stored out and lse, so none of those is an error of the backward, and the
cases' operands make every z exact: q and k are multiples of 2^-8 with sum |q||k| < 2^8 and the scale is a power of two
(`exact_scores` of tests/_attn_csr_tight.py, asserted here), so z = fma(scale, s, bias) is one rounding of an exact number and
its bits are determined, and with them t = fl32(z - lse), the argument of the exponential.
THE REFERENCE is a float64 evaluation of the header's formulas on those inputs: P = exp(t), dP = <g, v>, delta = <g, out>,
dS = scale P (dP - delta), and the three sums.
WHAT A KERNEL THAT KEEPS THE WORDS MAY DIFFER BY, and nothing else (u = 2^-24, u' = 2^-23, g_n = n u' / (1 - n u')):
  (a) the exponential: v_exp_f32 of fl(t fl(log2 e)) against exp(t): relative (3 |t| + 2) u, and a flushed subnormal, 2^-126;
      the one rounding of z - lse is in t itself and costs nothing more;
  (b) the order of the fp32 sums over Dv: dP within g_Dv sum |g||v|, delta within g_Dv sum |g||o|;
  (c) the three named roundings of dS: 3 u P |dP - delta|;
  (d) the order of the fp32 sums over the entries: g_L on sum |terms|, L the entries of the row or column.
    E_P = P expm1((3 |t| + 2) u) + 2^-126                       E_x = g_Dv (sum |g||v| + sum |g||o|) + 2 Dv 2^-126
    E_dS = |scale| (E_P (|x| + E_x) + P E_x + 3 u P |x|) + 3 2^-126,    x = dP - delta
    |dq - ref| <= 1.01 (sum_row E_dS |k| + g_L sum_row |dS||k| + L 2^-126), dk and dv alike over the column (dv with E_P, P, |g|).
No constant comes from running a kernel.  There are no flagged elements: the cases keep every non-empty row's lse finite
(`masked` leaves each row's last entry finite), so the reference covers every element; `coverage` returns that share."""
import numpy as np

import _attn_csr_bwd_ref as bref
import _attn_csr_tight as tight


def reference(case, out, lse):
    """((dq, dk, dv), (tolerances)) in float64 around a forward's stored out [H, M, Dv] and lse [H, M]."""
    op, csr = bref.operands(case), bref.matrix(case.name)
    assert tight.exact_scores(csr, op["q"], op["k"], op["scale"], op["bias"]), "the scores are not exact in fp32 -- use narrower operands"
    with np.errstate(invalid="ignore"):
        lse64 = np.where(np.isneginf(lse), 0.0, lse.astype(np.float64))          # an empty row: no entry reads it
    return bref.propagate(csr, op["q"], op["k"], op["v"], op["g"], op["scale"], op["bias"], out.astype(np.float64), lse64, None, None, None, 2.0,
                          tight.gamma)


def coverage(case, out, lse):
    """The share of the elements of dq, dk, dv whose reference and tolerance are finite numbers: what the check covers."""
    want, tols = reference(case, out, lse)
    good = sum(int((np.isfinite(w) & np.isfinite(t)).sum()) for w, t in zip(want, tols))
    return good / sum(w.size for w in want)


def tight_backward(got, case):
    """dq, dk, dv of `case` against the derived reference around got["out"], got["lse"]: (ok, worst |err| / tolerance per output)."""
    want, tols = reference(case, got["out"], got["lse"])
    res = [tight._worst(got[n], w, t) for n, w, t in zip(("dq", "dk", "dv"), want, tols)]
    return all(ok for ok, _ in res), tuple(worst for _, worst in res)
