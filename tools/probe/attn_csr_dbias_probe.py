"""The bias gradient of the fused CSR attention (attn_csr_dbias.attention_csr_dbias / attention_csr_dbias_bf16: one launch for all
heads) against what stands beside it, in the same process on the same operands.  Candidates:
  dbias     the new call
  backward  ops.attention_csr_bwd (fp32) or attn_csr_bf16.attention_csr_bf16_bwd (bf16, bf16 gradients) alone: dq, dk and dv in
            two launches -- what a training step pays anyway
  hand      what a user who trains the bias writes today, per head, at the ops level in FAST arithmetic: the backward of
            spmm(a, edge_softmax(a, sddmm(a, q * scale, k) + bias), v) as far as the bias -- torch.mul, ops.sddmm_csr, a torch add,
            ops.softmax_csr, ops.sddmm_csr, ops.softmax_csr_bwd, then torch.stack (fp32 only: bf16 operands are widened BEFOREHAND,
            not timed)
Shapes: n4c6-b13 and GL7d25 at D = Dv = 64 with 1 and 8 heads, fp32 and bf16, a bias per head; out and lse are the matching
fused forward's.  All candidates are timed in interleaved rounds (device events around a captured graph of `--loop` back-to-back
calls), medians reported, after the new call has been compared with the hand composition (inside 2^-12 of the largest entry).
floor: the index arrays, the DISTINCT K and V rows the pattern names, the Q, grad_out and out rows of rows with entries, lse, bias
and dBias, each once at 8 TB/s.  Each case runs in a child process of its own under `timeout`; after a case that fails nothing
more is started.  Prints one JSON line.  Nothing asserts on a time and no dispatcher takes a rule from the figures.
  python tools/probe/attn_csr_dbias_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_BYTES_PER_US = 8e6     # 8 TB/s
CASES = [(name, 64, heads, elem) for name in ("n4c6-b13", "GL7d25") for heads in (1, 8) for elem in ("f32", "bf16")]


def one_case(name, d, heads, elem, rounds, loop):
    import numpy as np
    import torch
    from mispmm import attn_csr_bf16, attn_csr_dbias, autograd, capi, capi_attn_csr_dbias, datasets, ops
    from sddmm_probe import captured, timed

    csr = datasets.load_csr(name)
    t = autograd.TrainableCSR.from_host(csr)
    a, at, perm = t.fwd, t.tpattern, t.perm32()
    rng = np.random.default_rng(d + heads)
    m, kk, nnz = csr.num_rows, csr.num_cols, csr.nnz
    bits = lambda shape: ops.f32_to_bf16(torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda())   # noqa: E731
    q, k, v, g = bits((heads, m, d)), bits((heads, kk, d)), bits((heads, kk, d)), bits((heads, m, d))
    qf, kf, vf, gf = (ops.bf16_to_f32(x) for x in (q, k, v, g))           # the same values for both element types
    bias = torch.from_numpy(rng.uniform(-2, 2, (heads, nnz)).astype(np.float32)).cuda()
    scale = d ** -0.5
    bf16 = elem == "bf16"
    if bf16:
        out, lse = attn_csr_bf16.attention_csr_bf16(a, q, k, v, scale=scale, bias=bias, return_lse=True)
    else:
        out, lse = ops.attention_csr(a, qf, kf, vf, scale=scale, bias=bias, return_lse=True)
    delta = torch.empty((heads, m), device="cuda")
    res_b = torch.empty((heads, nnz), device="cuda")
    shapes = ((heads, m, d), (heads, kk, d), (heads, kk, d))
    grads = [torch.empty(s, dtype=torch.int16 if bf16 else torch.float32, device="cuda") for s in shapes]

    def dbias():
        if bf16:
            attn_csr_dbias.attention_csr_dbias_bf16(a, q, k, v, out, lse, g, scale, bias, dbias=res_b)
        else:
            attn_csr_dbias.attention_csr_dbias(a, qf, kf, vf, out, lse, gf, scale, bias, dbias=res_b)

    def backward():
        if bf16:
            attn_csr_bf16.attention_csr_bf16_bwd(a, at, perm, q, k, v, out, lse, g, scale=scale, bias=bias, grads_bf16=True, dq=grads[0], dk=grads[1],
                                                 dv=grads[2], delta=delta)
        else:
            ops.attention_csr_bwd(a, at, perm, qf, kf, vf, out, lse, gf, scale=scale, bias=bias, dq=grads[0], dk=grads[1], dv=grads[2], delta=delta)

    def hand():
        per_head = []
        for h in range(heads):
            s = ops.sddmm_csr(a, qf[h] * scale, kf[h], acc="fast")
            p = ops.softmax_csr(a, s + bias[h], acc="fast")
            dp = ops.sddmm_csr(a, gf[h], vf[h], acc="fast")
            per_head.append(ops.softmax_csr_bwd(a, p, dp, acc="fast"))
        return torch.stack(per_head)

    dbias()
    tag = capi_attn_csr_dbias.last_kernel()
    want = hand()
    torch.cuda.synchronize()
    apart = float((res_b - want).abs().max() / want.abs().max())
    assert not bool(torch.isnan(res_b).any()) and apart <= 2.0 ** -12, f"new call and hand composition differ by {apart} of the largest entry"
    graphs = {key: captured(f, loop) for key, f in (("dbias", dbias), ("backward", backward), ("hand", hand))}
    for _ in range(2):
        for gr in graphs.values():
            timed(gr, loop)
    times = {key: [] for key in graphs}
    for _ in range(rounds):
        for key, gr in graphs.items():
            timed_us = timed(gr, loop)
            times[key].append(timed_us)
    med = {key: statistics.median(x) for key, x in times.items()}
    counts = np.diff(csr.row_ptrs.astype(np.int64))
    named = int(np.unique(csr.col_idxs).size)
    rows = int((counts > 0).sum())
    eb = 2 if bf16 else 4
    # K and V rows named, Q and grad_out rows of rows with entries at the element size; out rows at 4; lse, bias, dBias; indices
    floor_bytes = heads * (2 * named * d * eb + 2 * rows * d * eb + rows * d * 4 + rows * 4 + 2 * nnz * 4) + (nnz + m + 1) * 4
    floor_us = floor_bytes / HBM_BYTES_PER_US
    info = capi.device_info(0)
    res = {"matrix": name, "rows": m, "cols": kk, "nnz": nnz, "D": d, "Dv": d, "heads": heads, "elem": elem, "kernel": tag}
    for key in graphs:
        res[key + "_us"] = round(med[key], 2)
        res[key + "_best_us"] = round(min(times[key]), 2)
    res.update({"dbias_over_backward": round(med["dbias"] / med["backward"], 3), "hand_over_dbias": round(med["hand"] / med["dbias"], 2),
                "floor_us": round(floor_us, 2), "dbias_x_floor": round(med["dbias"] / floor_us, 2), "max_rel_difference_to_hand": apart,
                "distinct_columns": named, "mean_row": round(float(counts.mean()), 1), "longest_row": int(counts.max()),
                "device": info["name"], "cus": info["cu_count"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loop", type=int, default=20)
    ap.add_argument("--seconds", type=int, default=120, help="time limit of one case")
    ap.add_argument("--case", type=int, help="internal: index into CASES, run in this process")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(one_case(*CASES[a.case], a.rounds, a.loop)))
        return 0
    cases, status = [], "ok"
    for i, case in enumerate(CASES):
        cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--case", str(i),
               "--rounds", str(a.rounds), "--loop", str(a.loop)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
            status = f"case {case} ended with status {r.returncode}: {r.stderr.strip().splitlines()[-1:] or ''}"
            break
        cases.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"probe": "attn_csr_dbias", "rounds": a.rounds, "loop": a.loop,
                      "timing": "median of interleaved rounds of a captured graph of `loop` calls; backward = dq, dk, dv by the fused backward of the "
                                "element type alone; hand = per head torch.mul, ops.sddmm_csr, a torch add, ops.softmax_csr, ops.sddmm_csr, "
                                "ops.softmax_csr_bwd in fp32 FAST, then torch.stack; floor = index arrays, distinct K and V rows, Q, grad_out and out "
                                "rows, lse, bias and dBias once at 8 TB/s",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
