"""Fused CSR attention backward (ops.attention_csr_bwd: at most two launches for all heads) against the backward it stands beside
(what autograd.sparse_attention(fused=True) without fused_backward enqueues, at the ops level, once per head: a torch multiply
for the scale, ops.sddmm_csr and ops.softmax_csr to recompute P, a p[perm] gather and ops.spmm_csr on A^T for dV, ops.sddmm_csr
for dP, ops.softmax_csr_bwd, ops.spmm_csr and a torch multiply for dQ, a ds[perm] gather and ops.spmm_csr on A^T for dK, and a
torch.stack of the heads), in the same process on the same operands.  Shapes: n4c6-b13 and GL7d25 at D = Dv = 64 and 128 with 1
and 8 heads, no bias.  Both candidates are timed in interleaved rounds (device events around a captured graph of `--loop`
back-to-back backwards), medians reported, after the fused gradients have been compared with the chain's.
floor: Q, K, V, dO, out, lse, dQ, dK, dV, delta, both index sets and perm once each at 8 TB/s (there is no bias here).  Each case
runs in a child process of its own under `timeout`; after a case that fails nothing more is started.  Prints one JSON line.
  python tools/probe/attn_csr_fused_bwd_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
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
CASES = [(name, d, heads) for name in ("n4c6-b13", "GL7d25") for d in (64, 128) for heads in (1, 8)]


def one_case(name, d, heads, rounds, loop):
    import dataclasses

    import numpy as np
    import torch
    from mispmm import autograd, capi, capi_attn_csr_bwd, datasets, ops
    from sddmm_probe import captured, timed

    csr = datasets.load_csr(name)
    t = autograd.TrainableCSR.from_host(csr)
    a, at, perm, perm32 = t.fwd, t.tpattern, t.perm, t.perm32()
    rng = np.random.default_rng(d + heads)
    f32 = lambda shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda()   # noqa: E731
    q, k, v, g = f32((heads, csr.num_rows, d)), f32((heads, csr.num_cols, d)), f32((heads, csr.num_cols, d)), f32((heads, csr.num_rows, d))
    scale = d ** -0.5
    out, lse = ops.attention_csr(a, q, k, v, scale=scale, return_lse=True)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty_like(lse)
    kept = {}

    def fused():
        ops.attention_csr_bwd(a, at, perm32, q, k, v, out, lse, g, scale=scale, dq=dq, dk=dk, dv=dv, delta=delta)

    def chain():
        grads = ([], [], [])
        for h in range(heads):
            qs = q[h] * scale
            s = ops.sddmm_csr(a, qs, k[h], acc="fast")
            p = ops.softmax_csr(a, s, acc="fast")
            grads[2].append(ops.spmm_csr(dataclasses.replace(at, data=p[perm]), g[h], acc="fast"))
            dp = ops.sddmm_csr(a, g[h], v[h], acc="fast")
            ds = ops.softmax_csr_bwd(a, p, dp, acc="fast")
            grads[0].append(ops.spmm_csr(dataclasses.replace(a, data=ds), k[h], acc="fast") * scale)
            grads[1].append(ops.spmm_csr(dataclasses.replace(at, data=ds[perm]), qs, acc="fast"))
        kept["chain"] = [torch.stack(x) for x in grads]

    fused()
    tag = capi_attn_csr_bwd.last_kernel()
    chain()
    torch.cuda.synchronize()
    apart = max(float((x - y).abs().max()) for x, y in zip((dq, dk, dv), kept["chain"]))
    size = max(float(x.abs().max()) for x in kept["chain"])
    assert not any(bool(torch.isnan(x).any()) for x in (dq, dk, dv)) and apart <= 2.0 ** -12 * max(size, 1.0), f"fused and chain differ by {apart}"
    graphs = {"fused": captured(fused, loop), "chain": captured(chain, loop)}
    for _ in range(2):
        for gr in graphs.values():
            timed(gr, loop)
    times = {key: [] for key in graphs}
    for _ in range(rounds):
        for key, gr in graphs.items():
            times[key].append(timed(gr, loop))
    med = {key: statistics.median(x) for key, x in times.items()}
    m, kk = csr.num_rows, csr.num_cols
    floor_bytes = heads * (3 * m * d + 2 * kk * d + 2 * m + m * d + 2 * kk * d) * 4 + (3 * csr.nnz + m + 1 + kk + 1) * 4
    floor_us = floor_bytes / HBM_BYTES_PER_US
    counts, col_counts = np.diff(csr.row_ptrs.astype(np.int64)), np.bincount(csr.col_idxs.astype(np.int64), minlength=kk)
    info = capi.device_info(0)
    return {"matrix": name, "rows": m, "cols": kk, "nnz": csr.nnz, "D": d, "Dv": d, "heads": heads, "kernel": tag,
            "fused_us": round(med["fused"], 2), "fused_best_us": round(min(times["fused"]), 2), "chain_us": round(med["chain"], 2),
            "chain_us_per_head": round(med["chain"] / heads, 2), "chain_over_fused": round(med["chain"] / med["fused"], 2),
            "floor_us": round(floor_us, 2), "fused_x_floor": round(med["fused"] / floor_us, 2), "max_abs_difference": apart,
            "largest_gradient": size, "longest_row": int(counts.max()), "longest_column": int(col_counts.max()), "device": info["name"],
            "cus": info["cu_count"]}


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
    print(json.dumps({"probe": "attn_csr_fused_bwd", "rounds": a.rounds, "loop": a.loop,
                      "timing": "median of interleaved rounds of a captured graph of `loop` backwards; chain = the per-head backward of "
                                "sparse_attention(fused=True) at the ops level (FAST); floor = Q, K, V, dO, out, lse, dQ, dK, dV, delta, both "
                                "index sets and perm once at 8 TB/s",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
