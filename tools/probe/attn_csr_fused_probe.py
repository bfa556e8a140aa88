"""Fused CSR attention forward (ops.attention_csr: one launch for all heads) against the four-launch chain it replaces (a torch
multiply for the scale, ops.sddmm_csr, ops.softmax_csr, ops.spmm_csr in FAST arithmetic, once per head: what
autograd.sparse_attention(acc="fast") enqueues), in the same process on the same operands.  Shapes: n4c6-b13 and GL7d25 at
D = Dv = 64 and 128 with 1 and 8 heads, no bias.  Both candidates are timed in interleaved rounds (device events around a
captured graph of `--loop` back-to-back forwards), medians reported, after the fused result has been compared with the chain's.
floor: Q, K, V, out, lse and the index arrays once at 8 TB/s (there is no bias here).  Each case runs in a child process of its
own under `timeout`; after a case that fails nothing more is started.  Prints one JSON line.
  python tools/probe/attn_csr_fused_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
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
    from mispmm import capi, capi_attn_csr, datasets, ops
    from sddmm_probe import captured, timed

    csr = datasets.load_csr(name)
    a = ops.DeviceCSR.from_host(csr, plan=False)
    rng = np.random.default_rng(d + heads)
    f32 = lambda shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda()   # noqa: E731
    q, k, v = f32((heads, csr.num_rows, d)), f32((heads, csr.num_cols, d)), f32((heads, csr.num_cols, d))
    scale = d ** -0.5
    fused_out = torch.empty((heads, csr.num_rows, d), device="cuda")
    lse = torch.empty((heads, csr.num_rows), device="cuda")
    qs = torch.empty((csr.num_rows, d), device="cuda")
    s, p = torch.empty(csr.nnz, device="cuda"), torch.empty(csr.nnz, device="cuda")
    chain_out = torch.empty((heads, csr.num_rows, d), device="cuda")

    def fused():
        ops.attention_csr(a, q, k, v, scale=scale, out=fused_out, lse=lse)

    def chain():
        for h in range(heads):
            torch.mul(q[h], scale, out=qs)
            ops.sddmm_csr(a, qs, k[h], out=s, acc="fast")
            ops.softmax_csr(a, s, out=p, acc="fast")
            ops.spmm_csr(dataclasses.replace(a, data=p), v[h], out=chain_out[h], acc="fast")

    fused()
    tag = capi_attn_csr.last_kernel()
    chain()
    torch.cuda.synchronize()
    apart = float((fused_out - chain_out).abs().max())
    assert not bool(torch.isnan(fused_out).any()) and apart <= 2.0 ** -14, f"fused and chain differ by {apart}"   # |out| <= 1, fp32 throughout
    graphs = {"fused": captured(fused, loop), "chain": captured(chain, loop)}
    for _ in range(2):
        for g in graphs.values():
            timed(g, loop)
    times = {key: [] for key in graphs}
    for _ in range(rounds):
        for key, g in graphs.items():
            times[key].append(timed(g, loop))
    med = {key: statistics.median(t) for key, t in times.items()}
    floor_bytes = heads * (2 * csr.num_rows * d + 2 * csr.num_cols * d + csr.num_rows) * 4 + (csr.nnz + csr.num_rows + 1) * 4
    floor_us = floor_bytes / HBM_BYTES_PER_US
    counts = np.diff(csr.row_ptrs.astype(np.int64))
    info = capi.device_info(0)
    return {"matrix": name, "rows": csr.num_rows, "cols": csr.num_cols, "nnz": csr.nnz, "D": d, "Dv": d, "heads": heads, "kernel": tag,
            "fused_us": round(med["fused"], 2), "fused_best_us": round(min(times["fused"]), 2), "chain_us": round(med["chain"], 2),
            "chain_us_per_head": round(med["chain"] / heads, 2), "chain_over_fused": round(med["chain"] / med["fused"], 2),
            "floor_us": round(floor_us, 2), "fused_x_floor": round(med["fused"] / floor_us, 2), "max_abs_difference": apart,
            "mean_row": round(float(counts.mean()), 1), "longest_row": int(counts.max()), "device": info["name"], "cus": info["cu_count"]}


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
    print(json.dumps({"probe": "attn_csr_fused", "rounds": a.rounds, "loop": a.loop,
                      "timing": "median of interleaved rounds of a captured graph of `loop` forwards; chain = torch multiply, sddmm_csr, "
                                "softmax_csr, spmm_csr (FAST) once per head; floor = Q, K, V, out, lse and the index arrays once at 8 TB/s",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
