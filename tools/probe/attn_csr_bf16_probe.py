"""Fused CSR attention on bf16 q, k, v (attn_csr_bf16.attention_csr_bf16: one launch for all heads) against what a holder of bf16
operands had before it, in the same process on the same operands.  Candidates:
  bf16_out   the new launch, bf16 out
  f32_out    the new launch, fp32 out
  f32_kernel ops.attention_csr on operands widened BEFOREHAND (the widening is not timed): the fp32 kernel on twice the K / V bytes
  today      ops.bf16_to_f32 of q, k and v, ops.attention_csr, ops.f32_to_bf16 of out: five launches and fp32 copies of everything
Shapes: n4c6-b13 and ACTIVSg10K at D = Dv = 64 and 128 with 1 and 8 heads, no bias, lse written.  All candidates are timed in
interleaved rounds (device events around a captured graph of `--loop` back-to-back forwards), medians reported, after the new
launch has been compared with the fp32 kernel bit for bit where that is the contract (it is not here: these scores round) and
inside 2^-14 otherwise.  floor: the index arrays, the DISTINCT K and V rows the pattern names at 2 bytes an element, Q, out
(bf16) and lse once at 8 TB/s.  Each case runs in a child process of its own under `timeout`; after a case that fails nothing
more is started.  Prints one JSON line.  Nothing asserts on a time and no dispatcher takes a rule from the figures.
  python tools/probe/attn_csr_bf16_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
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
CASES = [(name, d, heads) for name in ("n4c6-b13", "ACTIVSg10K") for d in (64, 128) for heads in (1, 8)]


def one_case(name, d, heads, rounds, loop):
    import numpy as np
    import torch
    from mispmm import capi, capi_attn_csr, capi_attn_csr_bf16, datasets, ops
    from mispmm.attn_csr_bf16 import attention_csr_bf16
    from sddmm_probe import captured, timed

    csr = datasets.load_csr(name)
    a = ops.DeviceCSR.from_host(csr, plan=False)
    rng = np.random.default_rng(d + heads)
    bits = lambda shape: ops.f32_to_bf16(torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda())   # noqa: E731
    q, k, v = bits((heads, csr.num_rows, d)), bits((heads, csr.num_cols, d)), bits((heads, csr.num_cols, d))
    qf, kf, vf = (ops.bf16_to_f32(x) for x in (q, k, v))
    scale = d ** -0.5
    shape = (heads, csr.num_rows, d)
    out16, out32 = torch.empty(shape, dtype=torch.int16, device="cuda"), torch.empty(shape, device="cuda")
    ref32 = torch.empty(shape, device="cuda")
    lse = torch.empty((heads, csr.num_rows), device="cuda")

    def bf16_out():
        attention_csr_bf16(a, q, k, v, scale=scale, out_bf16=True, out=out16, lse=lse)

    def f32_out():
        attention_csr_bf16(a, q, k, v, scale=scale, out=out32, lse=lse)

    def f32_kernel():
        ops.attention_csr(a, qf, kf, vf, scale=scale, out=ref32, lse=lse)

    def today():
        ops.f32_to_bf16(ops.attention_csr(a, ops.bf16_to_f32(q), ops.bf16_to_f32(k), ops.bf16_to_f32(v), scale=scale, lse=lse))

    bf16_out()
    tag = capi_attn_csr_bf16.last_kernel()
    f32_out()
    f32_kernel()
    f32_tag = capi_attn_csr.last_kernel()
    torch.cuda.synchronize()
    apart = float((out32 - ref32).abs().max())
    rounded = bool(torch.equal(ops.f32_to_bf16(out32), out16))
    assert not bool(torch.isnan(out32).any()) and apart <= 2.0 ** -14 and rounded, f"new and fp32 kernel differ by {apart}; bf16 out rounded once: {rounded}"
    graphs = {key: captured(f, loop) for key, f in (("bf16_out", bf16_out), ("f32_out", f32_out), ("f32_kernel", f32_kernel), ("today", today))}
    for _ in range(2):
        for g in graphs.values():
            timed(g, loop)
    times = {key: [] for key in graphs}
    for _ in range(rounds):
        for key, g in graphs.items():
            times[key].append(timed(g, loop))
    med = {key: statistics.median(t) for key, t in times.items()}
    named = int(np.unique(csr.col_idxs).size)
    floor_bytes = heads * (2 * csr.num_rows * d * 2 + 2 * named * d * 2 + csr.num_rows * 4) + (csr.nnz + csr.num_rows + 1) * 4
    floor_us = floor_bytes / HBM_BYTES_PER_US
    counts = np.diff(csr.row_ptrs.astype(np.int64))
    info = capi.device_info(0)
    res = {"matrix": name, "rows": csr.num_rows, "cols": csr.num_cols, "nnz": csr.nnz, "named_cols": named, "D": d, "Dv": d, "heads": heads,
           "kernel": tag, "f32_kernel": f32_tag}
    for key in graphs:
        res[key + "_us"] = round(med[key], 2)
        res[key + "_best_us"] = round(min(times[key]), 2)
    res.update({"f32_kernel_over_bf16_out": round(med["f32_kernel"] / med["bf16_out"], 3), "today_over_bf16_out": round(med["today"] / med["bf16_out"], 2),
                "floor_us": round(floor_us, 2), "bf16_out_x_floor": round(med["bf16_out"] / floor_us, 2), "max_abs_difference_to_f32_kernel": apart,
                "mean_row": round(float(counts.mean()), 1), "longest_row": int(counts.max()), "device": info["name"], "cus": info["cu_count"]})
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
    print(json.dumps({"probe": "attn_csr_bf16", "rounds": a.rounds, "loop": a.loop,
                      "timing": "median of interleaved rounds of a captured graph of `loop` forwards; f32_kernel = ops.attention_csr on operands "
                                "widened beforehand; today = three bf16_to_f32, ops.attention_csr, f32_to_bf16; floor = index arrays, the distinct "
                                "K and V rows at 2 bytes, Q, a bf16 out and lse once at 8 TB/s",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
