"""The row-list product with B in bf16 (ops.spmm_csr_bf16 -> mispmm_rows_bf16, acc="fast") against the fp32 product on the same A
and the same B values, in the same process.  Contenders:
  bf16_out / f32_out   the new kernel, C in bf16 and in fp32
  f32_hint / f32_plain ops.spmm_csr(acc="fast") on B widened to fp32, with and without use_hint (the uniform-row wave, the span
                       list of the long-row matrices; the plan order is not uploaded)
  widen_today          what a user who holds bf16 activations does without the new kernel: ops.bf16_to_f32 of B, the fp32
                       product with its hints, ops.f32_to_bf16 of C -- three launches
Shapes: n4c6-b13 x {64, 128, 512}, GL7d25 x 64, ACTIVSg10K x 128.  Every contender is timed in interleaved rounds (device events
around a captured graph of `--loop` back-to-back calls), medians reported, after the new kernel's fp32 C has been compared bit
for bit with the fp32 kernel's on the uniform matrix (the same fma chain) and to a bound elsewhere.  floor: the index and value
arrays, the DISTINCT B rows the matrix names x 2N bytes, and a bf16 C, once at 8 TB/s.  Each case runs in a child process of its
own under `timeout`; after a case that fails nothing more is started.  Prints one JSON line.  Nothing here decides a dispatch.
  python tools/probe/spmm_bf16_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
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
CASES = [("n4c6-b13", 64), ("n4c6-b13", 128), ("n4c6-b13", 512), ("GL7d25", 64), ("ACTIVSg10K", 128)]


def one_case(name, n, rounds, loop):
    import numpy as np
    import torch
    from mispmm import capi, capi_bf16, datasets, ops
    from sddmm_probe import captured, timed

    csr = datasets.load_csr(name)
    a = ops.DeviceCSR.from_host(csr, plan=False)
    rng = np.random.default_rng(n)
    b32 = torch.from_numpy(rng.uniform(-1, 1, (csr.num_cols, n)).astype(np.float32)).cuda().to(torch.bfloat16)
    b16 = b32.view(torch.int16)
    b32 = b32.float()                                   # the same values, widened
    m = csr.num_rows
    c16 = torch.empty((m, n), dtype=torch.int16, device="cuda")
    c32, c_hint, c_plain, c_today = (torch.empty((m, n), dtype=torch.float32, device="cuda") for _ in range(4))

    def widen_today():
        ops.spmm_csr(a, ops.bf16_to_f32(b16), out=c_today, acc="fast")
        return ops.f32_to_bf16(c_today)

    runs = {"bf16_out": lambda: ops.spmm_csr_bf16(a, b16, out_bf16=True, out=c16, acc="fast"),
            "f32_out": lambda: ops.spmm_csr_bf16(a, b16, out=c32, acc="fast"),
            "f32_hint": lambda: ops.spmm_csr(a, b32, out=c_hint, acc="fast"),
            "f32_plain": lambda: ops.spmm_csr(a, b32, out=c_plain, acc="fast", use_hint=False),
            "widen_today": widen_today}
    tags = {}
    for key, fn in runs.items():
        fn()
        tags[key] = capi_bf16.last_kernel() if key in ("bf16_out", "f32_out") else capi.last_kernel()
    torch.cuda.synchronize()
    # sanity before timing (the parity tests are tests/test_gpu_spmm_bf16.py): one fma chain per element in the new kernel;
    # the fp32 kernels promise that chain on the uniform matrix and a fixed order elsewhere
    scale = torch.zeros((m, n), dtype=torch.float64, device="cuda")
    rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(csr.row_ptrs.astype(np.int64)))).cuda()
    scale.index_add_(0, rows, a.data.double().abs()[:, None] * b32.double().abs()[torch.from_numpy(csr.col_idxs.astype(np.int64)).cuda()])
    longest = int(np.diff(csr.row_ptrs.astype(np.int64)).max())
    apart = float(((c32.double() - c_plain.double()).abs() / (scale + 1e-300)).max())
    assert apart <= 2 * longest * 2.0 ** -24, f"{name} N={n}: new kernel and fp32 kernel differ by {apart} of sum|a||b|"
    same_bits = bool(torch.equal(c32.view(torch.int32), c_plain.view(torch.int32)))
    assert bool(torch.equal(c16, ops.f32_to_bf16(c32)))
    graphs = {key: captured(fn, loop) for key, fn in runs.items()}
    for _ in range(2):
        for g in graphs.values():
            timed(g, loop)
    times = {key: [] for key in graphs}
    for _ in range(rounds):
        for key, g in graphs.items():
            times[key].append(timed(g, loop))
    med = {key: statistics.median(t) for key, t in times.items()}
    distinct = int(np.unique(csr.col_idxs).shape[0])
    floor_bytes = (m + 1) * 4 + csr.nnz * 8 + distinct * n * 2 + m * n * 2
    floor_us = floor_bytes / HBM_BYTES_PER_US
    info = capi.device_info(0)
    out = {"matrix": name, "N": n, "rows": m, "cols": csr.num_cols, "nnz": int(csr.nnz), "longest_row": longest, "distinct_b_rows": distinct,
           "kernels": tags, "floor_us": round(floor_us, 2), "same_bits_as_f32_plain": same_bits, "max_difference_over_sum_abs": apart,
           "bf16_out_x_floor": round(med["bf16_out"] / floor_us, 2), "f32_hint_over_bf16_out": round(med["f32_hint"] / med["bf16_out"], 2),
           "widen_today_over_bf16_out": round(med["widen_today"] / med["bf16_out"], 2), "device": info["name"], "cus": info["cu_count"]}
    for key in runs:
        out[key + "_us"] = round(med[key], 2)
        out[key + "_best_us"] = round(min(times[key]), 2)
    return out


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
    print(json.dumps({"probe": "spmm_bf16", "rounds": a.rounds, "loop": a.loop, "acc": "fast",
                      "timing": "median of interleaved rounds of a captured graph of `loop` calls; floor = row pointers, column indices, "
                                "values, the distinct B rows x 2N bytes and a bf16 C once at 8 TB/s",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
