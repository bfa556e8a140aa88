"""SDDMM on a CSR pattern with X and Y in bf16 (sddmm_bf16.sddmm_csr_bf16 -> mispmm_sddmm_csr_bf16) against the fp32 kernel on the
same pattern and the same operand values, in the same process, in FAST and in REFERENCE.  Contenders:
  bf16          the new kernel, out in fp32 (what autograd.spmm_bf16(..., sddmm="bf16") launches for grad_values)
  f32_widened   ops.sddmm_csr on operands widened to fp32 BEFORE the clock starts: the kernel alone, twice the gather bytes
  today         what the default backward of autograd.spmm_bf16 does: ops.bf16_to_f32 of X and of Y, then ops.sddmm_csr -- three
                launches and an fp32 copy of both operands through memory
Shapes: n4c6-b13 x 128, GL7d25 x 64, ACTIVSg10K x 128, n4c6-b13 x 512.  Every contender is timed in interleaved rounds (device
events around a captured graph of `--loop` back-to-back calls), medians reported, after the new kernel's REFERENCE result has been
compared with the fp32 kernel's (whether the bits agree is recorded; both are held to the bound of mispmm.h) and its FAST result
to the header's bound.  floor: the index arrays, X once, the DISTINCT Y rows the pattern names x 2N bytes, and an fp32 out, once at
8 TB/s.  Each case runs in a child process of its own under `timeout`; after a case that fails nothing more is started.  Writes
one JSON (and prints it).  Nothing here asserts on a time, and nothing decides a dispatch.
  python tools/probe/sddmm_bf16_probe.py [--rounds 7] [--loop 20] [--seconds 120] [--out profiles/sddmm_bf16/probe.json]    GPU box only."""
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
CASES = [("n4c6-b13", 128), ("GL7d25", 64), ("ACTIVSg10K", 128), ("n4c6-b13", 512)]
ACCS = ("fast", "reference")


def one_case(name, n, rounds, loop):
    import numpy as np
    import torch
    from mispmm import capi, capi_sddmm_bf16, datasets, ops, sddmm_bf16
    from sddmm_probe import captured, timed

    csr = datasets.load_csr(name)
    a = ops.DeviceCSR.from_host(csr, plan=False)
    rng = np.random.default_rng(n)
    m, k, nnz = csr.num_rows, csr.num_cols, int(csr.nnz)
    x16 = torch.from_numpy(rng.uniform(-1, 1, (m, n)).astype(np.float32)).cuda().to(torch.bfloat16).view(torch.int16)
    y16 = torch.from_numpy(rng.uniform(-1, 1, (k, n)).astype(np.float32)).cuda().to(torch.bfloat16).view(torch.int16)
    x32, y32 = ops.bf16_to_f32(x16), ops.bf16_to_f32(y16)       # the same values, widened
    outs = {(key, acc): torch.empty(nnz, dtype=torch.float32, device="cuda") for key in ("bf16", "f32_widened", "today") for acc in ACCS}
    runs = {}
    for acc in ACCS:
        runs["bf16", acc] = lambda acc=acc: sddmm_bf16.sddmm_csr_bf16(a, x16, y16, out=outs["bf16", acc], acc=acc)
        runs["f32_widened", acc] = lambda acc=acc: ops.sddmm_csr(a, x32, y32, out=outs["f32_widened", acc], acc=acc)
        runs["today", acc] = lambda acc=acc: ops.sddmm_csr(a, ops.bf16_to_f32(x16), ops.bf16_to_f32(y16), out=outs["today", acc], acc=acc)
    tags = {}
    for (key, acc), fn in runs.items():
        fn()
        tags[f"{key}_{acc}"] = capi_sddmm_bf16.last_kernel() if key == "bf16" else capi.last_kernel()
    torch.cuda.synchronize()
    # sanity before timing (the parity tests are tests/test_gpu_sddmm_bf16.py)
    rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(csr.row_ptrs.astype(np.int64)))).cuda()
    cols = torch.from_numpy(csr.col_idxs.astype(np.int64)).cuda()
    scale, exact = torch.empty(nnz, dtype=torch.float64, device="cuda"), torch.empty(nnz, dtype=torch.float64, device="cuda")
    step = max(1, (1 << 24) // n)
    for s in range(0, nnz, step):
        p = x32[rows[s:s + step]].double() * y32[cols[s:s + step]].double()
        exact[s:s + step], scale[s:s + step] = p.sum(1), p.abs().sum(1)
    u = n * 2.0 ** -24
    worst_fast = float(((outs["bf16", "fast"].double() - exact).abs() / (u / (1 - u) * scale + 1e-300)).max())
    assert worst_fast <= 1.0, f"{name} N={n}: FAST outside the header's bound, {worst_fast} x"
    ref_same_bits = bool(torch.equal(outs["bf16", "reference"].view(torch.int32), outs["f32_widened", "reference"].view(torch.int32)))
    worst_ref = float(((outs["bf16", "reference"].double() - exact).abs() / (2.0 ** -24 * exact.abs() + n * 2.0 ** -52 * scale + 1e-300)).max())
    assert worst_ref <= 1.0, f"{name} N={n}: REFERENCE outside the fp32 kernel's bound, {worst_ref} x"
    assert bool(torch.equal(outs["today", "fast"].view(torch.int32), outs["f32_widened", "fast"].view(torch.int32)))
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
    floor_bytes = (m + 1) * 4 + nnz * 4 + m * n * 2 + distinct * n * 2 + nnz * 4
    floor_us = floor_bytes / HBM_BYTES_PER_US
    info = capi.device_info(0)
    out = {"matrix": name, "N": n, "rows": m, "cols": k, "nnz": nnz, "longest_row": int(np.diff(csr.row_ptrs.astype(np.int64)).max()),
           "distinct_y_rows": distinct, "kernels": tags, "floor_us": round(floor_us, 2), "reference_same_bits_as_f32_kernel": ref_same_bits,
           "fast_worst_error_over_bound": worst_fast, "device": info["name"], "cus": info["cu_count"]}
    for acc in ACCS:
        for key in ("bf16", "f32_widened", "today"):
            out[f"{key}_{acc}_us"] = round(med[key, acc], 2)
            out[f"{key}_{acc}_best_us"] = round(min(times[key, acc]), 2)
        out[f"bf16_{acc}_x_floor"] = round(med["bf16", acc] / floor_us, 2)
        out[f"f32_widened_over_bf16_{acc}"] = round(med["f32_widened", acc] / med["bf16", acc], 2)
        out[f"today_over_bf16_{acc}"] = round(med["today", acc] / med["bf16", acc], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loop", type=int, default=20)
    ap.add_argument("--seconds", type=int, default=120, help="time limit of one case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm_bf16", "probe.json"))
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
    result = json.dumps({"probe": "sddmm_bf16", "rounds": a.rounds, "loop": a.loop,
                         "timing": "median of interleaved rounds of a captured graph of `loop` calls; floor = row pointers, column indices, "
                                   "X once, the distinct Y rows x 2N bytes and an fp32 out once at 8 TB/s",
                         "status": status, "cases": cases})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(result + "\n")
    print(result)
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
