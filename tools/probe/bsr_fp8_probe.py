"""The fp8 e4m3 block-sparse product (bsr_fp8.spmm_bsr_fp8, one launch) against the bf16 one (ops.spmm_bsr_bf16) on the same
pattern and the exactly widened operands, against widening both operands first (two torch casts, then the bf16 product: what a
user with fp8 data did before), and against the byte floor, in the same process, fp32 C, no scales.
Shapes: the patterns of tools/probe/attn_fused_probe.py -- ACTIVSg10K at 16 x 16 with N = 128; the banded 32 x 32 pattern
(8192 rows, 8 blocks per block row) with N = 128 and 512.  All candidates are timed in interleaved rounds (device events around
a captured graph of `--loop` back-to-back products), medians reported, after the fp8 result has been compared with the bf16
one.  floor_us: A's blocks, B once, C and the index arrays over 8 TB/s, for either element size.  Each case runs in a child
process of its own under `timeout`; after a case that fails nothing more is started.  Prints one JSON line.
  python tools/probe/bsr_fp8_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = [("ACTIVSg10K", 128), ("banded", 128), ("banded", 512)]
HBM_BYTES_PER_US = 8e6


def one_case(name, n, rounds, loop):
    import numpy as np
    import torch
    from mispmm import bsr_fp8, capi, capi_bsr_fp8, ops
    from attn_fused_probe import pattern
    from sddmm_probe import captured, timed

    rows, cols, bs, ptrs, idxs, _ = pattern(name)
    u32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).cuda()   # noqa: E731
    a = ops.DeviceBSR(rows, cols, bs, bs, int(idxs.shape[0]), u32(ptrs), u32(idxs), torch.empty(0, device="cuda"))
    rng = np.random.default_rng(n)

    def e4m3(shape):                      # finite values of every exponent
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        x[(x & 0x7F) == 0x7F] = 0x08
        return torch.from_numpy(x).cuda()
    blocks8, b8 = e4m3(a.num_blocks * bs * bs), e4m3((cols, n))
    widen = lambda t: t.view(torch.float8_e4m3fn).to(torch.bfloat16).view(torch.int16)   # noqa: E731
    blocks16, b16 = widen(blocks8), widen(b8)
    outs = {k: torch.empty((rows, n), dtype=torch.float32, device="cuda") for k in ("fp8", "bf16", "widen_bf16")}
    runs = {"fp8": lambda: bsr_fp8.spmm_bsr_fp8(a, blocks8, b8, out=outs["fp8"]),
            "bf16": lambda: ops.spmm_bsr_bf16(a, blocks16, b16, out=outs["bf16"]),
            "widen_bf16": lambda: ops.spmm_bsr_bf16(a, widen(blocks8), widen(b8), out=outs["widen_bf16"])}
    tags = {}
    for k, run in runs.items():
        run()
        tags[k] = capi_bsr_fp8.last_kernel() if k == "fp8" else capi.last_kernel()
    torch.cuda.synchronize()
    apart = float((outs["fp8"] - outs["bf16"]).abs().max())
    top = float(outs["bf16"].abs().max())
    assert not bool(torch.isnan(outs["fp8"]).any()) and apart <= 1e-4 * top, f"fp8 and bf16 products differ by {apart} at a largest value of {top}"
    graphs = {k: captured(run, loop) for k, run in runs.items()}
    for g in graphs.values():
        timed(g, loop)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(timed(g, loop))
    med = {k: round(statistics.median(t), 2) for k, t in times.items()}
    index_bytes = 4 * (ptrs.shape[0] + idxs.shape[0])
    floor = {e: round((e * (a.num_blocks * bs * bs + cols * n) + 4 * rows * n + index_bytes) / HBM_BYTES_PER_US, 2) for e in (1, 2)}
    return {"pattern": name, "bS": bs, "N": n, "rows": rows, "blocks": a.num_blocks, "us": med, "spread_us": {k: [round(min(t), 2), round(max(t), 2)] for k, t in times.items()},
            "fp8_over_bf16": round(med["fp8"] / med["bf16"], 3), "fp8_over_widen_bf16": round(med["fp8"] / med["widen_bf16"], 3),
            "floor_us": {"fp8": floor[1], "bf16": floor[2]}, "kernels": tags, "max_abs_difference": apart, "largest_value": top,
            "device": capi.device_info(0)["name"]}


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
    print(json.dumps({"probe": "bsr_fp8", "rounds": a.rounds, "loop": a.loop, "c": "fp32",
                      "timing": "median us of interleaved rounds of a captured graph of `loop` products; widen_bf16 = two casts + the bf16 product",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
