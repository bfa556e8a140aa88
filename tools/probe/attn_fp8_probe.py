"""The fp8 e4m3 fused block-sparse attention forward (attn_bsr_fp8.attention_bsr_fp8, one launch) against the bf16 one
(ops.attention_bsr_bf16) on the same pattern and the exactly widened operands, against widening Q, K and V first (three torch
casts, then the bf16 launch: what a user with fp8 data did before), and against the byte floor, in the same process, fp32 out.
Shapes: those of tools/probe/attn_fused_probe.py -- the pattern of ACTIVSg10K at 16 x 16 at D = Dv = 64 and 128 with 1 and 8
heads, no mask; the banded causal 32 x 32 pattern with its mask, 16 heads.  All candidates are timed in interleaved rounds
(device events around a captured graph of `--loop` back-to-back launches), medians with min and max reported, after the fp8
result has been compared with the bf16 one.  floor_us: Q, K, V, the mask, out and the index arrays once over 8 TB/s, for either
element size.  Each case runs in a child process of its own under `timeout`; after a case that fails nothing more is started.
Prints one JSON line.
  python tools/probe/attn_fp8_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from attn_fused_probe import CASES   # noqa: E402  (pattern, D = Dv, heads)

HBM_BYTES_PER_US = 8e6


def one_case(name, d, heads, rounds, loop):
    import numpy as np
    import torch
    from mispmm import attn_bsr_fp8, capi, capi_attn, capi_attn_fp8, ops
    from attn_fused_probe import pattern
    from sddmm_probe import captured, timed

    rows, cols, bs, ptrs, idxs, mask = pattern(name)
    u32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).cuda()   # noqa: E731
    a = ops.DeviceBSR(rows, cols, bs, bs, int(idxs.shape[0]), u32(ptrs), u32(idxs), torch.empty(0, device="cuda"))
    md = None if mask is None else torch.from_numpy(mask).cuda()
    g = torch.Generator().manual_seed(d + heads)
    q8, qs = attn_bsr_fp8.quantize_heads(torch.randn((heads, rows, d), generator=g).cuda())
    k8, ks = attn_bsr_fp8.quantize_heads(torch.randn((heads, cols, d), generator=g).cuda())
    v8, vs = attn_bsr_fp8.quantize_heads(torch.randn((heads, cols, d), generator=g).cuda())
    widen = lambda t: t.to(torch.bfloat16).view(torch.int16)   # noqa: E731
    q16, k16, v16 = widen(q8), widen(k8), widen(v8)
    # the bf16 kernel has no per-head scales: the probe's heads share one, folded into `scale` (V's is left out on both sides)
    qs, ks = torch.full_like(qs, float(qs.mean())), torch.full_like(ks, float(ks.mean()))
    scale = d ** -0.5
    folded = float(np.float32(np.float32(scale) * np.float32(qs[0].item())) * np.float32(ks[0].item()))
    outs = {k: torch.empty((heads, rows, d), dtype=torch.float32, device="cuda") for k in ("fp8", "bf16", "widen_bf16")}
    runs = {"fp8": lambda: attn_bsr_fp8.attention_bsr_fp8(a, q8, k8, v8, qs, ks, None, scale=scale, mask=md, out=outs["fp8"]),
            "bf16": lambda: ops.attention_bsr_bf16(a, q16, k16, v16, scale=folded, mask=md, out=outs["bf16"]),
            "widen_bf16": lambda: ops.attention_bsr_bf16(a, widen(q8), widen(k8), widen(v8), scale=folded, mask=md, out=outs["widen_bf16"])}
    tags = {}
    for k, run in runs.items():
        run()
        tags[k] = capi_attn_fp8.last_kernel() if k == "fp8" else capi_attn.last_kernel()
    torch.cuda.synchronize()
    apart = float((outs["fp8"] - outs["bf16"]).abs().max())
    top = float(outs["bf16"].abs().max())
    # the weights differ: e4m3 against bf16, 2^-3 against 2^-8 of a convex combination of e4m3 values, at most 448
    assert not bool(torch.isnan(outs["fp8"]).any()) and apart <= 0.14 * 448.0, f"fp8 and bf16 results differ by {apart} with V up to 448"
    graphs = {k: captured(run, loop) for k, run in runs.items()}
    for gr in graphs.values():
        timed(gr, loop)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, gr in graphs.items():
            times[k].append(timed(gr, loop))
    med = {k: round(statistics.median(t), 2) for k, t in times.items()}
    fixed = (0 if mask is None else mask.nbytes) + heads * rows * d * 4 + 4 * (ptrs.shape[0] + idxs.shape[0])
    floor = {e: round((e * heads * (rows * d + 2 * cols * d) + fixed) / HBM_BYTES_PER_US, 2) for e in (1, 2)}
    return {"pattern": name, "bS": bs, "D": d, "Dv": d, "heads": heads, "mask": mask is not None, "rows": rows, "blocks": a.num_blocks, "us": med,
            "spread_us": {k: [round(min(t), 2), round(max(t), 2)] for k, t in times.items()},
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
    print(json.dumps({"probe": "attn_fp8", "rounds": a.rounds, "loop": a.loop, "out": "fp32",
                      "timing": "median us of interleaved rounds of a captured graph of `loop` launches; widen_bf16 = three casts + the bf16 launch",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
