"""The split-row fused attention forward (attn_bsr_split.attention_bsr_split_bf16: every block row dealt to S waves, two launches)
against the one-wave forward (ops.attention_bsr_bf16), in the same process on the same operands, bf16 out, S in 1, 2, 4, ..., 64.
Shapes: the probe shapes of tools/probe/attn_fused_probe.py (ACTIVSg10K at 16 x 16 with 1 and 8 heads; the banded-causal pattern
with 16), where units * H fills the card and the split is expected to lose; and a long-context shape -- M = 64 rows against
K = 65 536 keys in 32 x 32 blocks, every block stored (2048 steps per block row), 1 and 8 heads -- where the one-wave kernel runs
8 or 32 waves.  D = Dv = 64 and 128.  All candidates are timed in interleaved rounds (device events around a captured graph of
`--loop` back-to-back forwards), medians reported, after each split result has been compared with the one-wave kernel's.  Each
case runs in a child process of its own under `timeout`; after a case that fails nothing more is started.  Prints one JSON line;
`rule` is what attn_bsr_split.default_splits picks, `best` the fastest candidate (0: the one-wave kernel).
  python tools/probe/attn_split_probe.py [--rounds 5] [--loop 10] [--seconds 120]      GPU box only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SPLITS = (1, 2, 4, 8, 16, 32, 64)
CASES = [(name, d, h) for name, hs in (("ACTIVSg10K", (1, 8)), ("banded", (16,)), ("long", (1, 8))) for d in (64, 128) for h in hs]


def pattern(name):
    import numpy as np
    from attn_fused_probe import pattern as fused_pattern
    if name != "long":
        return fused_pattern(name)
    m, k, bs = 64, 65536, 32
    ptrs = (np.arange(m // bs + 1) * (k // bs)).astype(np.uint32)
    return m, k, bs, ptrs, np.tile(np.arange(k // bs), m // bs).astype(np.uint32), None


def one_case(name, d, heads, rounds, loop):
    import numpy as np
    import torch
    from mispmm import attn_bsr_split, capi, ops
    from sddmm_probe import captured, timed

    rows, cols, bs, ptrs, idxs, mask = pattern(name)
    u32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).cuda()   # noqa: E731
    a = ops.DeviceBSR(rows, cols, bs, bs, int(idxs.shape[0]), u32(ptrs), u32(idxs), torch.empty(0, device="cuda"))
    rng = np.random.default_rng(d + heads)
    bf = lambda shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda().to(torch.bfloat16).view(torch.int16)   # noqa: E731
    q, k, v = bf((heads, rows, d)), bf((heads, cols, d)), bf((heads, cols, d))
    md = None if mask is None else torch.from_numpy(mask).cuda()
    outs = {s: torch.empty((heads, rows, d), dtype=torch.int16, device="cuda") for s in (0,) + SPLITS}
    work = torch.empty(attn_bsr_split.workspace_bytes(a, heads, d, max(SPLITS)), dtype=torch.uint8, device="cuda")
    runs = {0: lambda: ops.attention_bsr_bf16(a, q, k, v, mask=md, out_bf16=True, out=outs[0])}
    for s in SPLITS:
        runs[s] = lambda s=s: attn_bsr_split.attention_bsr_split_bf16(a, q, k, v, mask=md, out_bf16=True, splits=s, out=outs[s], workspace=work)
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    one = outs[0].view(torch.bfloat16).float()
    assert bool((outs[1] == outs[0]).all()), "splits=1 does not have the one-wave kernel's bits"
    apart = max(float((outs[s].view(torch.bfloat16).float() - one).abs().max()) for s in SPLITS)
    assert not bool(torch.isnan(one).any()) and apart <= 2.0 ** -7, f"split and one-wave out differ by {apart}"   # |out| <= 1: a bf16 ulp or two
    graphs = {s: captured(run, loop) for s, run in runs.items()}
    for g in graphs.values():
        timed(g, loop)
    times = {s: [] for s in graphs}
    for _ in range(rounds):
        for s, g in graphs.items():
            times[s].append(timed(g, loop))
    med = {s: round(statistics.median(t), 2) for s, t in times.items()}
    counts = np.diff(ptrs.astype(np.int64))
    steps = counts // (2 if bs == 16 else 1)
    return {"pattern": name, "bS": bs, "D": d, "heads": heads, "units_x_heads": rows // 16 * heads, "mean_steps": round(float(steps.mean()), 1),
            "longest_steps": int(steps.max()), "one_wave_us": med[0], "split_us": {str(s): med[s] for s in SPLITS},
            "best": min(med, key=med.get), "rule": attn_bsr_split.default_splits(a, heads), "max_abs_difference": apart,
            "device": capi.device_info(0)["name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop", type=int, default=10)
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
    print(json.dumps({"probe": "attn_split", "rounds": a.rounds, "loop": a.loop, "out": "bf16",
                      "timing": "median us of interleaved rounds of a captured graph of `loop` forwards; split_us: by splits, two launches each",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
