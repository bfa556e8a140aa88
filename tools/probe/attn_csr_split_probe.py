"""The split-row fused attention forward on a CSR pattern (attn_csr_split: every long row dealt to up to S lane groups, two
launches) against the one-launch forward (ops.attention_csr, attn_csr_bf16.attention_csr_bf16), in the same process on the same
operands, fp32 and bf16 operands with an fp32 out, S in 1, 2, 4, ..., 256 at min_batches = 4.
Shapes: GL7d25 (one 422-entry row among short ones) at D = Dv in 64, 128 with 1 and 8 heads; a decoding shape -- M = 64 rows of
8192 sorted random keys out of 65 536, 1 and 8 heads; n4c6-b13 (rows of 14) with 1 and 8 heads, where the split is expected to lose.
All candidates are timed in interleaved rounds (device events around a captured graph of `--loop` back-to-back forwards), medians
and the spread (max - min) / median of the one-launch kernel's rounds reported, after each split result has been compared with the
one-launch kernel's.  Each case runs in a child process of its own under `timeout`; after a case that fails nothing more is
started.  Prints one JSON line; `rule` is what attn_csr_split.default_splits picks, `best` the fastest candidate (0: one launch).
  python tools/probe/attn_csr_split_probe.py [--rounds 5] [--loop 10] [--seconds 120]      GPU box only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SPLITS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
CASES = [(name, d, h, kind) for name, ds in (("GL7d25", (64, 128)), ("decode", (64, 128)), ("n4c6-b13", (64,)))
         for d in ds for h in (1, 8) for kind in ("f32", "bf16")]


def pattern(name):
    import numpy as np
    from mispmm import datasets, formats
    if name != "decode":
        return datasets.load_csr(name)
    m, k, per = 64, 65536, 8192
    rng = np.random.default_rng(31)
    cols = np.concatenate([np.sort(rng.choice(k, size=per, replace=False)) for _ in range(m)]).astype(np.uint32)
    return formats.CSR(m, k, (np.arange(m + 1) * per).astype(np.uint32), cols, np.ones(m * per, np.float32))


def one_case(name, d, heads, kind, rounds, loop):
    import numpy as np
    import torch
    from mispmm import attn_csr_bf16, attn_csr_split, capi, ops
    from sddmm_probe import captured, timed

    csr = pattern(name)
    a = ops.DeviceCSR.from_host(csr, plan=False)
    rng = np.random.default_rng(d + heads)
    f32 = lambda shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda()   # noqa: E731
    q, k, v = f32((heads, csr.num_rows, d)), f32((heads, csr.num_cols, d)), f32((heads, csr.num_cols, d))
    if kind == "bf16":
        q, k, v = (t.to(torch.bfloat16).view(torch.int16) for t in (q, k, v))
    one, split = ((ops.attention_csr, attn_csr_split.attention_csr_split) if kind == "f32" else
                  (attn_csr_bf16.attention_csr_bf16, attn_csr_split.attention_csr_split_bf16))
    outs = {s: torch.empty((heads, csr.num_rows, d), device="cuda") for s in (0,) + SPLITS}
    work = torch.empty(attn_csr_split.workspace_bytes(a, heads, d, max(SPLITS)), dtype=torch.uint8, device="cuda")
    runs = {0: lambda: one(a, q, k, v, out=outs[0])}
    for s in SPLITS:
        runs[s] = lambda s=s: split(a, q, k, v, splits=s, out=outs[s], workspace=work)
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    assert bool((outs[1].view(torch.int32) == outs[0].view(torch.int32)).all()), "splits=1 does not have the one-launch kernel's bits"
    apart = max(float((outs[s] - outs[0]).abs().max()) for s in SPLITS)
    assert not bool(torch.isnan(outs[0]).any()) and apart <= 2.0 ** -16, f"split and one-launch out differ by {apart}"   # |out| <= 1
    graphs = {s: captured(run, loop) for s, run in runs.items()}
    for g in graphs.values():
        timed(g, loop)
    times = {s: [] for s in graphs}
    for _ in range(rounds):
        for s, g in graphs.items():
            times[s].append(timed(g, loop))
    med = {s: round(statistics.median(t), 2) for s, t in times.items()}
    lens = np.diff(csr.row_ptrs.astype(np.int64))
    return {"pattern": name, "kind": kind, "D": d, "heads": heads, "rows": csr.num_rows, "mean_batches": round(float(lens.mean()) / 8, 1),
            "longest_batches": int(-(-lens.max() // 8)), "one_launch_us": med[0], "one_launch_spread": round((max(times[0]) - min(times[0])) / med[0], 3),
            "split_us": {str(s): med[s] for s in SPLITS}, "best": min(med, key=med.get),
            "rule": attn_csr_split.default_splits(a, heads, d, wide=4 if kind == "f32" else 8), "max_abs_difference": apart,
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
    print(json.dumps({"probe": "attn_csr_split", "rounds": a.rounds, "loop": a.loop, "out": "f32", "min_batches": 4,
                      "timing": "median us of interleaved rounds of a captured graph of `loop` forwards; split_us: by splits, two launches each",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
