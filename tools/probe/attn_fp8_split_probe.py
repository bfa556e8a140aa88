"""The split-row fp8 e4m3 fused attention forward (attn_bsr_fp8_split.attention_bsr_fp8_split, two launches) at S = 1 .. 64
against what a user had before it: attn_bsr_fp8.attention_bsr_fp8 (one launch, one wave per 16 rows) and
attn_bsr_split.attention_bsr_split_bf16 at its own default splits on widened operands, with and without the three casts; for
shared KV heads, the one-launch fp8 kernel on K and V repeated per query head, the repeat included (the bf16 split kernel has no
per-head scales and one head stride: it is not run there).  Shapes: the long-context shape of tools/probe/attn_split_probe.py
(M = 64, K = 65 536, 32 x 32 blocks, every block stored) at D = Dv = 64 and 128 with 1 and 8 heads, and 8 heads over 2 KV
heads; ACTIVSg10K at 16 x 16 and the banded causal 32 x 32 pattern as the shapes that should NOT gain.  All candidates are
timed in interleaved rounds (device events around a captured graph of `--loop` back-to-back forwards), medians with min and
max reported, after every split result has been compared with S = 1.  Each case runs in a child process of its own under
`timeout`; after a case that fails nothing more is started.  Prints one JSON line; `rule` is what default_splits picks.
  python tools/probe/attn_fp8_split_probe.py [--rounds 5] [--loop 10] [--seconds 150]      GPU box only."""
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
# (pattern, D = Dv, query heads, KV heads)
CASES = [("long", d, h, hkv) for d in (64, 128) for h, hkv in ((1, 1), (8, 8), (8, 2))] + [("ACTIVSg10K", 128, 8, 8), ("banded", 128, 16, 16)]


def one_case(name, d, heads, kv_heads, rounds, loop):
    import numpy as np
    import torch
    from mispmm import attn_bsr_fp8, attn_bsr_fp8_split, attn_bsr_split, capi, ops
    from attn_split_probe import pattern
    from sddmm_probe import captured, timed

    rows, cols, bs, ptrs, idxs, mask = pattern(name)
    u32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).cuda()   # noqa: E731
    a = ops.DeviceBSR(rows, cols, bs, bs, int(idxs.shape[0]), u32(ptrs), u32(idxs), torch.empty(0, device="cuda"))
    md = None if mask is None else torch.from_numpy(mask).cuda()
    g = torch.Generator().manual_seed(d + heads)
    q8, qs = attn_bsr_fp8.quantize_heads(torch.randn((heads, rows, d), generator=g).cuda())
    k8, ks = attn_bsr_fp8.quantize_heads(torch.randn((kv_heads, cols, d), generator=g).cuda())
    v8, _ = attn_bsr_fp8.quantize_heads(torch.randn((kv_heads, cols, d), generator=g).cuda())
    # the bf16 kernels have no per-head scales: the probe's heads share one, folded into `scale` (V's is left out on all sides)
    qs, ks = torch.full_like(qs, float(qs.mean())), torch.full_like(ks, float(ks.mean()))
    scale = d ** -0.5
    folded = float(np.float32(np.float32(scale) * np.float32(qs[0].item())) * np.float32(ks[0].item()))
    group = heads // kv_heads
    new = lambda: torch.empty((heads, rows, d), dtype=torch.float32, device="cuda")   # noqa: E731
    outs = {f"S{s}": new() for s in SPLITS}
    ws = torch.empty(attn_bsr_fp8_split.workspace_bytes(a, heads, d, max(SPLITS)), dtype=torch.uint8, device="cuda")
    split = attn_bsr_fp8_split.attention_bsr_fp8_split
    runs = {f"S{s}": (lambda s=s: split(a, q8, k8, v8, qs, ks, None, scale=scale, mask=md, splits=s, out=outs[f"S{s}"], workspace=ws)) for s in SPLITS}
    if group == 1:
        widen = lambda t: t.to(torch.bfloat16).view(torch.int16)   # noqa: E731
        q16, k16, v16 = widen(q8), widen(k8), widen(v8)
        s16 = attn_bsr_split.default_splits(a, heads)
        ws16 = torch.empty(max(16, attn_bsr_split.workspace_bytes(a, heads, d, s16)), dtype=torch.uint8, device="cuda")
        outs.update(fp8_one=new(), bf16_split=new(), widen_bf16_split=new())
        bf16 = lambda q, k, v, o: attn_bsr_split.attention_bsr_split_bf16(a, q, k, v, scale=folded, mask=md, splits=None if s16 == 1 else s16,   # noqa: E731
                                                                          out=o, workspace=None if s16 == 1 else ws16)
        runs["fp8_one"] = lambda: attn_bsr_fp8.attention_bsr_fp8(a, q8, k8, v8, qs, ks, None, scale=scale, mask=md, out=outs["fp8_one"])
        runs["bf16_split"] = lambda: bf16(q16, k16, v16, outs["bf16_split"])
        runs["widen_bf16_split"] = lambda: bf16(widen(q8), widen(k8), widen(v8), outs["widen_bf16_split"])
    else:
        s16 = None
        outs["fp8_one_repeat"] = new()
        rep = lambda t: t.repeat_interleave(group, dim=0)   # noqa: E731
        runs["fp8_one_repeat"] = lambda: attn_bsr_fp8.attention_bsr_fp8(a, q8, rep(k8), rep(v8), qs, rep(ks), None, scale=scale, mask=md,
                                                                       out=outs["fp8_one_repeat"])
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    one = "fp8_one" if group == 1 else "fp8_one_repeat"
    assert torch.equal(outs["S1"], outs[one]), "S = 1 differs from the one-launch kernel"
    apart = max(float((outs[f"S{s}"] - outs["S1"]).abs().max()) for s in SPLITS)
    # a segment rounds its weights to e4m3 against its own running maximum: 2^-3 of a convex combination of e4m3 values, at most 448
    assert not bool(torch.isnan(outs["S64"]).any()) and apart <= 0.14 * 448.0, f"split results differ from S = 1 by {apart}"
    graphs = {k: captured(run, loop) for k, run in runs.items()}
    for gr in graphs.values():
        timed(gr, loop)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, gr in graphs.items():
            times[k].append(timed(gr, loop))
    med = {k: round(statistics.median(t), 2) for k, t in times.items()}
    best = min((f"S{s}" for s in SPLITS), key=med.get)
    return {"pattern": name, "bS": bs, "D": d, "Dv": d, "heads": heads, "kv_heads": kv_heads, "mask": mask is not None, "rows": rows,
            "blocks": a.num_blocks, "us": med, "spread_us": {k: [round(min(t), 2), round(max(t), 2)] for k, t in times.items()},
            "rule": attn_bsr_fp8_split.default_splits(a, heads), "best": best, "bf16_splits": s16, "max_abs_difference_from_S1": apart,
            "device": capi.device_info(0)["name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=150, help="time limit of one case")
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
        print(f"{case}: {cases[-1]['us']}", file=sys.stderr, flush=True)
    print(json.dumps({"probe": "attn_fp8_split", "rounds": a.rounds, "loop": a.loop, "out": "fp32",
                      "timing": "median us of interleaved rounds of a captured graph of `loop` forwards; widen_bf16_split = three casts + the "
                                "bf16 split call at its default splits; fp8_one_repeat = K and V repeated per query head + the one-launch kernel",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
