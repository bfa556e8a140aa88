"""Decode attention on a paged fp8 e4m3 KV cache (attn_decode_fp8.attention_decode_fp8: a KV group's query heads packed into one
MFMA tile) against what a user had before it: the same decode problem through attn_bsr_fp8_split.attention_bsr_fp8_split, one
block row of bS query rows per sequence with the token's q in its first row, at S = 1 .. 64 on BOTH sides, each side's best S
compared.  Shapes: B in (1, 8, 64) sequences of 8 192 and 65 536 keys, D = Dv = 128, pages of 16 and 32 keys in a shuffled
cache, (H, Hkv) = (32, 8) and (64, 8); seq_lens is given (the `len` instances) and holds full pages, the old side runs without
a mask.  Before any timing both sides are compared bit for bit at every S.  All candidates are timed in interleaved rounds
(device events around a captured graph of `--loop` back-to-back forwards), medians with min and max reported.  `floor_us`:
K and V of every sequence read once over 8.0 TB/s, the HBM peak this project's fractions use.  The cases of one (bS, H) run in a
child process of their own under `timeout`; after a child that fails nothing more is started.  Prints one JSON line; `rule` is
what default_splits picks.
  python tools/probe/attn_fp8_decode_probe.py [--rounds 5] [--loop 10] [--seconds 280]      GPU box only."""
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
D, HKV, PEAK = 128, 8, 8.0e12
GROUPS = [(bs, h) for bs in (16, 32) for h in (32, 64)]                        # one child process each
SHAPES = [(b, ctx) for b in (1, 8, 64) for ctx in (8192, 65536)]


def one_case(bs, heads, batch, ctx, rounds, loop):
    import torch
    from mispmm import attn_bsr_fp8_split, attn_decode_fp8, capi, ops
    from sddmm_probe import captured, timed

    g = torch.Generator(device="cuda").manual_seed(batch + ctx)
    pages = batch * ctx // bs
    some = lambda *shape: (torch.randint(0x20, 0x40, shape, generator=g, device="cuda", dtype=torch.uint8)          # noqa: E731
                           | (torch.randint(0, 2, shape, generator=g, device="cuda", dtype=torch.uint8) << 7))      # +-[2^-3, 2): finite e4m3
    q, k, v = some(batch, heads, D), some(HKV, pages * bs, D), some(HKV, pages * bs, D)
    ptrs = (torch.arange(batch + 1, device="cuda") * (ctx // bs)).to(torch.int32)
    idxs = torch.randperm(pages, generator=g, device="cuda").to(torch.int32)                                       # a shuffled cache
    lens = torch.full((batch,), ctx, dtype=torch.int32, device="cuda")
    scale = D ** -0.5
    # the old side: one block row of bs query rows per sequence, the token in its first row
    a = ops.DeviceBSR(batch * bs, pages * bs, bs, bs, pages, ptrs, idxs, torch.empty(0, device="cuda"))
    rows = torch.zeros((heads, batch * bs, D), dtype=torch.uint8, device="cuda")
    rows[:, ::bs] = q.permute(1, 0, 2)
    new_out = {s: torch.empty((batch, heads, D), device="cuda") for s in SPLITS}
    old_out = {s: torch.empty((heads, batch * bs, D), device="cuda") for s in SPLITS}
    ws_new = torch.empty(attn_decode_fp8.workspace_bytes(batch, heads, heads // HKV, D, max(SPLITS)), dtype=torch.uint8, device="cuda")
    ws_old = torch.empty(attn_bsr_fp8_split.workspace_bytes(a, heads, D, max(SPLITS)), dtype=torch.uint8, device="cuda")
    runs = {}
    for s in SPLITS:
        runs[f"decode_S{s}"] = lambda s=s: attn_decode_fp8.attention_decode_fp8(ptrs, idxs, bs, q, k, v, seq_lens=lens, scale=scale, splits=s,
                                                                               out=new_out[s], workspace=ws_new)
        runs[f"split_S{s}"] = lambda s=s: attn_bsr_fp8_split.attention_bsr_fp8_split(a, rows, k, v, scale=scale, splits=s, out=old_out[s],
                                                                                    workspace=ws_old)
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    for s in SPLITS:   # packing changes no bit (include/mispmm_attn_fp8_decode.h)
        assert torch.equal(new_out[s].view(torch.int32), old_out[s][:, ::bs].permute(1, 0, 2).contiguous().view(torch.int32)), f"S = {s} differs"
    graphs = {name: captured(run, loop) for name, run in runs.items()}
    for gr in graphs.values():
        timed(gr, loop)
    times = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, gr in graphs.items():
            times[name].append(timed(gr, loop))
    med = {name: round(statistics.median(t), 2) for name, t in times.items()}
    best_new = min((f"decode_S{s}" for s in SPLITS), key=med.get)
    best_old = min((f"split_S{s}" for s in SPLITS), key=med.get)
    rule = attn_decode_fp8.default_splits(batch, HKV, pages, bs)
    return {"bS": bs, "heads": heads, "kv_heads": HKV, "B": batch, "context": ctx, "D": D, "Dv": D, "us": med,
            "spread_us": {name: [round(min(t), 2), round(max(t), 2)] for name, t in times.items()}, "best_decode": best_new,
            "best_split": best_old, "ratio_split_over_decode": round(med[best_old] / med[best_new], 3), "rule": rule,
            "rule_us": med[f"decode_S{rule}"] if rule in SPLITS else None, "rule_split": attn_bsr_fp8_split.default_splits(a, heads),
            "floor_us": round(2 * batch * ctx * HKV * D / PEAK * 1e6, 2), "device": capi.device_info(0)["name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=280, help="time limit of one child")
    ap.add_argument("--group", type=int, help="internal: index into GROUPS, run in this process")
    a = ap.parse_args()
    if a.group is not None:
        for shape in SHAPES:
            print(json.dumps(one_case(*GROUPS[a.group], *shape, a.rounds, a.loop)), flush=True)
        return 0
    cases, status = [], "ok"
    for i, group in enumerate(GROUPS):
        cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--group", str(i),
               "--rounds", str(a.rounds), "--loop", str(a.loop)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        cases += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
        if r.returncode != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
            status = f"group {group} ended with status {r.returncode}: {r.stderr.strip().splitlines()[-1:] or ''}"
            break
        print(f"{group}: done, {len(cases)} cases", file=sys.stderr, flush=True)
    print(json.dumps({"probe": "attn_fp8_decode", "rounds": a.rounds, "loop": a.loop, "out": "fp32",
                      "timing": "median us of interleaved rounds of a captured graph of `loop` forwards; decode_S<n> = attention_decode_fp8, "
                                "split_S<n> = attention_bsr_fp8_split on one block row per sequence; floor_us = K and V once over 8.0 TB/s",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
