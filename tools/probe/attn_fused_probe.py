"""Fused block-sparse attention forward (ops.attention_bsr_bf16: one launch for all heads) against the three-launch forward it
replaces (ops.sddmm_bsr_bf16 -> ops.softmax_bsr with bf16 out -> ops.spmm_bsr_bf16, once per head: what
autograd.block_sparse_attention(fused=False) enqueues), in the same process on the same operands, bf16 out.  Shapes: the block
pattern of ACTIVSg10K at 16 x 16 (tests/golden/ACTIVSg10K_bsr16_index.npz) at D = Dv = 64 and 128 with 1 and 8 heads, no mask;
a synthetic banded-causal pattern, M = K = 8192 in 32 x 32 blocks, block row R holding block columns R - 7 .. R (8 blocks per
row, the first rows fewer), the diagonal blocks masked above the diagonal, 16 heads.  Both candidates are timed in interleaved
rounds (device events around a captured graph of `--loop` back-to-back forwards), medians reported, after the fused result has
been compared with the chain's.  floor: Q, K, V, the mask and out once at 8 TB/s.  Each case runs in a child process of its own
under `timeout`; after a case that fails nothing more is started.  Prints one JSON line.
  python tools/probe/attn_fused_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
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
CASES = [("ACTIVSg10K", 64, 1), ("ACTIVSg10K", 64, 8), ("ACTIVSg10K", 128, 1), ("ACTIVSg10K", 128, 8), ("banded", 64, 16), ("banded", 128, 16)]


def pattern(name):
    """(rows, cols, bS, block_row_ptrs, block_col_idxs, mask or None)"""
    import numpy as np
    if name == "ACTIVSg10K":
        z = np.load(os.path.join(ROOT, "tests", "golden", "ACTIVSg10K_bsr16_index.npz"))
        rows, cols, _, bs, _, _ = (int(x) for x in z["header"])
        return rows, cols, bs, z["block_row_ptrs"].astype(np.uint32), z["block_col_idxs"].astype(np.uint32), None
    m, bs, band = 8192, 32, 8
    mb = m // bs
    lists = [np.arange(max(0, r - band + 1), r + 1) for r in range(mb)]
    ptrs = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.uint32)
    cols = np.concatenate(lists).astype(np.uint32)
    mask = np.zeros((cols.shape[0], bs, bs), np.float32)
    mask[ptrs[1:] - 1] = np.where(np.triu(np.ones((bs, bs), bool), k=1), -np.inf, 0.0).astype(np.float32)   # the diagonal block is a row's last
    return m, m, bs, ptrs, cols, mask


def one_case(name, d, heads, rounds, loop):
    import numpy as np
    import torch
    from mispmm import capi, capi_attn, ops
    from sddmm_probe import captured, timed

    rows, cols, bs, ptrs, idxs, mask = pattern(name)
    u32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).cuda()   # noqa: E731
    a = ops.DeviceBSR(rows, cols, bs, bs, int(idxs.shape[0]), u32(ptrs), u32(idxs), torch.empty(0, device="cuda"))
    nb = a.num_blocks
    rng = np.random.default_rng(d + heads)
    bf = lambda shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda().to(torch.bfloat16).view(torch.int16)   # noqa: E731
    q, k, v = bf((heads, rows, d)), bf((heads, cols, d)), bf((heads, cols, d))
    md = None if mask is None else torch.from_numpy(mask).cuda()
    scale = d ** -0.5
    fused_out = torch.empty((heads, rows, d), dtype=torch.int16, device="cuda")
    s = torch.empty((nb, bs, bs), dtype=torch.float32, device="cuda")
    p = torch.empty((nb, bs, bs), dtype=torch.int16, device="cuda")
    chain_out = torch.empty((heads, rows, d), dtype=torch.int16, device="cuda")

    def fused():
        ops.attention_bsr_bf16(a, q, k, v, scale=scale, mask=md, out_bf16=True, out=fused_out)

    def chain():
        for h in range(heads):
            ops.sddmm_bsr_bf16(a, q[h], k[h], out=s)
            ops.softmax_bsr(a, s, scale=scale, mask=md, out_bf16=True, out=p)
            ops.spmm_bsr_bf16(a, p, v[h], out_bf16=True, out=chain_out[h])

    fused()
    tag = capi_attn.last_kernel()
    chain()
    torch.cuda.synchronize()
    f, c = fused_out.view(torch.bfloat16).float(), chain_out.view(torch.bfloat16).float()
    apart = float((f - c).abs().max())
    assert not bool(torch.isnan(f).any()) and apart <= 2.0 ** -5, f"fused and chain differ by {apart}"   # |out| <= 1: a few bf16 ulps
    graphs = {"fused": captured(fused, loop), "chain": captured(chain, loop)}
    for _ in range(2):
        for g in graphs.values():
            timed(g, loop)
    times = {key: [] for key in graphs}
    for _ in range(rounds):
        for key, g in graphs.items():
            times[key].append(timed(g, loop))
    med = {key: statistics.median(t) for key, t in times.items()}
    floor_bytes = heads * (rows * d + 2 * cols * d) * 2 + (0 if mask is None else mask.nbytes) + heads * rows * d * 2 + (nb + len(ptrs)) * 4
    floor_us = floor_bytes / HBM_BYTES_PER_US
    counts = np.diff(ptrs.astype(np.int64))
    info = capi.device_info(0)
    return {"pattern": name, "bS": bs, "D": d, "Dv": d, "heads": heads, "mask": mask is not None, "kernel": tag,
            "fused_us": round(med["fused"], 2), "fused_best_us": round(min(times["fused"]), 2), "chain_us": round(med["chain"], 2),
            "chain_us_per_head": round(med["chain"] / heads, 2), "chain_over_fused": round(med["chain"] / med["fused"], 2),
            "floor_us": round(floor_us, 2), "fused_x_floor": round(med["fused"] / floor_us, 2), "max_abs_difference": apart, "blocks": nb,
            "mean_block_row": round(float(counts.mean()), 1), "longest_block_row": int(counts.max()), "device": info["name"], "cus": info["cu_count"]}


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
    print(json.dumps({"probe": "attn_fused", "rounds": a.rounds, "loop": a.loop, "out": "bf16",
                      "timing": "median of interleaved rounds of a captured graph of `loop` forwards; chain = sddmm_bsr_bf16, softmax_bsr, "
                                "spmm_bsr_bf16 once per head; floor = Q, K, V, mask, out and the index arrays once at 8 TB/s",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
