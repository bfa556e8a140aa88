"""Fused block-sparse attention backward (ops.attention_bsr_bwd_bf16: two launches for all heads) against the backward it
replaces at the ops level, once per head: recompute S and P (ops.sddmm_bsr_bf16 -> ops.softmax_bsr with bf16 out), then the
gradient chain of autograd._attention_grads (ops.spmm_bsr_bf16 on A^T for dV, ops.sddmm_bsr_bf16 for dP, ops.softmax_bsr_bwd,
two more ops.spmm_bsr_bf16) with its two `blocks[perm].transpose(1, 2).contiguous()` gathers in torch -- what
block_sparse_attention(fused=True, fused_backward=False) enqueues in its backward.  Same process, same operands, bf16 out of
the forward and bf16 gradients; the shapes of tools/probe/attn_fused_probe.py.  Both candidates are timed in interleaved rounds
(device events around a captured graph of `--loop` back-to-back backwards), medians reported, after the fused gradients have
been compared with the chain's.  floor: Q, K, V, dO, O, lse, the mask, the three gradients and both index sets once at 8 TB/s.
Each case runs in a child process of its own under `timeout`; after a case that fails nothing more is started.  Prints one JSON
line.
  python tools/probe/attn_fused_bwd_probe.py [--rounds 7] [--loop 20] [--seconds 150]      GPU box only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from attn_fused_probe import CASES, HBM_BYTES_PER_US, pattern  # noqa: E402


def one_case(name, d, heads, rounds, loop):
    import numpy as np
    import torch
    from mispmm import capi, capi_attn_bwd, formats, ops
    from sddmm_probe import captured, timed

    rows, cols, bs, ptrs, idxs, mask = pattern(name)
    nb = int(idxs.shape[0])
    t_bsr, perm = ops.bsr_transpose(formats.BSR(rows, cols, nb * bs * bs, bs, bs, ptrs, idxs, np.zeros((nb, bs, bs), np.float32)))
    u32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).cuda()   # noqa: E731
    a = ops.DeviceBSR(rows, cols, bs, bs, nb, u32(ptrs), u32(idxs), torch.empty(0, device="cuda"))
    at = ops.DeviceBSR(cols, rows, bs, bs, nb, u32(t_bsr.block_row_ptrs), u32(t_bsr.block_col_idxs), torch.empty(0, device="cuda"))
    perm32, perm64 = u32(perm), torch.from_numpy(perm.astype(np.int64)).cuda()
    rng = np.random.default_rng(d + heads)
    bf = lambda shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda().to(torch.bfloat16).view(torch.int16)   # noqa: E731
    q, k, v, g = bf((heads, rows, d)), bf((heads, cols, d)), bf((heads, cols, d)), bf((heads, rows, d))
    md = None if mask is None else torch.from_numpy(mask).cuda()
    scale = d ** -0.5
    out, lse = ops.attention_bsr_bf16(a, q, k, v, scale=scale, mask=md, out_bf16=True, return_lse=True)
    grads = lambda: [torch.empty((heads, n, d), dtype=torch.int16, device="cuda") for n in (rows, cols, cols)]   # noqa: E731
    fused_g, chain_g = grads(), grads()
    delta = torch.empty_like(lse)
    s = torch.empty((nb, bs, bs), dtype=torch.float32, device="cuda")
    p = torch.empty((nb, bs, bs), dtype=torch.int16, device="cuda")
    dp, ds = torch.empty_like(s), torch.empty_like(p)

    def fused():
        ops.attention_bsr_bwd_bf16(a, at, perm32, q, k, v, out, lse, g, scale=scale, mask=md, dq=fused_g[0], dk=fused_g[1], dv=fused_g[2], delta=delta)

    def chain():
        for h in range(heads):
            ops.sddmm_bsr_bf16(a, q[h], k[h], out=s)
            ops.softmax_bsr(a, s, scale=scale, mask=md, out_bf16=True, out=p)
            ops.spmm_bsr_bf16(at, p[perm64].transpose(1, 2).contiguous(), g[h], out_bf16=True, out=chain_g[2][h])
            ops.sddmm_bsr_bf16(a, g[h], v[h], out=dp)
            ops.softmax_bsr_bwd(a, p, dp, scale=scale, out_bf16=True, out=ds)
            ops.spmm_bsr_bf16(a, ds, k[h], out_bf16=True, out=chain_g[0][h])
            ops.spmm_bsr_bf16(at, ds[perm64].transpose(1, 2).contiguous(), q[h], out_bf16=True, out=chain_g[1][h])

    fused()
    tag = capi_attn_bwd.last_kernel()
    chain()
    torch.cuda.synchronize()
    apart = {}
    for what, f, c in zip(("dq", "dk", "dv"), fused_g, chain_g):
        f, c = f.view(torch.bfloat16).float(), c.view(torch.bfloat16).float()
        apart[what] = float(((f - c).abs().max() / c.abs().max()))
        assert not bool(torch.isnan(f).any()) and apart[what] <= 2.0 ** -5, f"fused and chain {what} differ by {apart[what]} of the largest element"
    graphs = {"fused": captured(fused, loop), "chain": captured(chain, loop)}
    for _ in range(2):
        for gr in graphs.values():
            timed(gr, loop)
    times = {key: [] for key in graphs}
    for _ in range(rounds):
        for key, gr in graphs.items():
            times[key].append(timed(gr, loop))
    med = {key: statistics.median(t) for key, t in times.items()}
    # Q, dO, O and dQ over the rows, K, V, dK and dV over the keys (bf16), lse, the mask, both index sets and perm
    floor_bytes = (heads * (4 * rows * d + 4 * cols * d) * 2 + heads * rows * 4 + (0 if mask is None else mask.nbytes)
                   + (2 * nb + len(ptrs) + len(t_bsr.block_row_ptrs) + (nb if mask is not None else 0)) * 4)
    floor_us = floor_bytes / HBM_BYTES_PER_US
    per_col = np.diff(t_bsr.block_row_ptrs.astype(np.int64))
    info = capi.device_info(0)
    return {"pattern": name, "bS": bs, "D": d, "Dv": d, "heads": heads, "mask": mask is not None, "kernel": tag,
            "fused_us": round(med["fused"], 2), "fused_best_us": round(min(times["fused"]), 2), "chain_us": round(med["chain"], 2),
            "chain_us_per_head": round(med["chain"] / heads, 2), "chain_over_fused": round(med["chain"] / med["fused"], 2),
            "floor_us": round(floor_us, 2), "fused_x_floor": round(med["fused"] / floor_us, 2), "max_difference_of_largest": apart, "blocks": nb,
            "longest_block_column": int(per_col.max()), "device": info["name"], "cus": info["cu_count"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loop", type=int, default=20)
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
    print(json.dumps({"probe": "attn_fused_bwd", "rounds": a.rounds, "loop": a.loop, "out": "bf16", "gradients": "bf16",
                      "timing": "median of interleaved rounds of a captured graph of `loop` backwards; chain = per head sddmm_bsr_bf16, "
                                "softmax_bsr, then spmm_bsr_bf16 on A^T, sddmm_bsr_bf16, softmax_bsr_bwd, two spmm_bsr_bf16 and two torch "
                                "gathers; floor = Q, K, V, dO, O, lse, mask, dQ, dK, dV and the index arrays once at 8 TB/s",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
