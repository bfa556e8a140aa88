"""The fused bf16 backward of CSR attention (attn_csr_bf16.attention_csr_bf16_bwd: at most two launches for all heads, reading
bf16) against what a holder of bf16 operands had before it, in the same process on the same operands.  Candidates:
  bf16_grads  the new call, bf16 gradients
  f32_grads   the new call, fp32 gradients
  f32_kernel  ops.attention_csr_bwd on operands widened BEFOREHAND (the widenings are not timed): the fp32 kernel on twice the
              gathered bytes
  today       the backward of autograd.sparse_attention_bf16 without the keyword: ops.bf16_to_f32 of q, k, v and grad_out,
              ops.attention_csr_bwd, ops.f32_to_bf16 of the three gradients -- nine launches and fp32 copies of everything
Shapes: n4c6-b13 and GL7d25 at D = Dv = 64 and 128 with 1 and 8 heads, no bias, all three gradients; out and lse are the bf16
forward's.  All candidates are timed in interleaved rounds (device events around a captured graph of `--loop` back-to-back
backwards), medians reported, after the new call has been compared with the fp32 kernel (inside 2^-12 of the largest gradient:
these scores round, and a lane's chain covers 8 columns against 4) and its bf16 gradients with its fp32 gradients rounded once.
floor: Q, K, V and grad_out at 2 bytes an element, the fp32 out, lse, delta written and read, bf16 dQ, dK and dV, both index
sets and perm, each once at 8 TB/s.  Each case runs in a child process of its own under `timeout`; after a case that fails
nothing more is started.  Prints one JSON line.  Nothing asserts on a time and no dispatcher takes a rule from the figures.
  python tools/probe/attn_csr_bf16_bwd_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
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
CASES = [(name, d, heads) for name in ("n4c6-b13", "GL7d25") for d in (64, 128) for heads in (1, 8)]


def one_case(name, d, heads, rounds, loop):
    import numpy as np
    import torch
    from mispmm import autograd, capi, capi_attn_csr_bf16_bwd, capi_attn_csr_bwd, datasets, ops
    from mispmm.attn_csr_bf16 import attention_csr_bf16, attention_csr_bf16_bwd
    from sddmm_probe import captured, timed

    csr = datasets.load_csr(name)
    t = autograd.TrainableCSR.from_host(csr)
    a, at, perm = t.fwd, t.tpattern, t.perm32()
    rng = np.random.default_rng(d + heads)
    bits = lambda shape: ops.f32_to_bf16(torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda())   # noqa: E731
    m, kk = csr.num_rows, csr.num_cols
    q, k, v, g = bits((heads, m, d)), bits((heads, kk, d)), bits((heads, kk, d)), bits((heads, m, d))
    qf, kf, vf, gf = (ops.bf16_to_f32(x) for x in (q, k, v, g))
    scale = d ** -0.5
    out, lse = attention_csr_bf16(a, q, k, v, scale=scale, return_lse=True)
    delta = torch.empty((heads, m), device="cuda")
    shapes = ((heads, m, d), (heads, kk, d), (heads, kk, d))
    g16 = [torch.empty(s, dtype=torch.int16, device="cuda") for s in shapes]
    g32 = [torch.empty(s, device="cuda") for s in shapes]
    r32 = [torch.empty(s, device="cuda") for s in shapes]

    def bf16_grads():
        attention_csr_bf16_bwd(a, at, perm, q, k, v, out, lse, g, scale=scale, grads_bf16=True, dq=g16[0], dk=g16[1], dv=g16[2], delta=delta)

    def f32_grads():
        attention_csr_bf16_bwd(a, at, perm, q, k, v, out, lse, g, scale=scale, grads_bf16=False, dq=g32[0], dk=g32[1], dv=g32[2], delta=delta)

    def f32_kernel():
        ops.attention_csr_bwd(a, at, perm, qf, kf, vf, out, lse, gf, scale=scale, dq=r32[0], dk=r32[1], dv=r32[2], delta=delta)

    def today():
        grads = ops.attention_csr_bwd(a, at, perm, ops.bf16_to_f32(q), ops.bf16_to_f32(k), ops.bf16_to_f32(v), out, lse, ops.bf16_to_f32(g), scale=scale,
                                      delta=delta)
        return [ops.f32_to_bf16(x) for x in grads]

    bf16_grads()
    tag = capi_attn_csr_bf16_bwd.last_kernel()
    f32_grads()
    f32_kernel()
    f32_tag = capi_attn_csr_bwd.last_kernel()
    torch.cuda.synchronize()
    apart = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(g32, r32))
    rounded = all(bool(torch.equal(ops.f32_to_bf16(x), y)) for x, y in zip(g32, g16))
    assert not any(bool(torch.isnan(x).any()) for x in g32) and apart <= 2.0 ** -12 and rounded, \
        f"new and fp32 kernel differ by {apart} of the largest gradient; bf16 gradients rounded once: {rounded}"
    graphs = {key: captured(f, loop) for key, f in (("bf16_grads", bf16_grads), ("f32_grads", f32_grads), ("f32_kernel", f32_kernel), ("today", today))}
    for _ in range(2):
        for gr in graphs.values():
            timed(gr, loop)
    times = {key: [] for key in graphs}
    for _ in range(rounds):
        for key, gr in graphs.items():
            times[key].append(timed(gr, loop))
    med = {key: statistics.median(t) for key, t in times.items()}
    # q, g, dq: M x d at 2 bytes; k, v, dk, dv: K x d at 2 bytes; out M x d at 4; lse once, delta written and read: 3 M floats
    floor_bytes = heads * (3 * m * d * 2 + 4 * kk * d * 2 + m * d * 4 + 3 * m * 4) + (3 * csr.nnz + m + kk + 2) * 4
    floor_us = floor_bytes / HBM_BYTES_PER_US
    counts = np.diff(csr.row_ptrs.astype(np.int64))
    ccounts = np.bincount(csr.col_idxs.astype(np.int64), minlength=kk)
    info = capi.device_info(0)
    res = {"matrix": name, "rows": m, "cols": kk, "nnz": csr.nnz, "D": d, "Dv": d, "heads": heads, "kernel": tag, "f32_kernel": f32_tag}
    for key in graphs:
        res[key + "_us"] = round(med[key], 2)
        res[key + "_best_us"] = round(min(times[key]), 2)
    res.update({"f32_grads_over_bf16_grads": round(med["f32_grads"] / med["bf16_grads"], 3),
                "f32_kernel_over_bf16_grads": round(med["f32_kernel"] / med["bf16_grads"], 3), "today_over_bf16_grads": round(med["today"] / med["bf16_grads"], 2),
                "floor_us": round(floor_us, 2), "bf16_grads_x_floor": round(med["bf16_grads"] / floor_us, 2), "max_rel_difference_to_f32_kernel": apart,
                "mean_row": round(float(counts.mean()), 1), "longest_row": int(counts.max()), "longest_column": int(ccounts.max()),
                "device": info["name"], "cus": info["cu_count"]})
    return res


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
    print(json.dumps({"probe": "attn_csr_bf16_bwd", "rounds": a.rounds, "loop": a.loop,
                      "timing": "median of interleaved rounds of a captured graph of `loop` backwards; f32_kernel = ops.attention_csr_bwd on operands "
                                "widened beforehand; today = four bf16_to_f32, ops.attention_csr_bwd, three f32_to_bf16; floor = q, k, v, grad_out and "
                                "bf16 dq, dk, dv at 2 bytes, the fp32 out, lse, delta twice, both index sets and perm once at 8 TB/s",
                      "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
