"""Row softmax on a BSR pattern (ops.softmax_bsr with bf16 out, ops.softmax_bsr_bwd with bf16 p and bf16 out) on ACTIVSg10K BSR-16,
against the torch composition on the SAME arrays -- forward: a multiply, amax over the block's columns, scatter_reduce(amax) over
the block row, an index, exp, a sum, index_add, an index, a divide and the cast to bfloat16; backward: a widening, a multiply, a
sum, index_add, an index, a subtract, two multiplies and the cast -- and against the byte floor at 8 TB/s: forward 4 B read +
2 B written per element, backward 2 + 4 B read + 2 B written.  8.47 M elements make the forward's floor 6.4 us, far above a
launch: unlike the CSR softmax, this kernel is to be judged against it.  The candidates are timed in interleaved rounds (device
events around a captured graph of `--loop` back-to-back launches), medians reported; every result is first checked against the
float64 composition.  Each pass runs in a child process of its own under `timeout`; after a pass that fails nothing more is
started.  Prints one JSON line.
  python tools/probe/softmax_bsr_probe.py [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
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
MATRIX, BLOCK, SCALE = "ACTIVSg10K", 16, 0.125


def one_pass(which, rounds, loop):
    """forward | backward on the GPU: a dict of times in us."""
    import numpy as np
    import torch
    from mispmm import capi, datasets, formats, ops
    from sddmm_probe import captured, timed

    bsr = formats.csr_to_bsr(datasets.load_csr(MATRIX), BLOCK)
    a = ops.DeviceBSR.from_host(bsr)
    mb, shape = bsr.num_block_rows, (bsr.num_blocks, BLOCK, BLOCK)
    counts = np.diff(bsr.block_row_ptrs.astype(np.int64))
    rows = torch.from_numpy(np.repeat(np.arange(mb), counts)).cuda()
    rng = np.random.default_rng(3)
    s = torch.from_numpy(rng.uniform(-4, 4, shape).astype(np.float32)).cuda()
    dp = torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).cuda()

    def torch_forward(s):
        z = s * SCALE
        top = torch.full((mb, BLOCK), float("-inf"), dtype=z.dtype, device=z.device)
        top = top.scatter_reduce(0, rows[:, None].expand(-1, BLOCK), z.amax(dim=2), "amax")
        e = torch.exp(z - top[rows][:, :, None])
        total = torch.zeros((mb, BLOCK), dtype=z.dtype, device=z.device).index_add_(0, rows, e.sum(dim=2))
        return e / total[rows][:, :, None]

    def torch_backward(p, dp):
        dot = torch.zeros((mb, BLOCK), dtype=dp.dtype, device=dp.device).index_add_(0, rows, (p * dp).sum(dim=2))
        return SCALE * (p * (dp - dot[rows][:, :, None]))

    want = torch_forward(s.double())
    p_bits = ops.softmax_bsr(a, s, scale=SCALE, out_bf16=True)
    p_bf = p_bits.view(torch.bfloat16)
    out = torch.empty(shape, dtype=torch.int16, device="cuda")
    if which == "forward":
        runs = {"kernel": lambda: ops.softmax_bsr(a, s, scale=SCALE, out_bf16=True, out=out),
                "torch": lambda: torch_forward(s).to(torch.bfloat16)}
        ref, tol, floor_bytes = want, 2.0 ** -7 * want, 4 + 2
    else:
        runs = {"kernel": lambda: ops.softmax_bsr_bwd(a, p_bits, dp, scale=SCALE, out_bf16=True, out=out),
                "torch": lambda: torch_backward(p_bf.float(), dp).to(torch.bfloat16)}
        ref = torch_backward(p_bf.double(), dp.double())
        tol, floor_bytes = 2.0 ** -7 * ref.abs() + 2.0 ** -12 * p_bf.double(), 2 + 4 + 2
    runs["kernel"]()
    tag = capi.last_kernel()
    err = (out.view(torch.bfloat16).double() - ref).abs()
    assert bool((err <= tol + 1e-300).all()), f"{which}: result off"
    graphs = {k: captured(fn, loop) for k, fn in runs.items()}
    for _ in range(2):
        for g in graphs.values():
            timed(g, loop)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(timed(g, loop))
    elements = bsr.num_blocks * BLOCK * BLOCK
    floor_us = (elements * floor_bytes + (mb + 1) * 4) / HBM_BYTES_PER_US
    med = {k: statistics.median(v) for k, v in times.items()}
    info = capi.device_info(0)
    return {"pass": which, "kernel": tag, "kernel_us": round(med["kernel"], 2), "best_us": round(min(times["kernel"]), 2),
            "torch_us": round(med["torch"], 2), "torch_over_kernel": round(med["torch"] / med["kernel"], 2), "floor_us": round(floor_us, 2),
            "x_floor": round(med["kernel"] / floor_us, 2), "blocks": bsr.num_blocks, "elements": elements,
            "mean_block_row": round(float(counts.mean()), 1), "longest_block_row": int(counts.max()), "device": info["name"], "cus": info["cu_count"]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--loop", type=int, default=20)
    p.add_argument("--seconds", type=int, default=120, help="time limit of one pass")
    p.add_argument("--case", help="internal: forward | backward, run in this process")
    a = p.parse_args()
    if a.case:
        print(json.dumps(one_pass(a.case, a.rounds, a.loop)))
        return 0
    cases, status = [], "ok"
    for which in ("forward", "backward"):
        cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--case", which,
               "--rounds", str(a.rounds), "--loop", str(a.loop)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
            status = f"{which} ended with status {r.returncode}: {r.stderr.strip().splitlines()[-1:] or ''}"
            break
        cases.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"probe": "softmax_bsr", "matrix": f"{MATRIX} BSR-{BLOCK}", "scale": SCALE, "rounds": a.rounds, "loop": a.loop,
                      "timing": "median of interleaved rounds of a captured graph; torch = the composition of amax / scatter_reduce / "
                                "exp / index_add / divide / cast; floor = the arrays' bytes once at 8 TB/s", "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
