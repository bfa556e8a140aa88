"""SDDMM on a BSR pattern in bf16 (ops.sddmm_bsr_bf16, fp32 and bf16 out) on ACTIVSg10K BSR-16 at N = 128 and N = 512, against the
torch composition -- a batched bmm over the gathered row panels, torch.bmm(x[rows], y[cols].transpose(1, 2)) in bfloat16 -- on
the SAME operands, and against the byte floor: X and Y read once, `out` written once, at 8 TB/s.  The candidates are timed in
interleaved rounds (device events around a captured graph of `--loop` back-to-back launches), medians reported; every result is
first checked against the float64 product.  Every (N, out type) case runs in a child process of its own under `timeout`; after
a case that fails nothing more is started.  Prints one JSON line.
  python tools/probe/sddmm_bsr_probe.py [--widths 128,512] [--rounds 7] [--loop 20] [--seconds 120]      GPU box only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))

HBM_BYTES_PER_US = 8e6     # 8 TB/s
MATRIX, BLOCK = "ACTIVSg10K", 16


def case(n, out_bf16, rounds, loop):
    """One (N, out type) on the GPU: a dict of times in us."""
    import numpy as np
    import torch
    from mispmm import capi, datasets, formats, ops
    from sddmm_probe import captured, timed

    bsr = formats.csr_to_bsr(datasets.load_csr(MATRIX), BLOCK)
    a = ops.DeviceBSR.from_host(bsr)
    rng = np.random.default_rng(n)
    x = torch.from_numpy(rng.uniform(-1, 1, (bsr.num_rows, n)).astype(np.float32)).cuda().to(torch.bfloat16)
    y = torch.from_numpy(rng.uniform(-1, 1, (bsr.num_cols, n)).astype(np.float32)).cuda().to(torch.bfloat16)
    within = torch.arange(BLOCK, device="cuda")
    rows = torch.from_numpy(np.repeat(np.arange(bsr.num_block_rows), np.diff(bsr.block_row_ptrs.astype(np.int64)))).cuda()[:, None] * BLOCK + within
    cols = torch.from_numpy(bsr.block_col_idxs.astype(np.int64)).cuda()[:, None] * BLOCK + within
    out = torch.empty((bsr.num_blocks, BLOCK, BLOCK), dtype=torch.int16 if out_bf16 else torch.float32, device="cuda")
    xb, yb = x.view(torch.int16), y.view(torch.int16)
    runs = {"sddmm": lambda: ops.sddmm_bsr_bf16(a, xb, yb, out_bf16=out_bf16, out=out),
            "torch": lambda: torch.bmm(x[rows], y[cols].transpose(1, 2))}
    runs["sddmm"]()
    tag = capi.last_kernel()
    got = (out.view(torch.bfloat16) if out_bf16 else out).double()
    step, worst = 2048, 0.0
    for lo in range(0, bsr.num_blocks, step):            # the float64 product, a slab of blocks at a time
        xp, yp = x[rows[lo:lo + step]].double(), y[cols[lo:lo + step]].double()
        want, scale = torch.bmm(xp, yp.transpose(1, 2)), torch.bmm(xp.abs(), yp.abs().transpose(1, 2))
        tol = n * 2.0 ** -22 * scale + (2.0 ** -8 * want.abs() if out_bf16 else 0.0)
        err = (got[lo:lo + step] - want).abs()
        assert bool((err <= tol + 1e-300).all()), f"N={n} out_bf16={out_bf16}: result off"
        worst = max(worst, float((err / (tol + 1e-300)).max()))
    graphs = {k: captured(fn, loop) for k, fn in runs.items()}
    for _ in range(2):
        for g in graphs.values():
            timed(g, loop)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(timed(g, loop))
    floor_us = ((bsr.num_rows + bsr.num_cols) * n * 2 + out.numel() * out.element_size()) / HBM_BYTES_PER_US
    med = {k: statistics.median(v) for k, v in times.items()}
    info = capi.device_info(0)
    return {"n": n, "out": "bf16" if out_bf16 else "f32", "kernel": tag, "sddmm_us": round(med["sddmm"], 2), "best_us": round(min(times["sddmm"]), 2),
            "torch_us": round(med["torch"], 2), "torch_over_sddmm": round(med["torch"] / med["sddmm"], 2), "floor_us": round(floor_us, 2),
            "x_floor": round(med["sddmm"] / floor_us, 2), "err_over_tol": round(worst, 4), "blocks": bsr.num_blocks, "device": info["name"], "cus": info["cu_count"]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--widths", default="128,512")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--loop", type=int, default=20)
    p.add_argument("--seconds", type=int, default=120, help="time limit of one case")
    p.add_argument("--case", help="internal: N:f32|bf16, run in this process")
    a = p.parse_args()
    if a.case:
        n, out = a.case.split(":")
        print(json.dumps(case(int(n), out == "bf16", a.rounds, a.loop)))
        return 0
    cases, status = [], "ok"
    for n in a.widths.split(","):
        for out in ("f32", "bf16"):
            cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--case", f"{n}:{out}",
                   "--rounds", str(a.rounds), "--loop", str(a.loop)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
                status = f"case {n}:{out} ended with status {r.returncode}: {r.stderr.strip().splitlines()[-1:] or ''}"
                break
            cases.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if status != "ok":
            break
    print(json.dumps({"probe": "sddmm_bsr_bf16", "matrix": f"{MATRIX} BSR-{BLOCK}", "rounds": a.rounds, "loop": a.loop,
                      "timing": "median of interleaved rounds of a captured graph; torch = bmm over gathered bf16 row panels; "
                                "floor = X, Y read once and out written once at 8 TB/s", "status": status, "cases": cases}))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
