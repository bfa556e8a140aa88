"""SDDMM on a CSR pattern (ops.sddmm_csr, REFERENCE and FAST) against the torch composition (x[rows] * y[cols]).sum(1) on the SAME
operands, and against the byte floor: nnz * N + M * N operand elements (one Y row per entry, every X row once) plus A's indices
and `out`, at 8 TB/s.  n4c6-b13 x N = 128 and GL7d25 x N = 64, float32 (and float64 with --f64).  The candidates are timed in
interleaved rounds (device events around a captured graph of `--loop` back-to-back launches), medians reported; every result is
first checked against the float64 composition.
  python tools/probe/sddmm_probe.py [--cases n4c6-b13:128,GL7d25:64] [--rounds 7] [--loop 20] [--f64]      GPU box only."""
import argparse
import os
import platform
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
from mispmm import capi, datasets, ops  # noqa: E402

HBM_BYTES_PER_US = 8e6     # 8 TB/s


def captured(fn, loop):
    """`loop` back-to-back calls of fn() as one graph (eager launches of a 10 us kernel time the host)."""
    # torch.cuda.graph, not mispmm_graph_*: the torch candidate allocates its nnz x N temporaries, which only torch's own
    # capture (a private pool of its caching allocator) allows
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(loop):
            fn()
    return g


def timed(graph, loop):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / loop


def probe(name, n, dtype, rounds, loop):
    csr = datasets.load_csr(name)
    a = ops.DeviceCSR.from_host(csr, plan=False)
    rng = np.random.default_rng(n)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    x = torch.from_numpy(rng.uniform(-1, 1, (csr.num_rows, n)).astype(npdt)).cuda()
    y = torch.from_numpy(rng.uniform(-1, 1, (csr.num_cols, n)).astype(npdt)).cuda()
    rows = torch.from_numpy(np.repeat(np.arange(csr.num_rows), np.diff(csr.row_ptrs.astype(np.int64)))).cuda()
    cols = torch.from_numpy(csr.col_idxs.astype(np.int64)).cuda()
    outs = {acc: torch.empty(csr.nnz, dtype=dtype, device="cuda") for acc in ("reference", "fast")}
    runs = {acc: (lambda acc=acc: ops.sddmm_csr(a, x, y, out=outs[acc], acc=acc)) for acc in outs}
    runs["torch"] = lambda: (x[rows] * y[cols]).sum(1)
    want = (x.double()[rows] * y.double()[cols]).sum(1)
    scale = (x.double()[rows].abs() * y.double()[cols].abs()).sum(1)
    tags = {}
    for acc in outs:
        runs[acc]()
        tags[acc] = capi.last_kernel()
        tol = 2.0 ** -50 if dtype == torch.float64 else n * 2.0 ** -23
        assert bool(((outs[acc].double() - want).abs() <= tol * scale + 1e-300).all()), f"{name} N={n} {acc}: result off"
    graphs = {k: captured(fn, loop) for k, fn in runs.items()}
    for _ in range(2):
        for g in graphs.values():
            timed(g, loop)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(timed(g, loop))
    elem = 4 if dtype == torch.float32 else 8
    floor_bytes = (csr.nnz * n + csr.num_rows * n) * elem + (csr.nnz + csr.num_rows + 1) * 4 + csr.nnz * elem
    floor_us = floor_bytes / HBM_BYTES_PER_US
    med = {k: statistics.median(v) for k, v in times.items()}
    for acc in outs:
        print(f"{name:>10s} {n:5d} {str(dtype).split('.')[-1]:>8s} {acc:>9s} {med[acc]:9.2f} {min(times[acc]):9.2f} {med['torch']:9.2f} "
              f"{med['torch'] / med[acc]:11.2f} {floor_us:8.2f} {med[acc] / floor_us:9.2f}  {tags[acc]}", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default="n4c6-b13:128,GL7d25:64")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--loop", type=int, default=20)
    p.add_argument("--f64", action="store_true", help="also time float64 operands")
    a = p.parse_args()
    info = capi.device_info(0)
    print(f"# box {platform.node()}: {info['name']}, {info['cu_count']} CUs")
    print(f"# median (and best) of {a.rounds} interleaved rounds of {a.loop} captured launches; torch = (x[rows] * y[cols]).sum(1); "
          f"floor = operand, index and out bytes at 8 TB/s")
    print(f"{'matrix':>10s} {'N':>5s} {'dtype':>8s} {'mode':>9s} {'sddmm_us':>9s} {'best_us':>9s} {'torch_us':>9s} {'torch/sddmm':>11s} "
          f"{'floor_us':>8s} {'x floor':>9s}  kernel")
    for case in a.cases.split(","):
        name, n = case.split(":")
        for dtype in (torch.float32, torch.float64) if a.f64 else (torch.float32,):
            probe(name, int(n), dtype, a.rounds, a.loop)


if __name__ == "__main__":
    main()
