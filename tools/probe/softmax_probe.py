"""Row softmax on a CSR pattern (ops.softmax_csr / ops.softmax_csr_bwd, REFERENCE and FAST) against the torch composition --
scatter_reduce(amax), an index, exp, index_add, an index and a divide (backward: a multiply, index_add, an index, a subtract
and a multiply) -- on the SAME scores, and against the byte floor at 8 TB/s: 2 nnz elements (forward: scores in, out out;
backward 3 nnz: p and dp in, ds out) plus the M + 1 row pointers.  n4c6-b13 and GL7d25, float32.  The candidates are timed in
interleaved rounds (device events around a captured graph of `--loop` back-to-back launches), medians reported; every result
is first checked against the float64 composition.
  python tools/probe/softmax_probe.py [--cases n4c6-b13,GL7d25] [--rounds 7] [--loop 20]      GPU box only."""
import argparse
import os
import platform
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mispmm import capi, datasets, ops  # noqa: E402
from sddmm_probe import HBM_BYTES_PER_US, captured, timed  # noqa: E402


def torch_forward(s, rows, m):
    top = torch.full((m,), float("-inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, rows, s, "amax")
    e = torch.exp(s - top[rows])
    return e / torch.zeros(m, dtype=s.dtype, device=s.device).index_add_(0, rows, e)[rows]


def torch_backward(p, dp, rows, m):
    t = p * dp
    return p * (dp - torch.zeros(m, dtype=p.dtype, device=p.device).index_add_(0, rows, t)[rows])


def probe(name, rounds, loop):
    csr = datasets.load_csr(name)
    a = ops.DeviceCSR.from_host(csr, plan=False)
    m, nnz = csr.num_rows, csr.nnz
    lens = np.diff(csr.row_ptrs.astype(np.int64))
    rng = np.random.default_rng(3)
    s = torch.from_numpy(rng.uniform(-4, 4, nnz).astype(np.float32)).cuda()
    dp = torch.from_numpy(rng.uniform(-1, 1, nnz).astype(np.float32)).cuda()
    rows = torch.from_numpy(np.repeat(np.arange(m), lens)).cuda()
    want = torch_forward(s.double(), rows, m)
    want_ds = torch_backward(want, dp.double(), rows, m)
    p32 = want.float()
    for which, floor_elems in (("forward", 2), ("backward", 3)):
        outs = {acc: torch.empty(nnz, dtype=torch.float32, device="cuda") for acc in ("reference", "fast")}
        if which == "forward":
            runs = {acc: (lambda acc=acc: ops.softmax_csr(a, s, out=outs[acc], acc=acc)) for acc in outs}
            runs["torch"] = lambda: torch_forward(s, rows, m)
            ref, tol = want, 2.0 ** -14
        else:
            runs = {acc: (lambda acc=acc: ops.softmax_csr_bwd(a, p32, dp, out=outs[acc], acc=acc)) for acc in outs}
            runs["torch"] = lambda: torch_backward(p32, dp, rows, m)
            ref, tol = want_ds, 2.0 ** -12
        tags = {}
        for acc in outs:
            runs[acc]()
            tags[acc] = capi.last_kernel()
            assert bool(((outs[acc].double() - ref).abs() <= tol * want + 1e-30).all()), f"{name} {which} {acc}: result off"
        graphs = {k: captured(fn, loop) for k, fn in runs.items()}
        for _ in range(2):
            for g in graphs.values():
                timed(g, loop)
        times = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, g in graphs.items():
                times[k].append(timed(g, loop))
        floor_us = (floor_elems * nnz * 4 + (m + 1) * 4) / HBM_BYTES_PER_US
        med = {k: statistics.median(v) for k, v in times.items()}
        for acc in outs:
            print(f"{name:>10s} {m:7d} {nnz:8d} {int(lens.max()):7d} {which:>9s} {acc:>9s} {med[acc]:9.2f} {min(times[acc]):9.2f} "
                  f"{med['torch']:9.2f} {med['torch'] / med[acc]:13.2f} {floor_us:8.2f} {med[acc] / floor_us:9.2f}  {tags[acc]}", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default="n4c6-b13,GL7d25")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--loop", type=int, default=20)
    a = p.parse_args()
    info = capi.device_info(0)
    print(f"# box {platform.node()}: {info['name']}, {info['cu_count']} CUs")
    print(f"# float32; median (and best) of {a.rounds} interleaved rounds of {a.loop} captured launches; torch = the composition of "
          f"scatter_reduce / index / exp / index_add / divide; floor = score, result and row-pointer bytes at 8 TB/s")
    print(f"{'matrix':>10s} {'M':>7s} {'nnz':>8s} {'longest':>7s} {'pass':>9s} {'mode':>9s} {'kernel_us':>9s} {'best_us':>9s} {'torch_us':>9s} "
          f"{'torch/kernel':>13s} {'floor_us':>8s} {'x floor':>9s}  kernel")
    for name in a.cases.split(","):
        probe(name, a.rounds, a.loop)


if __name__ == "__main__":
    main()
