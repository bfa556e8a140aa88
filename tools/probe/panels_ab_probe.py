"""In-process A/B: the panel-tiled LDS kernel (ops.spmm_csr_panels) against the row-gather kernel (ops.spmm_csr(kernel=5)) on the
SAME operands -- random M x K matrices over a range of densities, N in {128, 1024}, REFERENCE and FAST mode.  The two are timed
in interleaved rounds (HIP events around a hipGraph of `--loop` back-to-back launches), medians reported; every panel result is first
compared with kernel 5's (bitwise in REFERENCE mode).
  python tools/probe/panels_ab_probe.py [--densities 0.01,...] [--ns 128,1024] [--rows 2048 --cols 2048]      GPU box only."""
import argparse
import ctypes
import os
import platform
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mispmm import capi, ops  # noqa: E402
import gen_sparse  # noqa: E402


def captured(fn, loop, stream):
    """`loop` back-to-back launches of fn(stream) as one hipGraph (eager launches of a 10 us kernel time the host)."""
    l, sp, g = capi.lib(), ctypes.c_void_p(stream.cuda_stream), ctypes.c_void_p()
    capi.check(l.mispmm_graph_begin(sp))
    for _ in range(loop):
        fn(stream)
    capi.check(l.mispmm_graph_end(sp, ctypes.byref(g)))
    return g


def timed(graph, loop, stream):
    l, sp = capi.lib(), ctypes.c_void_p(stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    capi.check(l.mispmm_graph_launch(graph, sp))
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / loop


def ab(csr, n, acc, rounds, loop):
    """(median us of kernel 5, median us of the panel kernel, the panel kernel's tag)"""
    rng = np.random.default_rng(n)
    b = torch.from_numpy(rng.uniform(-100, 100, (csr.num_cols, n)).astype(np.float32)).cuda()
    a5, ap = ops.DeviceCSR.from_host(csr), ops.DeviceCSRPanels.from_host(csr)
    c5, cp = torch.empty((csr.num_rows, n), device="cuda"), torch.empty((csr.num_rows, n), device="cuda")
    run5 = lambda st=None: ops.spmm_csr(a5, b, out=c5, kernel=5, acc=acc, stream=st)
    runp = lambda st=None: ops.spmm_csr_panels(ap, b, out=cp, acc=acc, stream=st)
    run5()
    runp()
    tag = capi.last_kernel()
    torch.cuda.synchronize()
    if acc == "reference":
        assert torch.equal(c5.view(torch.int32), cp.view(torch.int32)), "REFERENCE results differ in their bits"
    else:
        assert torch.allclose(c5, cp, rtol=1e-3, atol=1e-5 * 1e4 * csr.num_cols)      # both FAST: a sanity check, |a b| < 1e4 per term
    stream = torch.cuda.Stream()
    g5, gp = captured(run5, loop, stream), captured(runp, loop, stream)
    for g in (g5, gp, g5, gp):                                    # warm-up replays
        timed(g, loop, stream)
    t5, tp = [], []
    for _ in range(rounds):
        t5.append(timed(g5, loop, stream))
        tp.append(timed(gp, loop, stream))
    for g in (g5, gp):
        capi.check(capi.lib().mispmm_graph_destroy(g))
    return statistics.median(t5), statistics.median(tp), tag


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--densities", default="0.01,0.02,0.05,0.1,0.2,0.3,0.5,0.7,0.9")
    p.add_argument("--ns", default="128,1024")
    p.add_argument("--rows", type=int, default=2048)
    p.add_argument("--cols", type=int, default=2048)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--loop", type=int, default=20)
    a = p.parse_args()
    info = capi.device_info(0)
    print(f"# box {platform.node()}: {info['name']}, {info['cu_count']} CUs")
    print(f"# {a.rows} x {a.cols} random A; median of {a.rounds} interleaved rounds of {a.loop} launches")
    print(f"{'density':>7s} {'N':>5s} {'mode':>9s} {'kernel5_us':>11s} {'panels_us':>10s} {'panels/k5':>9s}  panel kernel")
    for d in (float(x) for x in a.densities.split(",")):
        csr = gen_sparse.random_csr(a.rows, a.cols, d, np.random.default_rng([20241218, int(round(d * 1000))]))
        for n in (int(x) for x in a.ns.split(",")):
            for acc in ("reference", "fast"):
                t5, tp, tag = ab(csr, n, acc, a.rounds, a.loop)
                print(f"{d:7.2f} {n:5d} {acc:>9s} {t5:11.1f} {tp:10.1f} {tp / t5:9.3f}  {tag}", flush=True)


if __name__ == "__main__":
    main()
