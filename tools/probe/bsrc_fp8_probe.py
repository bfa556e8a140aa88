"""The fp8 e4m3 product on column-compacted strips in step slots (bsrc_fp8.spmm_bsrc_slots_fp8, one launch) against three other
ways to the same product, in the same process, fp32 C, no scales, on ACTIVSg10K as BSR-16 with its values quantised per row to
e4m3 (bsrc_fp8.quantize_bsr_rows) and B in random finite e4m3:
  slots_fp8        the new kernel;
  bsr_fp8          the dense-block fp8 product (bsr_fp8.spmm_bsr_fp8) on the same bytes;
  slots_bf16       ops.spmm_bsrc_slots_bf16 on the exactly widened operands (widened once, outside the timing);
  widen_slots_bf16 the tiles and B cast to bf16 inside the timing (two torch casts), then ops.spmm_bsrc_slots_bf16.
Shapes: N = 128 (BASELINE config 4's) and N = 512.  All candidates are timed in interleaved rounds (device events around a
captured graph of `--loop` back-to-back products), the median with min-max reported, after every result has been compared with
slots_bf16's.  floor_us: the operand bytes of A in either layout and element size, B once and C, over 8 TB/s.  Each case runs in
a child process of its own under `timeout`; after a case that fails nothing more is started.  Prints one JSON line.
  python tools/probe/bsrc_fp8_probe.py [--rounds 9] [--loop 20] [--seconds 180]      GPU box only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cuda-optimization-for-spmm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = [("ACTIVSg10K", 128), ("ACTIVSg10K", 512)]
HBM_BYTES_PER_US = 8e6


def one_case(name, n, rounds, loop):
    import numpy as np
    import torch
    from mispmm import bsr_fp8, bsrc_fp8, capi, capi_bsr_fp8, capi_bsrc_fp8, datasets, formats, ops
    from sddmm_probe import captured, timed

    f8 = torch.float8_e4m3fn
    bsr = formats.csr_to_bsr(datasets.load_csr(name), 16)
    q, _ = bsrc_fp8.quantize_bsr_rows(bsr)
    rows, cols, nb = bsr.num_rows, bsr.num_cols, bsr.num_blocks
    a8 = bsrc_fp8.DeviceBSRCSlotsFP8.from_blocks(bsr, q)
    dense8 = ops.DeviceBSR(rows, cols, 16, 16, nb, ops._dev_u32(bsr.block_row_ptrs, "cuda"), ops._dev_u32(bsr.block_col_idxs, "cuda"), None)
    blocks8 = q.view(torch.uint8).reshape(-1).cuda()
    bsr.data = q.to(torch.float32).numpy()                       # the widened values: exact in bf16
    a16 = ops.DeviceBSRCSlots.from_host(bsr)
    widen = lambda t: t.view(f8).to(torch.bfloat16).view(torch.int16)   # noqa: E731
    # block columns ascend and none repeats here, so both layouts list the same columns in the same order
    assert a16.num_steps == a8.num_steps and torch.equal(a16.cols, a8.cols) and torch.equal(a16.tiles, widen(a8.tiles).reshape(-1))
    rng = np.random.default_rng(n)
    x = rng.integers(0, 256, (cols, n), dtype=np.uint8)
    x[(x & 0x7F) == 0x7F] = 0x08
    b8 = torch.from_numpy(x).cuda()
    b16 = widen(b8)
    outs = {k: torch.empty((rows, n), dtype=torch.float32, device="cuda") for k in ("slots_fp8", "bsr_fp8", "slots_bf16", "widen_slots_bf16")}

    def widened():
        return ops.DeviceBSRCSlots(rows, cols, a8.num_steps, a8.used_steps, a8.extra_ptrs, a8.cols, widen(a8.tiles))
    runs = {"slots_fp8": lambda: bsrc_fp8.spmm_bsrc_slots_fp8(a8, b8, out=outs["slots_fp8"]),
            "bsr_fp8": lambda: bsr_fp8.spmm_bsr_fp8(dense8, blocks8, b8, out=outs["bsr_fp8"]),
            "slots_bf16": lambda: ops.spmm_bsrc_slots_bf16(a16, b16, out=outs["slots_bf16"]),
            "widen_slots_bf16": lambda: ops.spmm_bsrc_slots_bf16(widened(), widen(b8), out=outs["widen_slots_bf16"])}
    last = {"slots_fp8": capi_bsrc_fp8.last_kernel, "bsr_fp8": capi_bsr_fp8.last_kernel}
    tags = {}
    for k, run in runs.items():
        run()
        tags[k] = last.get(k, capi.last_kernel)()
    torch.cuda.synchronize()
    top = float(outs["slots_bf16"].abs().max())
    apart = {k: float((o - outs["slots_bf16"]).abs().max()) for k, o in outs.items()}
    assert not any(bool(torch.isnan(o).any()) for o in outs.values()) and max(apart.values()) <= 1e-3 * top, f"the products differ: {apart} at {top}"
    graphs = {k: captured(run, loop) for k, run in runs.items()}
    for g in graphs.values():
        timed(g, loop)
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(timed(g, loop))
    med = {k: round(statistics.median(t), 2) for k, t in times.items()}
    floor = {"slots_fp8": a8.operand_bytes() + cols * n, "bsr_fp8": nb * 256 + 4 * (nb + rows // 16 + 1) + cols * n,
             "slots_bf16": a16.operand_bytes() + 2 * cols * n}
    return {"pattern": name, "bS": 16, "N": n, "rows": rows, "blocks": nb, "steps": a8.num_steps, "used_steps": a8.used_steps, "us": med,
            "spread_us": {k: [round(min(t), 2), round(max(t), 2)] for k, t in times.items()},
            "slots_fp8_over_slots_bf16": round(med["slots_fp8"] / med["slots_bf16"], 3), "slots_fp8_over_bsr_fp8": round(med["slots_fp8"] / med["bsr_fp8"], 3),
            "slots_fp8_over_widen_slots_bf16": round(med["slots_fp8"] / med["widen_slots_bf16"], 3),
            "floor_us": {k: round((v + 4 * rows * n) / HBM_BYTES_PER_US, 2) for k, v in floor.items()}, "kernels": tags,
            "max_abs_difference_from_slots_bf16": apart, "largest_value": top, "device": capi.device_info(0)["name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--loop", type=int, default=20)
    ap.add_argument("--seconds", type=int, default=180, help="time limit of one case")
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
            status = f"case {case} ended with status {r.returncode}: {r.stderr.strip().splitlines()[-3:] or ''}"
            break
        cases.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"probe": "bsrc_fp8", "rounds": a.rounds, "loop": a.loop, "c": "fp32",
                      "timing": "median us of interleaved rounds of a captured graph of `loop` products; widen_slots_bf16 = two casts + the bf16 slots product",
                      "status": status, "cases": cases}, indent=1))
    return 0 if status == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
