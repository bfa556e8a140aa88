"""bench.py itself: the plain line (the headline and nothing else), --dump-outputs, and the argument checks.  The --full line
is checked by tests/test_cli.py::test_bench_line_contract and tests/test_zz_perf_gpu.py (fixture bench_line)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float32_and_caps_the_size_with_a_seeded_row_sample(tmp_path, monkeypatch):
    bench = _bench_module()
    c = np.arange(600 * 16, dtype=np.float32).reshape(600, 16)
    bench.dump_outputs(str(tmp_path / "whole"), {"c": c})
    got = np.load(tmp_path / "whole" / "c.npy")
    assert got.dtype == np.float32 and np.array_equal(got, c) and not (tmp_path / "whole" / "c_rows.npy").exists()
    monkeypatch.setattr(bench, "DUMP_BYTES", 100 * (16 * 4 + 8))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"c": c})
    rows = np.load(tmp_path / "a" / "c_rows.npy")
    part = np.load(tmp_path / "a" / "c.npy")
    assert rows.dtype == np.float64 and len(rows) == 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(part, c[rows.astype(np.int64)])
    assert part.nbytes + rows.nbytes <= bench.DUMP_BYTES
    assert np.array_equal(rows, np.load(tmp_path / "b" / "c_rows.npy"))      # the same sample every run


def test_bench_rejects_zero_steps():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr


@pytest.mark.gpu
def test_plain_line_times_exactly_its_steps_and_dumps_the_product(tmp_path, oracle):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the contract fields, K timed steps, no extras; the dumped C of
    the last timed step is the oracle's product bit for bit (REFERENCE accumulate mode)."""
    from mispmm import datasets, synth
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "1500", "--warmup", "3", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 1500 and line["warmup"] == 3 and line["timing"]["timed_steps"] == 1500
    assert abs(line["timing"]["timed_ms"] / 1500 - line["ms_per_step"]) <= 1e-6 + 1e-3 * line["ms_per_step"]
    for extra in ("cpu_baseline", "hbm_streaming", "other_acc_mode", "batched"):
        assert extra not in line, extra
    csr = datasets.load_csr("n4c6-b13")
    want = oracle.spmm_csr(csr.row_ptrs, csr.col_idxs, csr.data, synth.dense_b(csr.num_cols, 128))
    got = np.load(out / "c.npy")
    assert got.dtype == np.float32 and np.array_equal(got, want)
