"""bench.py --dump-outputs and the plain / --full split.

CPU: the row sample of a dump is fixed by the shape alone (two runs, two builds write
the same rows), stays inside its byte budget, and the files hold the sampled rows as
they are plus every row's float64 sum. GPU: one plain run of the headline with
--dump-outputs; the line carries the headline's fields and none of the --full legs,
and the dumped shard is the oracle's, bit for bit, whatever number of steps warmed up."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("shuffled", "config4", "config4_w8", "config4_w32", "config5", "config4_ada", "sparse",
             "cpu_baseline", "native_group")


def test_dump_rows_fixed_sample():
    """All rows when they fit the budget; otherwise budget // row_bytes distinct rows,
    ascending, the same on every call."""
    assert bench.dump_rows(100, 4096, 100 * 4096).tolist() == list(range(100))
    r = bench.dump_rows(bench.ROWS, bench.COLS * 4, bench.DUMP_BYTES)
    assert len(r) == bench.DUMP_BYTES // (bench.COLS * 4) < bench.ROWS
    assert len(r) * bench.COLS * 4 + bench.ROWS * 8 <= 64_000_000  # sample + row sums, bytes
    assert np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < bench.ROWS
    assert np.array_equal(r, bench.dump_rows(bench.ROWS, bench.COLS * 4, bench.DUMP_BYTES))
    assert len(bench.dump_rows(10, 1 << 20, 5)) == 1  # never empty


def test_dump_outputs_files(tmp_path):
    rng = np.random.default_rng(3)
    v = rng.standard_normal((1000, 64)).astype(np.float32)
    d = str(tmp_path / "out")
    bench.dump_outputs(d, "shard", v, budget=300 * 64 * 4)
    assert sorted(os.listdir(d)) == ["shard.npy", "shard_row_sums.npy"]
    a, s = np.load(os.path.join(d, "shard.npy")), np.load(os.path.join(d, "shard_row_sums.npy"))
    assert a.dtype == np.float32 and a.shape == (300, 64)
    assert a.tobytes() == v[bench.dump_rows(1000, 64 * 4, 300 * 64 * 4)].tobytes()
    assert s.dtype == np.float64 and s.shape == (1000,)
    assert np.array_equal(s, v.sum(axis=1, dtype=np.float64))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_shard_bit_exact(oracle, tmp_path):
    """`bench.py --gpus 1 --steps 1 --warmup 2 --dump-outputs DIR`: one line with the
    headline's fields, steps = 1, no --full leg; DIR/shard.npy and shard_row_sums.npy
    equal the oracle fed synth_fill(7), then the first bucket set (32 pushes,
    bench.perm_for orders, value seeds 1000+b) — the warm-up and ramp steps over both
    sets, whose number varies from run to run, leave no trace (the sets' alternation:
    test_gpu_parity.test_config2_headline_steady_state_bit_exact)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "2",
                        "--dump-outputs", d], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    algo = bench.W * bench.BUCKET + 2 * bench.SHARD
    assert line["value"] == pytest.approx(algo / (line["ms_per_step"] * 1e-3) / 2**30, rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line], sorted(line)
    rows, cols, W = bench.ROWS, bench.COLS, bench.W
    o = oracle.OracleStore(1, 0, 1, 0, rows - 1, cols)
    o.synth_fill(7)
    host = [oracle.synth_dense_bucket(0, 1, 0, rows, rows, cols, 1000 + b, *bench.perm_for(b)) for b in range(W)]
    assert o.push_many(host, threads=16) == 0
    del host
    got = np.load(os.path.join(d, "shard.npy"))
    sample = bench.dump_rows(rows, cols * 4, bench.DUMP_BYTES)
    assert got.dtype == np.float32 and got.tobytes() == np.ascontiguousarray(o.data[sample]).tobytes()
    assert np.array_equal(np.load(os.path.join(d, "shard_row_sums.npy")), o.data.sum(axis=1, dtype=np.float64))
