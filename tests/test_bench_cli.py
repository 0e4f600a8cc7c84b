"""bench.py's command line: a plain run measures the headline figure only
(everything else sits behind --full), --dump-outputs writes what the last
timed step computed, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_drops_every_extra_leg(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    assert not (a.cpu_baseline or a.e2e or a.cold)
    a = _args(monkeypatch, "--full")
    assert a.full and a.cpu_baseline and a.e2e and a.cold
    a = _args(monkeypatch, "--full", "--no-cpu-baseline", "--no-cold")
    assert a.full and a.e2e and not (a.cpu_baseline or a.cold)


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _args(monkeypatch, "--steps", "0")


def test_sample_rows_fixed_sorted_and_within_budget():
    n = 16384
    r = bench.sample_rows(n, n * 12, 3)
    assert np.array_equal(r, bench.sample_rows(n, n * 12, 3))  # the seed and the sizes only
    assert len(r) * n * 12 <= bench.DUMP_BUDGET < 64e6 and len(r) == 256
    assert np.all(np.diff(r) > 0) and 0 <= r[0] and r[-1] < n
    assert not np.array_equal(r, bench.sample_rows(n, n * 12, 4))
    # a table that fits: every row; a shard's rows: inside the shard
    assert np.array_equal(bench.sample_rows(1000, 12000, 1), np.arange(1000))
    s = bench.sample_rows(n // 2, n * 12, 3, first=n // 2)
    assert n // 2 <= s[0] and s[-1] < n and len(s) == 256
    assert len(bench.sample_rows(100_000, 100_000 * 12, 4)) == bench.DUMP_BUDGET // (100_000 * 12)


def test_dump_outputs_writes_float_arrays(tmp_path, monkeypatch):
    a = _args(monkeypatch, "--dump-outputs", str(tmp_path / "out"))
    lat = np.array([[5_000_000, 2**40 + 1]], np.uint64)
    bench.dump_outputs(a, {"latency_ns": lat, "packet_loss": np.array([0.25], np.float32)})
    got = np.load(tmp_path / "out" / "latency_ns.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint64), lat)  # exact below 2^53
    assert np.load(tmp_path / "out" / "packet_loss.npy").dtype == np.float32


@pytest.mark.gpu
def test_plain_run_line_and_dump_match_oracle(tmp_path):
    """One plain run (a 300-node complete graph): the result line's fields, nulls
    where --full would measure, and the dumped table bit-exact vs the oracle."""
    from oracle import oracle as O
    from shadow_amd import synth

    n, seed = 300, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "c2", "--nodes", str(n), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and len(d["config"]["step_ms"]) == 2 and d["ms_per_step"] > 0
    assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"]
    assert d["value"] == pytest.approx(n * n / (d["ms_per_step"] / 1e3))
    assert d["cpu_baseline"] is None and d["cpu_baseline_opt"] is None and d["config"]["e2e"] is None
    rows = np.load(tmp_path / "rows.npy")
    lat, loss = np.load(tmp_path / "latency_ns.npy"), np.load(tmp_path / "packet_loss.npy")
    assert lat.dtype == np.float64 and loss.dtype == np.float32 and np.array_equal(rows, np.arange(n))
    nodes = np.arange(n, dtype=np.uint32)
    elat, eloss = O.compute_shortest_paths(O.Graph(False, np.arange(n), *synth.complete_graph(n, seed)), nodes)
    assert np.array_equal(lat.astype(np.uint64), elat)
    assert np.array_equal(loss.view(np.uint32), eloss.view(np.uint32))
    assert np.load(tmp_path / "min_latency_ns.npy")[0] == float(elat.min())
