"""bench.py's command line and its --dump-outputs writer, without a GPU."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_writes_float64_exactly_when_they_fit(tmp_path):
    labels = np.array([0, 1, 1, 2, -1, 123456789], np.int64)
    medoids = np.array([0, 1, 3], np.int64)
    got = bench.dump_outputs(str(tmp_path), {"labels": labels, "medoids": medoids})
    assert got == {"labels": {"n": 6, "sampled": False}, "medoids": {"n": 3, "sampled": False}}
    assert sorted(os.listdir(tmp_path)) == ["labels.npy", "medoids.npy"]
    for name, a in (("labels", labels), ("medoids", medoids)):
        b = np.load(tmp_path / f"{name}.npy")
        assert b.dtype == np.float64 and np.array_equal(b, a)


def test_dump_outputs_samples_the_same_elements_within_the_budget(tmp_path):
    budget = 40_000
    arrays = {"labels": np.arange(50_000) * 3, "medoids": np.arange(100)}
    runs = []
    for k in range(2):
        d = str(tmp_path / str(k))
        got = bench.dump_outputs(d, arrays, budget=budget)
        assert got["labels"]["sampled"] and got["labels"]["kept"] == budget // 32 and not got["medoids"]["sampled"]
        assert _sizes(d) <= budget + 4 * 128                     # + the npy headers
        idx = np.load(os.path.join(d, "labels_index.npy"))
        val = np.load(os.path.join(d, "labels.npy"))
        assert np.all(np.diff(idx) > 0) and np.array_equal(val, idx * 3)
        assert np.array_equal(np.load(os.path.join(d, "medoids.npy")), arrays["medoids"])
        runs.append(idx)
    assert np.array_equal(runs[0], runs[1])                      # a fixed, seeded sample


def test_the_default_budget_is_below_64_mb():
    assert bench.DUMP_BUDGET_BYTES + 16 * 128 < 64_000_000


def test_with_strong_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--with-strong"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr
