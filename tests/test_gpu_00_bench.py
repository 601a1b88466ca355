"""A plain `bench.py --gpus 1` run: the headline line only, and --dump-outputs writes the same outputs on every run.

The benchmark runs in fresh child processes; this file creates no GPU context in the pytest process (it sorts in front of
tests/test_gpu_00_world2.py, which needs that too)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SPECTRA = 100_000


def _plain_run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--spectra", str(N_SPECTRA), "--dump-outputs", str(out_dir)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_its_outputs_repeat(tmp_path):
    outs = []
    for k, steps in enumerate((3, 2)):
        line = _plain_run(tmp_path / str(k), steps)
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == steps and line["warmup"] == 1 and line["unit"] == "spectra/s" and line["higher_is_better"] is True
        assert abs(line["value"] - N_SPECTRA * 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
        for key in ("roofline", "stage_ms", "configs", "cpu_baseline", "cold_pass", "value_host_to_host"):
            assert key not in line, key                                  # --full measurements
        assert line["outputs"] == {"labels": {"n": N_SPECTRA, "sampled": False},
                                   "medoids": {"n": line["outputs"]["medoids"]["n"], "sampled": False}}
        labels = np.load(tmp_path / str(k) / "labels.npy")
        medoids = np.load(tmp_path / str(k) / "medoids.npy")
        assert labels.dtype == medoids.dtype == np.float64 and len(labels) == N_SPECTRA
        assert np.array_equal(labels[medoids.astype(np.int64)], np.arange(len(medoids)))    # one medoid per cluster, in order
        assert (np.bincount(labels.astype(np.int64)) > 1).sum() > 20                     # a non-trivial clustering
        outs.append((labels, medoids))
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))                 # same inputs -> same outputs
