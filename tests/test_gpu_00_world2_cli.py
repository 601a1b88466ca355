"""The CLI on two ranks, and on one (`--distributed` under `python -m torch.distributed.run --module falcon_amd.falcon`, gloo, both ranks on
GPU 0 through the FALCON_DIST_* hooks) against the one-process CLI: same header, same table except the cluster ids, which
are rank-major but give the same partition, and the same representatives -- in exact mode and on the default
nearest-neighbour path.  One rank is a job of its own (the first point of a scaling run): its table equals the
one-process table, cluster ids included.

This file sorts next to test_gpu_00_world2.py on purpose: the pytest process must not own a GPU context when it starts the
launcher.  Both runs are fresh subprocesses; the test itself creates no context."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _mgf(path):
    """two precursor charges, several buckets each"""
    from falcon_amd.ms_io import ms_io
    from tests.test_gpu_exact import _spectra
    specs = []
    for charge, seed, centres in ((2, 5, [450.0, 451.5, 500.0, 620.0, 800.0]), (3, 6, [430.2, 555.0, 556.3, 910.0])):
        d = _spectra(4, 50, centres, seed=seed, jitter=0.005, n_peaks=30)
        for i in range(len(d["precursor_mz"])):
            a, b = d["indptr"][i], d["indptr"][i + 1]
            specs.append({"identifier": f"scan={charge}{i:04d}", "precursor_mz": float(d["precursor_mz"][i]),
                          "precursor_charge": charge, "retention_time": float(d["retention_time"][i]),
                          "mz": d["mz"][a:b].astype(np.float64), "intensity": d["intensity"][a:b]})
    ms_io.write_spectra(path, specs)


def _run(cmd, env, what):
    proc = subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        log, _ = proc.communicate(timeout=600)
    except subprocess.TimeoutExpired:
        proc.kill()
        log, _ = proc.communicate()
        pytest.fail(f"{what} timed out:\n" + log[-3000:])
    assert proc.returncode == 0, f"{what} failed:\n" + log[-3000:]


def _read_csv(path):
    lines = open(path).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    body = [l for l in lines if not l.startswith("#")]
    import csv
    rows = list(csv.reader(body))
    return head, rows[0], rows[1:]


EXACT = ["--exact", "--linkage", "complete"]


@pytest.mark.parametrize("mode,ranks", [(EXACT, 2), ([], 2), (EXACT, 1)], ids=["exact", "ann", "exact-one-rank"])
def test_cli_on_n_ranks_equals_one_process(tmp_path, mode, ranks):
    import torch
    if torch.cuda.is_initialized():
        pytest.fail("this pytest process already owns a GPU context (a GPU test file sorted in front of this one?): "
                    "tests/test_gpu_00_world2_cli.py must run before the in-process GPU tests")
    mgf = str(tmp_path / "in.mgf")
    _mgf(mgf)
    work = str(tmp_path / "work")
    common = [mgf, "--work_dir", work, "--overwrite", "--export_representatives", "--eps", "0.35",
              "--min_matched_peaks", "2"] + mode
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    _run([sys.executable, "-m", "falcon_amd.falcon", *common[:1], one, *common[1:]], env, "one-process CLI")
    denv = dict(env, FALCON_DIST_BACKEND="gloo", FALCON_DIST_DEVICE="0")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), "--module", "falcon_amd.falcon", *common[:1], two, *common[1:], "--distributed"],
         denv, f"{ranks}-rank CLI")
    h1, c1, r1 = _read_csv(one + ".csv")
    h2, c2, r2 = _read_csv(two + ".csv")
    assert h1 == h2 and c1 == c2                                               # --distributed is not in the header
    assert len(r1) == len(r2) > 400
    assert [r[:5] for r in r1] == [r[:5] for r in r2]
    a, b = np.array([int(r[5]) for r in r1]), np.array([int(r[5]) for r in r2])
    pairs = np.unique(np.stack([a, b]), axis=1)
    assert pairs.shape[1] == len(np.unique(a)) == len(np.unique(b))         # the same partition
    if ranks == 1:
        assert np.array_equal(a, b)                                            # one rank: the one-process ids
    assert (np.bincount(a) > 1).sum() > 10                                     # a non-trivial clustering
    from falcon_amd.ms_io import ms_io
    reps1 = {s["identifier"] for s in ms_io.get_spectra(one + ".mgf")}
    reps2 = {s["identifier"] for s in ms_io.get_spectra(two + ".mgf")}
    assert reps1 == reps2 and len(reps1) == len(np.unique(a))
