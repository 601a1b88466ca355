"""`--representatives consensus` under `--distributed` on two gloo ranks (both on GPU 0 through the FALCON_DIST_* hooks) against
the one-process CLI: rank 0 computes the consensus after the gather, so the representatives, keyed by TITLE, carry the same
peaks.  (Cluster ids are rank-major there: CLUSTER= is not compared.)

This file sorts next to test_gpu_00_world2_cli.py on purpose: the pytest process must not own a GPU context when it starts the
launcher.  Both runs are fresh subprocesses; the test itself creates no context."""
import os
import sys

import pytest

from tests.test_gpu_00_world2_cli import ROOT, _free_port, _mgf, _read_csv, _run

pytestmark = pytest.mark.gpu


def _by_title(path):
    out, title, peaks = {}, None, None
    for line in open(path).read().splitlines():
        if line == "BEGIN IONS":
            title, peaks = None, []
        elif line.startswith("TITLE="):
            title = line[6:]
        elif line == "END IONS":
            out[title] = peaks
        elif line and "=" not in line and peaks is not None:
            peaks.append(line)
    return out


def test_consensus_representatives_on_two_ranks_equal_one_process(tmp_path):
    import torch
    if torch.cuda.is_initialized():
        pytest.fail("this pytest process already owns a GPU context: tests/test_gpu_00_world2_consensus.py must run before the "
                    "in-process GPU tests")
    mgf = str(tmp_path / "in.mgf")
    _mgf(mgf)
    work = str(tmp_path / "work")
    common = [mgf, "--work_dir", work, "--overwrite", "--export_representatives", "--eps", "0.35", "--min_matched_peaks", "2",
              "--representatives", "consensus"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    med, one, two = str(tmp_path / "med"), str(tmp_path / "one"), str(tmp_path / "two")
    _run([sys.executable, "-m", "falcon_amd.falcon", mgf, med, *common[1:-2]], env, "one-process CLI, medoids")
    _run([sys.executable, "-m", "falcon_amd.falcon", mgf, one, *common[1:]], env, "one-process CLI, consensus")
    denv = dict(env, FALCON_DIST_BACKEND="gloo", FALCON_DIST_DEVICE="0")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), "--module", "falcon_amd.falcon", mgf, two, *common[1:], "--distributed"],
         denv, "2-rank CLI, consensus")
    h1, _, r1 = _read_csv(one + ".csv")
    h2, _, r2 = _read_csv(two + ".csv")
    assert h1 == h2 and "# representatives = consensus" in h1 and [r[:5] for r in r1] == [r[:5] for r in r2]
    a, b, m = _by_title(one + ".mgf"), _by_title(two + ".mgf"), _by_title(med + ".mgf")
    assert set(a) == set(b) == set(m) and len(a) > 20
    assert a == b                                                       # the same peaks per representative
    assert sum(a[t] != m[t] for t in a) > 10                            # and they are merged peaks, not the medoids'
