"""The per-spectrum kernels in front of the search at the sizes where their launch shape changes, against the oracle
(oracle/falcon_oracle.py), bit for bit:
  * `fal_vectorize_rows` at 2, 4, 8 and 16 rows per wave and turn (the path of every job above cus * 256 rows) and at the
    last size of one row per wave;
  * `fal_process_spectra` over three turns of its grid-stride loop, and a deterministic table of its filters' edges;
  * `fal_to_vector_indices` and `fal_rescore_neighbors` over more than two turns of their grids;
  * all of it once more in a process under FALCON_DEBUG_POISON=1 (tests/front_poison_worker.py).
The sizes follow from the device's CU count (tests/front_cases.py restates the host rules); the oracle runs on a small library
of spectra, the large cases gather library rows and their expected output the same way."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import front_cases as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def cus():
    return device_cus()


# ---- the checks (also run by tests/front_poison_worker.py) ---------------------------------------------------------------------
def _same_bits(got, want):
    import torch
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    return torch.equal(got.view(view), want.view(view))


def check_vectorize(ctx, cus, chunk, low_dim, width, mode, normalize):
    import torch
    n = fc.vectorize_n(chunk, cus)
    assert fc.vectorize_chunk(n, cus) == chunk, (n, cus)           # the size runs the chunk it names on THIS device
    lib = fc.vec_library()
    order = fc.vec_row_order(n)
    order_d = ctx.to_dev(order, torch.int64)
    got = ctx.vectorize(lib["mz"], lib["intensity"], lib["indptr"], order_d, lib["min_mz"], fc.BIN, lib["n_bins"], low_dim,
                        normalize=normalize, dtype=mode, width=width)
    got = got if isinstance(got, tuple) else (got,)
    want = fc.vec_expected(fc.vec_reference(low_dim, width, normalize), mode)
    assert len(got) == len(want)
    for which, (g, w) in enumerate(zip(got, want)):
        e = torch.from_numpy(w).to(ctx.tdev).index_select(0, order_d)
        assert g.dtype == e.dtype and g.shape == e.shape == (n,) + w.shape[1:]
        if not _same_bits(g, e):
            view = torch.int32 if g.dtype == torch.float32 else torch.int16
            bad = (g.view(view).reshape(n, -1) != e.view(view).reshape(n, -1)).any(1).nonzero()
            row = int(bad[0])
            peaks = int(np.diff(lib["indptr"])[order[row]])
            raise AssertionError(f"output {which} of {mode}: {bad.numel()} of {n} rows differ; first row {row} (row % 16 = "
                                 f"{row % 16}, library row {int(order[row])}, {peaks} peaks)")


def _same_f32(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_prep(ctx, batch, opts, expected, what=""):
    """the assertions of test_gpu_preprocess.py::test_process_spectra_matches_oracle"""
    e_valid, e_ip, e_mz, e_it = expected
    valid, ip, omz, oit = (t.cpu().numpy() for t in ctx.process_spectra(*batch, **opts))
    assert np.array_equal(valid, e_valid), what                    # the same spectra survive
    assert np.array_equal(ip, e_ip), what                          # with the same number of peaks
    assert _same_f32(omz, e_mz), what                              # the same peaks, bit for bit
    assert np.array_equal(np.isnan(oit), np.isnan(e_it)), what
    ok = ~np.isnan(e_it)
    assert _same_f32(oit[ok], e_it[ok]), what                      # intensities bit-identical


def check_edge_table(ctx):
    for c in fc.prep_edge_cases():
        e = fo.process_spectra(*c["batch"], **c["opts"])
        fc.check_edge_counts(c, e)
        check_prep(ctx, c["batch"], c["opts"], e, c["name"])


def check_small_prep(ctx):
    """five spectra: the first call of a context sizes the scratch slots small"""
    pick = np.array([0, 1281, 1280, 5, 1500])                      # random, 130 peaks, 70 peaks, random, rejected
    check_prep(ctx, fc.prep_gather(pick), fc.DEFAULTS_RANK, fc.prep_gather_expected(0, pick), "five spectra")


# ---- 1. vectorize ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk,low_dim,width,mode,normalize", fc.VECTORIZE_CASES)
def test_vectorize_rows_per_wave(ctx, cus, chunk, low_dim, width, mode, normalize):
    check_vectorize(ctx, cus, chunk, low_dim, width, mode, normalize)


# ---- 2. preprocess --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_process_spectra_three_grid_turns(ctx, cus, which):
    n = fc.prep_turns_n(cus)
    assert n > 2 * cus * 64 * 4 and n % 4 == 1
    pick = fc.prep_pick(n)
    e = fc.prep_gather_expected(which, pick)
    assert 0.1 < e[0].mean() < 0.9
    check_prep(ctx, fc.prep_gather(pick), fc.PREP_OPTION_SETS[which], e)


def test_process_spectra_edge_table(ctx):
    check_edge_table(ctx)


# ---- 3. the flat kernels ------------------------------------------------------------------------------------------------------
def test_to_vector_indices_past_two_grid_turns(ctx, cus):
    mz = fc.bin_values(cus)
    assert len(mz) == 2 * cus * 8 * 256 + 77
    n_bins, start, _ = fo.get_dim(fc.MZ_LO, fc.MZ_HI, fc.BIN)
    want = fo.bin_indices(mz, start, fc.BIN)
    assert (want < 0).any() and (want >= n_bins).any() and ((want >= 0) & (want < n_bins)).sum() > len(mz) // 2
    assert np.array_equal(ctx.to_vector_indices(mz, start, fc.BIN).cpu().numpy(), want)


def test_rescore_neighbors_past_two_grid_turns(ctx, cus):
    import torch
    case = fc.rescore_case(cus)
    n, k, turn = case["n"], case["k"], case["turn"]
    assert k == 64 and n == 2 * (turn // 64) + 3 and n * k > 2 * turn
    forced = np.concatenate([v[0] for v in case["slots"].values()])
    assert {turn - 1, turn} <= set(forced.tolist()) and (forced // k == n - 1).any()
    for tol, (pos, nb, _, _) in case["slots"].items():
        pos_d = torch.from_numpy(pos).to(ctx.tdev)
        nb_idx = torch.full((n, k), -1, dtype=torch.int32, device=ctx.tdev)
        nb_idx.view(-1)[pos_d] = torch.from_numpy(nb).to(ctx.tdev)
        for min_matches in (0, 3):
            nb_dist = torch.full((n, k), float("inf"), dtype=torch.float32, device=ctx.tdev)
            out = ctx.rescore_neighbors(nb_idx, nb_dist, case["mz"], case["intensity"], case["indptr"], case["order"], tol,
                                        min_matches)
            got = out.view(-1)[pos_d].cpu().numpy()
            want = fc.rescore_expected(case, tol, min_matches)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tol, min_matches, int((got != want).sum()))
            assert int(torch.isinf(out).sum()) == n * k - len(pos)                  # every other slot is still +inf


# ---- 4. scratch hygiene ---------------------------------------------------------------------------------------------------------
def test_front_kernels_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 (scratch filled with 0xFF before use, a slot that grows while a pointer into it is held fails) is
    read once per process: a fresh child runs a five-spectrum batch, the edge table, a 20,000-peak spectrum, the chunk-2
    vectorize case in two output modes and the rescore golden case on one context"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "front_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
