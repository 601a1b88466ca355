"""Assigning new spectra to representatives on the GPU (`fal_assign_nearest`, `cluster.assign_to_library`, `--assign_to`):
every output is compared with the numpy restatement `assign_cases.assign_ref` by `np.array_equal` -- bits, not tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import assign_cases as ac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def run(ctx, q, l, tol, mode, rt_tol, fragment_tol, min_matches):
    out = ctx.assign_nearest(q["mz"], q["intensity"], q["indptr"], q["precursor_mz"], q["retention_time"], l["mz"], l["intensity"],
                             l["indptr"], l["precursor_mz"], l["retention_time"], tol, mode, rt_tol, fragment_tol, min_matches)
    return tuple(t.cpu().numpy() for t in out)


def check(ctx, q, l, tol, mode, rt_tol, fragment_tol, min_matches, ref=None):
    ref = ref if ref is not None else ac.assign_ref(q, l, tol, mode, rt_tol, fragment_tol, min_matches)
    got = run(ctx, q, l, tol, mode, rt_tol, fragment_tol, min_matches)
    for name, g, r in zip(("best_row", "best_dist", "n_cand"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, name
        bad = np.flatnonzero(g.view(np.int32) != r.view(np.int32)) if g.dtype == np.float32 else np.flatnonzero(g != r)
        assert len(bad) == 0, (name, len(bad), bad[:5], g[bad[:5]], r[bad[:5]])
    return got


# ---- template data: the solver path must be on the winners' side ---------------------------------------------------------
_template = {}


def template(name):
    """(queries, library, reference, stats) of one parameter set, computed once"""
    if "split" not in _template:
        _template["split"] = ac.template_split()
    if name not in _template:
        q, l = _template["split"]
        st = {}
        _template[name] = (q, l, ac.assign_ref(q, l, *ac.TEMPLATE_PARAMS[name], stats=st), st)
    return _template[name]


@pytest.mark.parametrize("name", list(ac.TEMPLATE_PARAMS))
def test_template_spectra_equal_the_restatement(ctx, name):
    q, l, ref, st = template(name)
    assert len(q["precursor_mz"]) == 236 and len(l["precursor_mz"]) == 236
    # asserted from the inputs: the solver path cannot silently go untested
    assert st["solver_pairs"] >= 100, st
    assert st["solver_winners"] >= 10 and st["max_component"] <= 32, st
    assert (ref[1] <= np.float32(0.1)).sum() >= 50 and (ref[1] == 1).sum() >= 1
    check(ctx, q, l, *ac.TEMPLATE_PARAMS[name], ref=ref)
    assert ctx.counter(9) == st["solver_pairs"]


def test_assign_to_library_applies_dbscans_comparison(ctx):
    from falcon_amd.cluster.cluster import ClusterPipeline, SpectrumDataset, assign_to_library
    q, l, ref, _ = template("ppm20")
    ds = lambda d: SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
    tol, mode, rt_tol, ft, mm = ac.TEMPLATE_PARAMS["ppm20"]
    eps = float(ref[1][np.argsort(ref[1])[100]])             # a distance that occurs: <= must include it
    row, dist, cand, assigned = assign_to_library(ds(q), ds(l), eps, tol, mode, rt_tol, ft, mm, pipeline=ClusterPipeline(ctx))
    assert np.array_equal(row, ref[0]) and np.array_equal(dist.view(np.int32), ref[1].view(np.int32)) and np.array_equal(cand, ref[2])
    assert assigned.dtype == bool and np.array_equal(assigned, (ref[0] >= 0) & (ref[1] <= np.float32(eps)))
    assert assigned[ref[1] == np.float32(eps)].all() and 90 <= assigned.sum() <= 236


# ---- tile and window edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", [1, 64, 65, 200])
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 130])
def test_tile_and_window_edges(ctx, nq, nl):
    q, l = ac.ladder_case(nq, nl)
    got = check(ctx, q, l, 20.0, "ppm", None, 0.05, 0)
    if nq >= 7 and nl >= 64:
        # queries 0 / 1 lie outside every window; 2..5 sit on the +- 1 ulp bounds of a rung: outside, inside, inside, outside
        assert got[2][0] == 0 and got[2][1] == 0 and got[0][0] == -1 and got[1][0] == 1.0
        lo_out, lo_in, hi_in, hi_out = (ac.take(q, [k]) for k in (2, 3, 4, 5))
        rung = ac.take(l, [int(np.argsort(l["precursor_mz"], kind="stable")[nl // 2])])
        cand = [run(ctx, x, rung, 20.0, "ppm", None, 0.05, 0)[2][0] for x in (lo_out, lo_in, hi_in, hi_out)]
        assert cand == [0, 1, 1, 0]


@pytest.mark.parametrize("mode,tol", [("Da", 0.01), ("ppm", 20.0)])
def test_ulp_bounds_both_modes_and_rt(ctx, mode, tol):
    q, l = ac.ladder_case(65, 130, seed=1, tol=tol, mode=mode)
    check(ctx, q, l, tol, mode, None, 0.05, 0)
    check(ctx, q, l, tol, mode, 25.0, 0.05, 2)


def test_empty_library_and_no_queries(ctx):
    q, l = ac.ladder_case(70, 0)
    row, dist, cand = check(ctx, q, l, 20.0, "ppm", None, 0.05, 0)
    assert (row == -1).all() and (dist == 1.0).all() and (cand == 0).all()
    q0, l0 = ac.ladder_case(0, 70)
    row, dist, cand = run(ctx, q0, l0, 20.0, "ppm", None, 0.05, 0)
    assert row.shape == dist.shape == cand.shape == (0,)


def test_spectra_without_peaks_score_one(ctx):
    q, l = ac.ladder_case(10, 64)
    e = np.zeros(0, np.float32)
    q2 = ac.concat(q, ac.side([e], [e], [l["precursor_mz"][3]]))
    l2 = ac.concat(l, ac.side([e], [e], [q["precursor_mz"][8]]))
    row, dist, cand = check(ctx, q2, l2, 20.0, "ppm", None, 0.05, 0)
    assert dist[-1] == 1.0 and cand[-1] >= 1 and row[-1] >= 0           # d = 1 is still a candidate


def test_wide_tolerances_take_the_whole_library(ctx):
    q, l = ac.ladder_case(65, 200)
    check(ctx, q, l, 2e6, "ppm", None, 0.05, 0)                           # no bounded range: every row is walked
    check(ctx, q, l, 5.0, "Da", None, 0.05, 0)


# ---- ties -------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_precursor_then_the_lowest_row(ctx):
    q, l = ac.tie_case()
    ref = ac.assign_ref(q, l, 20.0, "ppm", None, 0.05, 0)
    assert (ref[1] < 1e-6).all() and (ref[2] == 3).all()
    for s in range(20):                                                   # the rule's pick, spelled out
        same = np.flatnonzero([np.array_equal(ac.peaks(l, r)[0], ac.peaks(q, s)[0]) for r in range(60)])
        assert len(same) == 3
        pm = l["precursor_mz"][same]
        assert ref[0][s] == same[pm == pm.min()].min()
    check(ctx, q, l, 20.0, "ppm", None, 0.05, 0, ref=ref)


# ---- LDS overflow -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_peaks,l_peaks", [(120, 120), (120, 40), (40, 120)])
def test_sides_beyond_the_staged_peaks_are_read_from_global_memory(ctx, q_peaks, l_peaks):
    q, l = ac.overflow_case(q_peaks, l_peaks)
    assert (q["indptr"][-1] > 3200) == (q_peaks == 120) and (l["indptr"][-1] > 3200) == (l_peaks == 120)
    row, dist, cand = check(ctx, q, l, 20.0, "ppm", None, 0.05, 0)
    assert (cand == 64).all() and (dist < 0.5).sum() >= 32


# ---- unsupported input ------------------------------------------------------------------------------------------------------
def test_a_component_beyond_the_solver_fails_inside_a_window_only(ctx):
    from falcon_amd._lib import FalconHipError
    q, l, tol = ac.unsupported_case(inside=True)
    with pytest.raises(FalconHipError, match="code -5"):
        run(ctx, q, l, 20.0, "ppm", None, tol, 0)
    q, l, tol = ac.unsupported_case(inside=False)
    row, dist, cand = check(ctx, q, l, 20.0, "ppm", None, tol, 0)
    assert cand[-1] == 0 and row[-1] == -1


# ---- debug poison -----------------------------------------------------------------------------------------------------------
def test_template_case_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 is read once per process: a fresh child runs the template case (and a second, larger call on the
    same context) with every scratch block filled with 0xFF before use"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "assign_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- command line -----------------------------------------------------------------------------------------------------------
def _specs(d, charge, prefix):
    return [{"identifier": f"{prefix}{i}", "precursor_mz": float(d["precursor_mz"][i]), "precursor_charge": charge,
             "retention_time": float(d["retention_time"][i]), "mz": ac.peaks(d, i)[0].astype(np.float64),
             "intensity": ac.peaks(d, i)[1]} for i in range(len(d["precursor_mz"]))]


def _csv(path):
    lines = open(path).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    rows = [l.split(",") for l in lines[len(head) + 1:]]
    return head, {r[1]: (r[2], int(r[5])) for r in rows}


def _rep_ids(path):
    from falcon_amd.ms_io import mgf_io
    return {s["identifier"]: s["cluster"] for s in mgf_io.get_library_spectra(path)}


def _expected(work, first_new):
    """labels by identifier from the work directory's partitions: `assign_ref` against the library the run left there, a plain
    generate_clusters call (the run's own parameters: the configuration is still the run's) on the rows that are left"""
    import json
    from falcon_amd import falcon
    from falcon_amd.cluster import cluster
    from falcon_amd.config import config as cfg
    out, current, n_assigned = {}, first_new, 0
    for charge in json.load(open(work / "spectra" / "charges.json")):
        part = dict(np.load(work / "spectra" / f"spectra_charge_{charge}.npz"))
        n = len(part["precursor_mz"])
        labels = np.full(n, -1, np.int64)
        rest = np.arange(n)
        lib_fn = work / "spectra" / f"library_charge_{charge}.npz"
        if lib_fn.exists():
            lib = dict(np.load(lib_fn))
            row, dist, _ = ac.assign_ref(part, lib, cfg.precursor_tol[0], cfg.precursor_tol[1], cfg.rt_tol, cfg.fragment_tol,
                                         cfg.min_matched_peaks)
            assigned = (row >= 0) & (dist <= np.float32(cfg.eps))
            labels[assigned] = lib["cluster"][row[assigned]]
            rest = np.flatnonzero(~assigned)
            n_assigned += int(assigned.sum())
        if len(rest):
            sub = ac.take(part, rest)
            lab, _ = cluster.generate_clusters(
                cluster.SpectrumDataset(sub["precursor_mz"], sub["retention_time"], sub["mz"], sub["intensity"], sub["indptr"]),
                cfg.linkage, cfg.distance_threshold, cfg.min_matched_peaks, cfg.precursor_tol[0], cfg.precursor_tol[1], cfg.rt_tol,
                cfg.fragment_tol, cfg.batch_size, ann=falcon._ann_params())
            labels[rest] = lab + current
            current = int(labels[rest].max()) + 1
        out.update({str(i): int(l) for i, l in zip(part["identifier"], labels)})
    return out, n_assigned


@pytest.mark.parametrize("exact", [False, True], ids=["ann", "exact"])
def test_main_assigns_to_the_representatives_of_an_earlier_run(tmp_path, exact):
    from falcon_amd.falcon import main
    from falcon_amd.ms_io import mgf_io, ms_io
    gen = dict(n_templates=4, per=45, chained=0)
    known = ac.template_spectra(pmz_centres=(500, 640), seed=11, **gen)                  # 90 spectra of 8 templates
    fresh = ac.template_spectra(pmz_centres=(560,), seed=12, **gen)                     # templates run A has not seen
    other = ac.template_spectra(pmz_centres=(700,), seed=13, n_templates=3, per=20, chained=0)     # a charge A does not have
    half = len(known["precursor_mz"]) // 2
    spec_a = _specs(ac.take(known, np.arange(half)), 2, "a")
    spec_b = (_specs(ac.take(known, np.arange(half, 2 * half)), 2, "b") + _specs(fresh, 2, "n") + _specs(other, 3, "z"))
    a_mgf, b_mgf = str(tmp_path / "A.mgf"), str(tmp_path / "B.mgf")
    ms_io.write_spectra(a_mgf, spec_a)
    ms_io.write_spectra(b_mgf, spec_b)
    mode = ["--exact"] if exact else []
    opts = ["--eps", "0.4", "--export_representatives"] + mode
    out_a, out_b, out_c, out_p = (str(tmp_path / n) for n in ("outA", "outB", "outC", "outPlain"))
    assert main([a_mgf, out_a, "--work_dir", str(tmp_path / "workA")] + opts) == 0
    a_ids = set(_rep_ids(out_a + ".mgf").values())
    first_new = max(a_ids) + 1
    assert len(a_ids) >= 8 and a_ids == set(v[1] for v in _csv(out_a + ".csv")[1].values())

    work_b = tmp_path / "workB"
    assert main([b_mgf, out_b, "--work_dir", str(work_b), "--assign_to", out_a + ".mgf"] + opts) == 0
    head, got = _csv(out_b + ".csv")
    assert f"# assign_to = {out_a}.mgf" in head
    want, n_assigned = _expected(work_b, first_new)
    assert {k: v[1] for k, v in got.items()} == want
    assert n_assigned >= 30 and len(want) == len(spec_b)
    old = {k: v for k, v in want.items() if v < first_new}
    assert len(old) == n_assigned and set(old.values()) <= a_ids and all(k.startswith("b") for k in old)
    assert all(v >= first_new for k, v in want.items() if k[0] in "nz")                # new templates, and the charge A lacks
    new_ids = {v for v in want.values() if v >= first_new}
    b_reps = _rep_ids(out_b + ".mgf")
    assert set(b_reps.values()) == new_ids and len(b_reps) == len(new_ids)                # out.mgf: exactly the new clusters
    assert all(want[title] == cid for title, cid in b_reps.items())                      # ... represented by a member

    # a third run chains both files: a copy of the representative of one of B's new clusters goes to B's id
    title, cid = next((t, c) for t, c in sorted(b_reps.items()) if t.startswith("n"))
    c_mgf = str(tmp_path / "C.mgf")
    ms_io.write_spectra(c_mgf, [dict(s, identifier="copy") for s in spec_b if s["identifier"] == title])
    assert main([c_mgf, out_c, "--work_dir", str(tmp_path / "workC"), "--assign_to", out_a + ".mgf", out_b + ".mgf"] + opts) == 0
    head_c, got_c = _csv(out_c + ".csv")
    assert f"# assign_to = {out_a}.mgf {out_b}.mgf" in head_c and got_c == {"copy": ("2", cid)}
    assert list(mgf_io.get_spectra(out_c + ".mgf")) == []

    # without the option: no header line, labels from 0
    assert main([b_mgf, out_p, "--work_dir", str(tmp_path / "workP")] + opts) == 0
    head_p, got_p = _csv(out_p + ".csv")
    assert not any("assign_to" in l for l in head_p) and len(head_p) == len(head) - 1
    assert min(v[1] for v in got_p.values()) == 0
