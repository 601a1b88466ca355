"""Member scores and cluster summary on the device (`fal_member_scores`, `fal_cluster_summary`) against the numpy restatement of
tests/memberscore_cases.py: every comparison is on bits.  Template clusters whose pairs mostly take the solver (the context's
counter against the count from the inputs), tile edges, the consensus form (permuted rows, a representative above the LDS
capacity, spectra without peaks, a component beyond the solver), the summary's sizes, the public functions end to end and
`main()` with `--cluster_summary`.

No test forces the fallback list to overflow: `fal_assign_nearest`'s tests have no hook for that either."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import consensus_cases as cc
from tests import memberscore_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def gpu_scores(ctx, case, rep, rep_row, tol):
    sim, matched = ctx.member_scores(case["mz"], case["intensity"], case["indptr"], case["labels"], rep["mz"], rep["intensity"],
                                     rep["indptr"], rep_row, tol)
    return sim, matched


def gpu_summary(ctx, labels, n_clusters, sim, pmz, rt):
    return {k: v.cpu().numpy() for k, v in ctx.cluster_summary(labels, n_clusters, sim, pmz, rt).items()}


def check(ctx, case, rep, rep_row, tol, stats=None):
    """scores and summary of one case on the device == the restatement -> the device's (similarity, matched)"""
    want_sim, want_matched = mc.scores_ref(case, rep, rep_row, tol, stats)
    sim, matched = gpu_scores(ctx, case, rep, rep_row, tol)
    got_sim, got_matched = sim.cpu().numpy(), matched.cpu().numpy()
    assert mc.same(got_matched, want_matched), np.flatnonzero(got_matched != want_matched)[:10]
    assert mc.same(got_sim, want_sim), np.flatnonzero(mc.bits(got_sim) != mc.bits(want_sim))[:10]
    nc = len(rep_row)
    want = mc.summary_ref(case["labels"], nc, want_sim, case["precursor_mz"], case["retention_time"])
    got = gpu_summary(ctx, case["labels"], nc, sim, case["precursor_mz"], case["retention_time"])
    for k in mc.COLUMNS:
        assert mc.same(got[k], want[k]), k
    return got_sim, got_matched


# ---- the solver ----------------------------------------------------------------------------------------------------------------
def check_template(ctx):
    case, tol = mc.template_case()
    assert len(case["labels"]) <= 300
    stats = {}
    check(ctx, case, *mc.medoid_form(case), tol, stats)
    assert stats["solver_pairs"] >= 100 and stats["max_component"] <= 32, stats
    assert ctx.counter(9) == stats["solver_pairs"]
    return stats


def test_template_clusters_take_the_solver_and_the_counter_counts_them(ctx):
    check_template(ctx)


def test_pairs_of_every_component_size(ctx):
    case, tol = mc.solver_pairs_case()
    stats = {}
    check(ctx, case, *mc.medoid_form(case), tol, stats)
    assert stats["solver_pairs"] >= 60 and 16 <= stats["max_component"] <= 32, stats
    assert ctx.counter(9) == stats["solver_pairs"]


# ---- tile edges ----------------------------------------------------------------------------------------------------------------
TILE_CASES = [(n, layout) for n in mc.TILE_SIZES for layout in mc.tile_layouts(n)]


@pytest.mark.parametrize("n,layout", TILE_CASES, ids=[f"{n}-{l}" for n, l in TILE_CASES])
def test_tile_edges(ctx, n, layout):
    case, tol = mc.tile_case(n, layout)
    assert len(case["labels"]) == n
    if layout == "straddle":
        assert np.sort(case["labels"])[63] == 1 and np.sort(case["labels"])[62] == 0 and np.sum(case["labels"] == 1) == 65
    if layout == "interleaved":
        assert (np.diff(case["labels"]) < 0).any()            # the (label, row) order is not the row order
    check(ctx, case, *mc.medoid_form(case), tol)


def test_labels_outside_the_clusters_score_zero(ctx):
    case, tol = mc.tile_case(130, "interleaved")
    case = dict(case, labels=case["labels"].copy())
    case["labels"][[5, 77]] = [-1, 9]
    rep, rep_row = mc.medoid_form(case)
    sim, matched = check(ctx, case, rep, rep_row, tol)
    assert not sim[[5, 77]].any() and not matched[[5, 77]].any()


# ---- consensus form --------------------------------------------------------------------------------------------------------------
def test_consensus_form_and_permuted_representative_rows(ctx):
    case, tol = mc.tile_case(130, "interleaved", seed=3)
    rep, rep_row = mc.consensus_rep(case, tol)
    assert np.array_equal(rep_row, np.arange(3))
    a = check(ctx, case, rep, rep_row, tol)
    rep2, rep_row2 = mc.permute_rep(rep, rep_row, np.random.default_rng(5))
    assert not np.array_equal(rep_row2, rep_row)
    b = check(ctx, case, rep2, rep_row2, tol)
    assert mc.same(a[0], b[0]) and mc.same(a[1], b[1])
    case, tol = mc.solver_pairs_case(n_pairs=30, seed=12)
    check(ctx, case, *mc.consensus_rep(case, tol), tol)


def test_sides_above_the_lds_capacity_and_spectra_without_peaks(ctx):
    case, rep, rep_row, tol = mc.big_rep_case()
    assert np.diff(rep["indptr"]).tolist()[1:] == [4000, 0] and np.diff(case["indptr"])[:64].sum() > 3200
    assert (np.diff(case["indptr"]) == 0).any()
    sim, matched = check(ctx, case, rep, rep_row, tol)
    assert not sim[case["labels"] == 2].any() and not matched[case["labels"] == 2].any()
    assert sim[case["labels"] == 1].any()
    # a rep_row outside the representative CSR is a representative without peaks
    sim, _ = gpu_scores(ctx, case, rep, np.array([0, 7, -1], np.int32), tol)
    assert not sim.cpu().numpy()[case["labels"] != 0].any()


def test_a_component_beyond_the_solver_is_an_error_and_the_context_stays_usable(ctx):
    from falcon_amd._lib import FalconHipError
    case, tol = mc.unsupported_case()
    with pytest.raises(FalconHipError, match="more than 32 peaks"):
        gpu_scores(ctx, case, *mc.medoid_form(case), tol)
    case, tol = mc.tile_case(65, "interleaved")
    check(ctx, case, *mc.medoid_form(case), tol)


# ---- summary -----------------------------------------------------------------------------------------------------------------------
def test_summary_sizes_on_the_device(ctx):
    labels, sim, pmz, rt = mc.summary_case(mc.SUMMARY_SIZES, seed=4)
    want = mc.summary_ref(labels, len(mc.SUMMARY_SIZES), sim, pmz, rt)
    got = gpu_summary(ctx, labels, len(mc.SUMMARY_SIZES), sim, pmz, rt)
    for k in mc.COLUMNS:
        assert mc.same(got[k], want[k]), k
    got = gpu_summary(ctx, labels, len(mc.SUMMARY_SIZES), sim, pmz, None)
    want = mc.summary_ref(labels, len(mc.SUMMARY_SIZES), sim, pmz, None)
    for k in mc.COLUMNS:
        assert mc.same(got[k], want[k]), k


def test_a_large_cluster_beside_singletons(ctx):
    """5,000 members beside 3,000 singletons, rows interleaved: the large cluster's bits are those of the stated order"""
    labels, sim, pmz, rt = mc.summary_case([5000] + [1] * 3000, seed=9)
    want = mc.summary_ref(labels, 3001, sim, pmz, rt)
    got = gpu_summary(ctx, labels, 3001, sim, pmz, rt)
    for k in mc.COLUMNS:
        assert mc.same(got[k], want[k]), k
    alone = mc.summary_case([5000], seed=9, interleave=False)
    assert want["size"][0] == 5000 and gpu_summary(ctx, *alone[:1], 1, *alone[1:])["size"][0] == 5000


# ---- the public functions, end to end ----------------------------------------------------------------------------------------------
def test_generate_clusters_then_scores_and_summary(ctx):
    from falcon_amd import synth
    from falcon_amd.cluster import cluster as fc
    from oracle.falcon_oracle import cosine_fast
    d = synth.select_charge(synth.generate(4000, seed=5), 2)
    ds = fc.SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
    pipe = fc.ClusterPipeline(ctx)
    labels, medoids = fc.generate_clusters(ds, "complete", 0.1, 0, 20.0, "ppm", None, 0.05, 2 ** 15, pipeline=pipe)
    case = dict(mz=d["mz"], intensity=d["intensity"], indptr=d["indptr"], labels=labels, medoids=medoids,
                precursor_mz=d["precursor_mz"], retention_time=d["retention_time"])
    assert np.bincount(labels).max() >= 3
    cons = fc.consensus_spectra(ds, labels, medoids, 0.05, pipeline=pipe)[:3]
    for consensus in (None, cons):
        if consensus is None:
            rep, rep_row = mc.medoid_form(case)
        else:
            rep, rep_row = dict(indptr=cons[0], mz=cons[1], intensity=cons[2]), np.arange(len(medoids), dtype=np.int32)
        want = mc.scores_ref(case, rep, rep_row, 0.05)
        sim, matched = fc.member_scores(ds, labels, medoids, 0.05, consensus=consensus, pipeline=pipe)
        assert mc.same(sim, want[0]) and mc.same(matched, want[1])
        out = fc.cluster_summary(ds.to_device(ctx.tdev), labels, medoids, 0.05, consensus=consensus, pipeline=pipe)
        ref = mc.summary_ref(labels, len(medoids), want[0], d["precursor_mz"], d["retention_time"])
        for k in mc.COLUMNS:
            assert mc.same(out[k], ref[k]), k
        assert mc.same(out["similarity"], want[0]) and mc.same(out["matched"], want[1])
        if consensus is None:                                  # a medoid is scored against itself like any other pair
            own = np.array([cosine_fast(*mc.peaks(case, m), *mc.peaks(case, m), 0.05)[0] for m in medoids], np.float32)
            assert mc.same(sim[medoids], own)


# ---- main() ------------------------------------------------------------------------------------------------------------------------
def _write_input(path):
    """spectra of tests/peakfile_writer.py, each with up to four noisy copies (clusters of 1 .. 5) -> the MGF file"""
    from falcon_amd.ms_io import ms_io
    from tests import peakfile_writer as pw
    rng = np.random.default_rng(8)
    specs = []
    for s in pw.synthetic_spectra(80, seed=8):
        specs.append(s)
        for _ in range(int(rng.integers(0, 5))):
            specs.append(dict(s, identifier=f"scan={1000 + len(specs)}", precursor_mz=s["precursor_mz"] * (1.0 + rng.normal(0, 1e-6)),
                              intensity=(s["intensity"] * rng.uniform(0.6, 1.4, len(s["intensity"]))).astype(np.float32)))
    ms_io.write_spectra(path, specs)


def _expected_files(out, work, consensus):
    """the two files' text from the run's own partitions, the cluster CSV's labels and the exported representatives' titles"""
    from falcon_amd.ms_io import summary_io
    lines = open(out + ".csv", newline="").read().split("\n")
    header = [l[2:] for l in lines if l.startswith("# ")]
    rows = [l.split(",") for l in lines if l and not l.startswith("#")][1:]
    cluster_of = {r[1]: int(r[5]) for r in rows}
    title_of = {}
    for entry in open(out + ".mgf").read().split("BEGIN IONS")[1:]:
        fields = dict(l.split("=", 1) for l in entry.splitlines() if "=" in l and not l[0].isdigit())
        title_of[int(fields["CLUSTER"])] = fields["TITLE"]
    blocks = []
    for charge in json.load(open(os.path.join(work, "spectra", "charges.json"))):
        z = np.load(os.path.join(work, "spectra", f"spectra_charge_{charge}.npz"))
        glob = np.array([cluster_of[str(i)] for i in z["identifier"]], np.int64)
        first = int(glob.min())
        labels = (glob - first).astype(np.int32)
        row_of = {str(t): i for i, t in enumerate(z["identifier"])}
        medoids = np.array([row_of[title_of[c + first]] for c in range(int(labels.max()) + 1)], np.int32)
        case = dict(mz=z["mz"], intensity=z["intensity"], indptr=z["indptr"], labels=labels, medoids=medoids)
        rep, rep_row = mc.consensus_rep(case, 0.05) if consensus else mc.medoid_form(case)
        sim, matched = mc.scores_ref(case, rep, rep_row, 0.05)
        cols = mc.summary_ref(labels, len(medoids), sim, z["precursor_mz"], z["retention_time"])
        cols.update(charge=charge, cluster=np.arange(len(medoids)) + first, labels=glob, filename=z["filename"],
                    identifier=z["identifier"], medoids=medoids, similarity=sim, matched=matched)
        blocks.append((first, cols))
    blocks = [b for _, b in sorted(blocks, key=lambda x: x[0])]
    a, b = io.StringIO(newline=""), io.StringIO(newline="")
    summary_io.write_clusters(a, header, blocks)
    summary_io.write_scores(b, header, blocks)
    return a.getvalue(), b.getvalue(), blocks


@pytest.mark.parametrize("mode", [[], ["--exact"], ["--representatives", "consensus"]], ids=["default", "exact", "consensus"])
def test_main_writes_the_cluster_summary(tmp_path, mode):
    from falcon_amd.falcon import main
    mgf, work = str(tmp_path / "in.mgf"), str(tmp_path / "work")
    _write_input(mgf)
    plain, full = str(tmp_path / "plain"), str(tmp_path / "full")
    common = ["--eps", "0.3", "--export_representatives", "--work_dir", work] + mode
    assert main([mgf, plain] + common) == 0
    assert main([mgf, full] + common + ["--cluster_summary"]) == 0
    for ext in (".csv", ".mgf"):
        assert open(plain + ext, "rb").read() == open(full + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".clusters.csv") and not os.path.exists(plain + ".scores.csv")
    clusters, scores, blocks = _expected_files(full, work, consensus="consensus" in mode)
    assert sum(len(b["cluster"]) for b in blocks) >= 60 and max(int(b["size"].max()) for b in blocks) >= 3
    assert open(full + ".clusters.csv", newline="").read() == clusters
    assert open(full + ".scores.csv", newline="").read() == scores
    assert main([mgf, full] + common + ["--cluster_summary"]) == 1          # the files are there: refused without --overwrite


# ---- scratch hygiene -------------------------------------------------------------------------------------------------------------
def test_template_case_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 (scratch filled with 0xFF before use, a slot that grows while a pointer into it is held fails) is
    read once per process: a fresh child runs the template case, a tile case and the summary's sizes again"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "memberscore_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
