"""Annotation propagation on the device (`fal_network_propagate`) against the numpy restatement of tests/propagate_cases.py: every
comparison is on bits, every "at least" is asserted on the restatement's statistics (propagate_cases.expected does that before it
hands a result out).  Chains (the same-launch cascade), ties, levels against scores, link oddities, degenerate inputs, stars, wave
and block boundaries, random graphs with and without the early-out, link order and duplicates, every refused input, counter 15,
the public function and `main()` with `--library_propagate`."""
import csv
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import propagate_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32 = np.float32, np.int32
MARK = -7


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def gpu_propagate(ctx, g, seed, max_hops, min_score):
    source, hops, parent, score, n_reached, n_levels = ctx.network_propagate(g["u"], g["v"], g["sim"], g["n"], seed, max_hops, min_score)
    return dict(source=source.cpu().numpy(), hops=hops.cpu().numpy(), parent=parent.cpu().numpy(), score=score.cpu().numpy(),
                n_reached=n_reached, n_levels=n_levels)


def check_case(ctx, name):
    """the device == the restatement, counter 15 included"""
    g, seed, max_hops, min_score, _ = pc.CASES[name]
    want = pc.expected(name)
    got = gpu_propagate(ctx, g, seed, max_hops, min_score)
    print(name, got["n_reached"], got["n_levels"], "restatement:", want["n_reached"], want["n_levels"], "tied", want["tied"],
          want["tied_sources"])
    assert pc.same(got, want), (name, got["n_reached"], want["n_reached"], got["n_levels"], want["n_levels"],
                                {k: int((got[k].view(i32) != want[k].view(i32)).sum()) for k in pc.ARRAYS if got[k].shape == want[k].shape})
    assert ctx.counter(15) == want["n_reached"], (name, ctx.counter(15))
    return got


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_the_device_is_the_restatement(ctx, name):
    check_case(ctx, name)


def test_link_shuffles_with_duplicates_change_nothing(ctx):
    for name in ("random-300", "random-5000-min-0.6", "hub-of-seeds-300", "min-score-detour"):
        g, seed, max_hops, min_score, _ = pc.CASES[name]
        want = pc.expected(name)
        for s in (7, 8):
            h = pc.shuffled(g, seed=s, duplicates=min(40, len(g["u"])))
            assert pc.same(gpu_propagate(ctx, h, seed, max_hops, min_score), want), (name, s)


def raw_call(ctx, g, seed, max_hops, min_score):
    """the C entry point with marked outputs -> (rc, outputs on the host, n_reached, n_levels)"""
    import torch
    u, v, sim = ctx.to_dev(g["u"], torch.int32), ctx.to_dev(g["v"], torch.int32), ctx.to_dev(g["sim"], torch.float32)
    n, m = g["n"], len(g["u"])
    sd = ctx.to_dev(np.ascontiguousarray(seed, i32) if n else np.zeros(1, i32), torch.int32)
    out = [ctx.empty((max(n, 1),), t) for t in (torch.int32, torch.int32, torch.int32, torch.float32)]
    for t in out:
        t.fill_(MARK)
    nr, nl = C.c_int64(MARK), C.c_int64(MARK)
    ptr = lambda t: ctx._p(t if t.numel() else None)
    rc = ctx.lib.fal_network_propagate(ctx._h, ptr(u), ptr(v), ptr(sim), m, n, ctx._p(sd), int(max_hops), float(min_score),
                                       *(ctx._p(t) for t in out), C.byref(nr), C.byref(nl))
    ctx.sync()
    return rc, [t.cpu().numpy() for t in out], nr.value, nl.value


@pytest.mark.parametrize("name", sorted(pc.invalid_cases()))
def test_a_refused_input_writes_nothing_and_the_context_stays_usable(ctx, name):
    g, seed, max_hops, min_score = pc.invalid_cases()[name]
    assert not pc.valid(g["n"], g["u"], g["v"], g["sim"], seed, max_hops, min_score)
    rc, out, nr, nl = raw_call(ctx, g, seed, max_hops, min_score)
    assert rc == -1 and all((o == MARK).all() for o in out) and (nr, nl) == (MARK, MARK), (rc, nr, nl)      # FAL_EINVAL
    from falcon_amd._lib import FalconHipError
    with pytest.raises(FalconHipError, match="code -1.*fal_network_propagate"):
        gpu_propagate(ctx, g, seed, max_hops, min_score)
    check_case(ctx, "min-score-detour")


def test_no_nodes_and_no_links_and_counter_15_is_the_last_calls(ctx):
    assert check_case(ctx, "random-300")["n_reached"] == ctx.counter(15) >= 200
    g, seed, max_hops, min_score, _ = pc.CASES["n-0"]
    rc, out, nr, nl = raw_call(ctx, g, seed, max_hops, min_score)
    assert rc == 0 and all((o == MARK).all() for o in out) and (nr, nl) == (0, 0) and ctx.counter(15) == 0
    assert check_case(ctx, "star-300")["n_reached"] == ctx.counter(15) == 299
    got = check_case(ctx, "no-links")
    assert got["hops"].tolist() == [-1, 0, -1, 0, -1] and got["source"].tolist() == [-1, 1, -1, 3, -1] and ctx.counter(15) == 0
    assert not got["score"][[0, 2, 4]].view(i32).any() and (got["score"][[1, 3]] == 1).all()
    rc, *_ = raw_call(ctx, dict(pc.CASES["n-0"][0], u=np.zeros(1, i32), v=np.ones(1, i32), sim=np.ones(1, f32)), seed, 3, 0.0)
    assert rc == -1                                                                # a link between no nodes


# ---- the public function -----------------------------------------------------------------------------------------------------------
def test_propagate_annotations_of_the_analogue_network(ctx):
    from falcon_amd.cluster import cluster as fcl
    from tests import network_cases as nc
    n_templates = 20
    nodes = nc.analogue_case(n_templates=n_templates)
    a = nc.ANALOGUE
    n = len(nodes["rows"])
    assert n == 300
    n_rows = len(nodes["indptr"]) - 1
    pm_row = np.full(n_rows, 300.0, f32)
    pm_row[nodes["rows"]] = nodes["precursor_mz"]
    ds = fcl.SpectrumDataset(pm_row, np.zeros(n_rows, f32), nodes["mz"], nodes["intensity"], nodes["indptr"])
    pipe = fcl.ClusterPipeline(ctx)
    net = fcl.representative_network(ds, nodes["rows"], a["fragment_tol"], a["max_shift"], a["min_cosine"], a["min_matched"], 5,
                                     pipeline=pipe)
    fam = fcl.network_families(net, n, max_size=0, pipeline=pipe)
    # the library: the first two copies at shift 0 of every third template; 0.05 Da takes that template's three copies at shift
    # 0, each with two hits
    named = np.sort(np.concatenate([np.arange(0, n_templates, 3) * 15, np.arange(0, n_templates, 3) * 15 + 1]))
    l_side = nc.make_nodes([nc.peaks(nodes, int(v)) for v in named], nodes["precursor_mz"][named])
    lds = fcl.SpectrumDataset(l_side["precursor_mz"], None, l_side["mz"], l_side["intensity"], l_side["indptr"])
    hits = fcl.library_search(ds, nodes["rows"], lds, a["fragment_tol"], 0.05, "Da", min_cosine=a["min_cosine"],
                              min_matched_peaks=a["min_matched"], top_n=2, pipeline=pipe)
    assert len(fam["a"]) >= 300 and fam["n_cut"] == 0 and len(hits["cluster"]) > len(np.unique(hits["cluster"])) >= 7
    # the restatement, composed by hand: a cluster's seed is the index of the first entry of its run in `hits`
    seed = np.full(n, -1, i32)
    for e in range(len(hits["cluster"]) - 1, -1, -1):
        seed[hits["cluster"][e]] = e
    for max_hops, min_score in ((3, 0.0), (1, 0.0), (64, 0.99)):
        want = pc.propagate(n, fam["a"], fam["b"], fam["similarity"], seed, max_hops, min_score)
        rows = np.flatnonzero(want["hops"] >= 0)
        print(max_hops, min_score, {k: v for k, v in want.items() if not isinstance(v, np.ndarray)}, len(rows))
        got = fcl.propagate_annotations(fam, hits, n, max_hops, min_score, pipeline=pipe)
        assert all(isinstance(got[k], np.ndarray) for k in ("cluster", "hops", "source", "via", "score", "hit"))
        assert nc.same(got["cluster"], rows.astype(i32)) and nc.same(got["hops"], want["hops"][rows])
        assert nc.same(got["source"], want["source"][rows]) and nc.same(got["via"], want["parent"][rows])
        assert nc.same(got["score"], want["score"][rows]) and nc.same(got["hit"], seed[want["source"][rows]])
        assert (got["n_seeds"], got["n_reached"], got["n_levels"]) == (int((seed >= 0).sum()), want["n_reached"], want["n_levels"])
        # some families hold a seed and some none: every cluster of a named template's family within reach, none of the others
        assert got["n_seeds"] >= 7 and got["n_reached"] >= 7 and len(rows) < n
        assert set(fam["node_family"][rows].tolist()) == set(fam["node_family"][seed >= 0].tolist())
        assert len(set(fam["node_family"].tolist()) - {-1}) > len(set(fam["node_family"][rows].tolist()))
        # the hit of a row is a rank-1 entry of its source
        assert np.array_equal(hits["cluster"][got["hit"]], got["source"]) and (got["hit"] == seed[got["source"]]).all()


# ---- main() ------------------------------------------------------------------------------------------------------------------------
NETWORK_ARGS = ["--network", "--network_min_cosine", "0.5", "--network_min_matched_peaks", "4", "--network_top_k", "2",
                "--network_max_shift", "60", "--network_families", "--network_max_family_size", "0"]
NETWORK_LINES = ["network = True", "network_min_cosine = 0.500", "network_min_matched_peaks = 4", "network_top_k = 2",
                 "network_max_shift = 60.000", "network_families = True", "network_max_family_size = 0", "network_family_delta = 0.020"]
LIBRARY_ARGS = ["--library_min_cosine", "0.5", "--library_min_matched_peaks", "4", "--library_top_n", "2"]
PROPAGATE_ARGS = ["--library_propagate", "--library_propagate_hops", "2", "--library_propagate_min_score", "0.8"]
CHAIN_STEPS = (0.95, 0.95, 0.915)
NAMED = (0, 1, 3)


def _write_chains_and_library(mgf, lib_mgf):
    """tests/test_gpu_families.py's chains: six templates, each at four precursor shifts with about half of its peaks moving
    along; three peaks join the spectrum at every shift, sized so that the cosine of a variant and the next is CHAIN_STEPS (that
    of variants further apart is the product of the steps between them; with --network_top_k 2 the variants of a template are a chain).  Every variant with two noisy copies at nearly its
    precursor (they cluster with it), charges 2 and 3 -> the input MGF; and a GNPS-style library of variant 0 of the templates
    NAMED (charges 2, 3, 3), with a name that needs quoting: the families of the other templates hold no annotated cluster"""
    from falcon_amd.ms_io import ms_io
    from tests import network_cases as nc
    rng = np.random.default_rng(12)
    specs, lines = [], []
    for t in range(6):
        mz, it = np.sort(rng.uniform(150.0, 850.0, 30)), rng.uniform(1e3, 1e4, 30)
        moves = rng.permutation(30) < 15
        group = rng.permutation(30)[:9].reshape(3, 3)
        energy = float(np.sum(np.delete(it, group.ravel()) ** 2))
        for g, cos in zip(group, CHAIN_STEPS):                 # cosine of a variant and the next: sqrt(energy before / after)
            it[g] = np.sqrt(energy * (1.0 / cos ** 2 - 1.0) / 3.0)
            energy /= cos ** 2
        for k, s in enumerate(nc.ANALOGUE_SHIFTS[:4]):
            has = np.ones(30, bool)
            has[group[k:].ravel()] = False
            pmz = 940.0 + 3.0 * t + s
            if k == 0 and t in NAMED:
                lines += ["BEGIN IONS", f"PEPMASS={pmz:.4f}", f"CHARGE={2 + t % 2}+", f'NAME=Compound {t}, "form {t}" M+H',
                          f"SPECTRUMID=CCMSLIB{t:08d}", "ADDUCT=M+H", f"INCHIKEY=KEY-{t}", "IONMODE=Positive"]
                lines += [f"{a:.4f} {b:.2f}" for a, b in zip(mz[has], (0.01 * it)[has])] + ["END IONS", ""]
            for c in range(3):
                m = (mz + moves * s + rng.normal(0.0, 0.002, 30))[has]
                o = np.argsort(m)
                specs.append({"identifier": f"scan={len(specs) + 1}", "precursor_mz": pmz * (1.0 + rng.normal(0, 1e-6)),
                              "precursor_charge": 2 + t % 2, "retention_time": float(np.round(rng.uniform(0.0, 3600.0), 3)),
                              "mz": m[o], "intensity": (it * rng.uniform(0.97, 1.03, 30))[has][o].astype(np.float32)})
    ms_io.write_spectra(mgf, [specs[i] for i in rng.permutation(len(specs))])
    open(lib_mgf, "w").write("\n".join(lines))


def _table(path):
    return list(csv.DictReader(l for l in open(path, newline="").read().split("\n") if l and not l.startswith("#")))


def _expected_annotations(ctx, out, work, header):
    """the annotations file's text: per charge the surviving links, the families and the hits read back from the run's other
    files (float32 columns are written in their shortest round-trip form), the library the run left in its work directory and
    the medoids' precursors from its partitions, through `cluster.propagate_annotations` and `annotation_io`
    -> (text, per-charge results of the Python API)"""
    from falcon_amd.cluster import cluster as fcl
    from falcon_amd.ms_io import annotation_io
    pipe = fcl.ClusterPipeline(ctx)
    rows = _table(out + ".csv")
    cluster_of = {r["spectrum_id"]: int(r["cluster"]) for r in rows}
    title_of = {}
    for entry in open(out + ".mgf").read().split("BEGIN IONS")[1:]:
        fields = dict(l.split("=", 1) for l in entry.splitlines() if "=" in l and not l[0].isdigit())
        title_of[int(fields["CLUSTER"])] = fields["TITLE"]
    links, fams, hits = _table(out + ".network.csv"), _table(out + ".families.csv"), _table(out + ".library.csv")
    blocks, results = [], []
    for charge in json.load(open(os.path.join(work, "spectra", "charges.json"))):
        z = np.load(os.path.join(work, "spectra", f"spectra_charge_{charge}.npz"))
        ref = np.load(os.path.join(work, "spectra", f"reference_charge_{charge}.npz"))
        glob = np.array([cluster_of[str(i)] for i in z["identifier"]], np.int64)
        first, n = int(glob.min()), int(glob.max()) - int(glob.min()) + 1
        row_of = {str(t): i for i, t in enumerate(z["identifier"])}
        pmz = z["precursor_mz"].astype(f32)[[row_of[title_of[c + first]] for c in range(n)]]
        mine = [r for r in links if r["precursor_charge"] == charge]
        net = dict(a=np.array([int(r["cluster_a"]) - first for r in mine], i32), b=np.array([int(r["cluster_b"]) - first for r in mine], i32),
                   similarity=np.array([r["cosine"] for r in mine], f32))
        family = np.array([int(r["family"]) for r in fams if r["precursor_charge"] == charge], i32)         # (global ids)
        assert len(family) == n
        mine = [r for r in hits if r["precursor_charge"] == charge]
        lib_row = {str(x): i for i, x in enumerate(ref["library_id"])}
        hit = dict(cluster=np.array([int(r["cluster"]) - first for r in mine], i32), library=np.array([lib_row[r["library_id"]] for r in mine], i32),
                   similarity=np.array([r["cosine"] for r in mine], f32))
        res = fcl.propagate_annotations(net, hit, n, 2, 0.8, pipeline=pipe)
        b = dict(res, charge=charge, first=first, family=family[res["cluster"]], n_families=0, delta_mz=pmz[res["cluster"]] - pmz[res["source"]],
                 library=hit["library"][res["hit"]], library_cosine=hit["similarity"][res["hit"]])
        b.update({k: ref[k] for k in ("library_id", "name", "library_file", "adduct", "smiles", "inchikey")})
        blocks.append(b)
        results.append(dict(res, seed_clusters=np.unique(hit["cluster"]), n=n, links=net))
    order = sorted(range(len(blocks)), key=lambda k: blocks[k]["first"])
    f = io.StringIO(newline="")
    annotation_io.write_annotations(f, header, [blocks[k] for k in order])
    return f.getvalue(), [results[k] for k in order]


def test_main_writes_the_annotations(ctx, tmp_path):
    from falcon_amd.falcon import main
    mgf, lib_mgf, work = str(tmp_path / "in.mgf"), str(tmp_path / "gnps_like.mgf"), str(tmp_path / "work")
    _write_chains_and_library(mgf, lib_mgf)
    plain, full = str(tmp_path / "plain"), str(tmp_path / "full")
    common = ["--eps", "0.3", "--export_representatives", "--work_dir", work] + NETWORK_ARGS + ["--library", lib_mgf] + LIBRARY_ARGS
    assert main([mgf, plain] + common) == 0
    assert main([mgf, full] + common + PROPAGATE_ARGS) == 0
    for ext in (".csv", ".mgf", ".network.csv", ".families.csv", ".library.csv"):
        assert open(plain + ext, "rb").read() == open(full + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".annotations.csv")
    header = [l[2:] for l in open(full + ".csv", newline="").read().split("\n") if l.startswith("# ")]
    header += NETWORK_LINES
    header += [f"library = {lib_mgf}", "library_analog = False", "library_max_shift = 200.000", "library_min_cosine = 0.500",
               "library_min_matched_peaks = 4", "library_top_n = 2"]
    header += ["library_propagate = True", "library_propagate_hops = 2", "library_propagate_min_score = 0.800"]
    text, results = _expected_annotations(ctx, full, work, header)
    got = open(full + ".annotations.csv", newline="").read()
    assert got == text
    # what the run found, by the restatement: in every charge annotated clusters, clusters reached from them, and clusters of
    # families without a name (or too far from it) that have no row
    assert len(results) == 2
    for r in results:
        seed = np.full(r["n"], -1, i32)
        seed[r["seed_clusters"]] = 1
        want = pc.propagate(r["n"], r["links"]["a"], r["links"]["b"], r["links"]["similarity"], seed, 2, 0.8)
        rows = np.flatnonzero(want["hops"] >= 0)
        print({k: v for k, v in want.items() if not isinstance(v, np.ndarray)}, len(rows), r["n"])
        assert np.array_equal(r["cluster"], rows) and np.array_equal(r["hops"], want["hops"][rows])
        assert np.array_equal(r["score"].view(i32), want["score"][rows].view(i32)) and np.array_equal(r["source"], want["source"][rows])
        assert r["n_seeds"] >= 1 and want["n_reached"] >= 1 and len(rows) < r["n"]
    assert max(r["n_levels"] for r in results) == 2
    table = _table(full + ".annotations.csv")
    assert len(table) == sum(len(r["cluster"]) for r in results)
    assert [int(r["cluster"]) for r in table] == sorted(int(r["cluster"]) for r in table)
    for row in table:
        t = int(row["library_id"][-1])
        assert t in NAMED and row["name"] == f'Compound {t}, "form {t}" M+H' and row["precursor_charge"] == str(2 + t % 2)
        assert (row["via_cluster"] == "") == (row["hops"] == "0") == (row["source_cluster"] == row["cluster"])
        assert int(row["family"]) >= 0 or row["hops"] == "0"
    assert main([mgf, full] + common + PROPAGATE_ARGS) == 1                         # the files are there: refused without --overwrite
    for ext in (".csv", ".mgf", ".network.csv", ".families.csv", ".library.csv"):
        os.remove(full + ext)
    assert main([mgf, full] + common + PROPAGATE_ARGS) == 1                         # the annotations file alone refuses too


# ---- scratch hygiene -------------------------------------------------------------------------------------------------------------
def test_cases_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 (scratch filled with 0xFF before use, a slot that grows while a pointer into it is held fails) is
    read once per process: a fresh child runs the cases again, a small one first"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "propagate_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
