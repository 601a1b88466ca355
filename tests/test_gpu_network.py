"""The representative network on the device (`fal_network_edges`) against the numpy restatement of tests/network_cases.py: every
comparison is on bits, every "at least" is asserted on the restatement's statistics.  Analogue families (the greedy kernel's
pair count against the count from the inputs), tile and band edges, the scope at one ulp, the thresholds' boundaries, ties,
large sides and the peak limit, `max_edges`, node order, the public function and `main()` with `--network`.

The strip case lists more large-sided pairs than the list of its one tile holds before the host has seen a count: it takes the
second run.  No test overflows the small-sided list or the edge buffer (4 M entries)."""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import network_cases as nc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def analogue():
    nodes = nc.analogue_case()
    return nodes, nc.score_pairs(nodes, nc.ANALOGUE["fragment_tol"], nc.ANALOGUE["max_shift"])


def gpu_edges(ctx, nodes, tol, max_shift, min_cosine, min_matched, top_k, max_edges=None):
    out = ctx.network_edges(nodes["mz"], nodes["intensity"], nodes["indptr"], nodes["rows"], nodes["precursor_mz"], tol, max_shift,
                            min_cosine, min_matched, top_k, max_edges=max_edges)
    return tuple(t.cpu().numpy() for t in out)


def check(ctx, nodes, tol, max_shift, min_cosine, min_matched, top_k, scored=None):
    """the device == the restatement, the greedy kernel's pairs included -> (edges, stats of the restatement)"""
    stats = {}
    scored = nc.score_pairs(nodes, tol, max_shift) if scored is None else scored
    want = nc.network_from(scored, min_cosine, min_matched, top_k, stats)
    got = gpu_edges(ctx, nodes, tol, max_shift, min_cosine, min_matched, top_k)
    assert nc.same_edges(got, want), (len(got[0]), len(want[0]))
    assert ctx.counter(12) == stats["greedy_pairs"], (ctx.counter(12), stats)
    return want, stats


# ---- analogue families ---------------------------------------------------------------------------------------------------------
def check_analogue(ctx, analogue, top_k):
    nodes, scored = analogue
    a = nc.ANALOGUE
    _, stats = check(ctx, nodes, a["fragment_tol"], a["max_shift"], a["min_cosine"], a["min_matched"], top_k, scored)
    assert len(nodes["rows"]) == 120
    assert stats["edges_before_top_k"] >= 300 and stats["refused_pairs"] >= 200 and stats["shift_only_edges"] >= 200, stats
    if top_k == 5:
        assert 0 < stats["edges"] <= stats["edges_before_top_k"] // 2, stats
    return stats


@pytest.mark.parametrize("top_k", [0, 1, 5])
def test_analogue_families(ctx, analogue, top_k):
    check_analogue(ctx, analogue, top_k)


def test_the_result_does_not_depend_on_the_node_order(ctx, analogue):
    nodes, scored = analogue
    a = nc.ANALOGUE
    assert len(set(nodes["precursor_mz"].tolist())) == 120
    want = nc.network_from(scored, a["min_cosine"], a["min_matched"], 5)
    perm = np.random.default_rng(2).permutation(120)
    got = gpu_edges(ctx, nc.permute_nodes(nodes, perm), a["fragment_tol"], a["max_shift"], a["min_cosine"], a["min_matched"], 5)
    assert nc.same_edges(nc.map_back(got, perm), want)


# ---- tiles, bands, scope ---------------------------------------------------------------------------------------------------------
TILE_CASES = [(n, band) for n in nc.TILE_SIZES for band in nc.TILE_BANDS]


def check_tile(ctx, n, band):
    nodes, max_shift = nc.tile_case(n, band)
    _, stats = check(ctx, nodes, 0.05, max_shift, 0.0, 0, 0)
    if n >= 63:
        assert stats["in_scope"] >= 100 and stats["edges"] >= stats["in_scope"] // 3, stats
    check(ctx, nodes, 0.05, max_shift, 0.0, 0, 3)


@pytest.mark.parametrize("n,band", TILE_CASES, ids=[f"{n}-{b}" for n, b in TILE_CASES])
def test_tile_and_band_edges(ctx, n, band):
    check_tile(ctx, n, band)


def test_scope_at_one_ulp(ctx):
    nodes, max_shift = nc.ulp_case()
    want, stats = check(ctx, nodes, 0.05, max_shift, 0.0, 0, 0)
    assert stats["edges"] == stats["in_scope"] and 64 * 63 // 2 + 64 * 6 < stats["in_scope"] < 73 * 72 // 2, stats


def test_threshold_boundaries(ctx, analogue):
    nodes, scored = analogue
    a = nc.ANALOGUE
    p = next(p for p in scored if p["matched"] >= 8 and 0.75 < p["sim"] < 0.999)
    has = lambda edges: (p["u"], p["v"]) in set(zip(edges[0].tolist(), edges[1].tolist()))
    up = float(np.nextafter(p["sim"], f32(2), dtype=f32))
    assert has(check(ctx, nodes, a["fragment_tol"], a["max_shift"], float(p["sim"]), 6, 0, scored)[0])
    assert not has(check(ctx, nodes, a["fragment_tol"], a["max_shift"], up, 6, 0, scored)[0])
    assert has(check(ctx, nodes, a["fragment_tol"], a["max_shift"], 0.7, p["matched"], 0, scored)[0])
    assert not has(check(ctx, nodes, a["fragment_tol"], a["max_shift"], 0.7, p["matched"] + 1, 0, scored)[0])
    q = next(q for q in scored if 2 <= min(q["hit_a"], q["hit_b"]) <= 20)
    h = min(q["hit_a"], q["hit_b"])
    assert nc.classify(q, h) != nc.REJECT and nc.classify(q, h + 1) == nc.REJECT
    check(ctx, nodes, a["fragment_tol"], a["max_shift"], 0.0, h, 0, scored)
    check(ctx, nodes, a["fragment_tol"], a["max_shift"], 0.0, h + 1, 0, scored)


@pytest.mark.parametrize("top_k", [0, 2, 5])
def test_ties(ctx, top_k):
    nodes = nc.tie_case()
    _, stats = check(ctx, nodes, 0.05, 50.0, 0.5, 3, top_k)
    assert stats["refused_pairs"] >= 15


# ---- large sides -------------------------------------------------------------------------------------------------------------------
def check_large(ctx):
    nodes = nc.strip_case()
    _, stats = check(ctx, nodes, 0.05, 10.0, 0.3, 6, 0)
    assert stats["greedy_pairs"] >= 600 and stats["edges"] >= 300, stats
    nodes = nc.lds_case()
    assert np.sort(np.diff(nodes["indptr"])[nodes["rows"]])[-64:].sum() > 3200
    _, stats = check(ctx, nodes, 0.05, 10.0, 0.0, 0, 4)
    assert stats["edges_before_top_k"] >= 1000, stats


def test_sides_above_a_strip_and_above_the_lds_capacity(ctx):
    check_large(ctx)


def test_the_peak_limit_counts_only_inside_the_scope_and_the_context_stays_usable(ctx):
    from falcon_amd._lib import FalconHipError
    nodes, max_shift = nc.limit_case(True)
    with pytest.raises(FalconHipError, match="code -5.*more than 4096 peaks"):
        gpu_edges(ctx, nodes, 0.05, max_shift, 0.0, 0, 0)
    nodes, max_shift = nc.limit_case(False)
    _, stats = check(ctx, nodes, 0.05, max_shift, 0.0, 0, 0)
    assert stats["in_scope"] == 6 and stats["greedy_pairs"] >= 1 and stats["edges"] >= 3, stats


def test_a_row_outside_the_csr_is_an_error(ctx):
    from falcon_amd._lib import FalconHipError
    nodes, max_shift = nc.tile_case(65, "all")
    bad = dict(nodes, rows=nodes["rows"].copy())
    bad["rows"][7] = len(nodes["indptr"]) - 1
    with pytest.raises(FalconHipError, match="code -1.*outside"):
        gpu_edges(ctx, bad, 0.05, max_shift, 0.0, 0, 0)
    check(ctx, nodes, 0.05, max_shift, 0.0, 0, 0)


# ---- max_edges -------------------------------------------------------------------------------------------------------------------
def test_max_edges_and_no_nodes(ctx, analogue):
    import torch
    nodes, scored = analogue
    a = nc.ANALOGUE
    want = nc.network_from(scored, a["min_cosine"], a["min_matched"], 5)
    m_true = len(want[0])
    dev = [ctx.to_dev(nodes[k], t) for k, t in (("mz", torch.float32), ("intensity", torch.float32), ("indptr", torch.int64),
                                               ("rows", torch.int32), ("precursor_mz", torch.float32))]

    def call(room, n=120):
        out = [ctx.empty((max(room, 1),), t) for t in (torch.int32, torch.int32, torch.float32, torch.int32)]
        for t in out:
            t.fill_(-7)
        m = C.c_int64(-1)
        rc = ctx.lib.fal_network_edges(ctx._h, *(ctx._p(t) for t in dev[:3]), len(nodes["indptr"]) - 1, ctx._p(dev[3]), ctx._p(dev[4]),
                                       n, a["fragment_tol"], a["max_shift"], a["min_cosine"], a["min_matched"], 5,
                                       *(ctx._p(t) for t in out), room, C.byref(m))
        ctx.sync()
        return rc, m.value, tuple(t.cpu().numpy() for t in out)

    rc, m, out = call(m_true - 1)
    assert rc == -1 and m == m_true and all((o == -7).all() for o in out)           # FAL_EINVAL, nothing written
    rc, m, out = call(m)
    assert rc == 0 and m == m_true and nc.same_edges(tuple(o[:m] for o in out), want)
    rc, m, out = call(4, n=0)
    assert rc == 0 and m == 0 and all((o == -7).all() for o in out)
    # the wrapper asks again with the room the library reported
    assert nc.same_edges(gpu_edges(ctx, nodes, a["fragment_tol"], a["max_shift"], a["min_cosine"], a["min_matched"], 5, max_edges=3), want)


# ---- the public function -----------------------------------------------------------------------------------------------------------
def test_representative_network_with_medoid_and_consensus_peaks(ctx):
    from falcon_amd.cluster import cluster as fc
    from tests import consensus_cases as cc
    from tests import memberscore_cases as mc
    case, _ = mc.tile_case(130, "interleaved", seed=3)
    rng = np.random.default_rng(4)
    n_members = len(case["labels"])
    # many small clusters of the same spectra, so that the representatives are related: labels = row mod 40
    labels = (np.arange(n_members) % 40).astype(np.int32)
    medoids = np.array([rng.choice(np.flatnonzero(labels == c)) for c in range(40)], np.int32)
    case = dict(case, labels=labels, medoids=medoids, precursor_mz=(500.0 + rng.uniform(0.0, 30.0, n_members)).astype(f32))
    ds = fc.SpectrumDataset(case["precursor_mz"], case["retention_time"], case["mz"], case["intensity"], case["indptr"])
    pipe = fc.ClusterPipeline(ctx)
    cons = cc.consensus_reference(case["mz"], case["intensity"], case["indptr"], labels, medoids, 0.05, 0.25)[:3]
    for consensus in (None, cons):
        if consensus is None:
            nodes = dict(mz=case["mz"], intensity=case["intensity"], indptr=case["indptr"], rows=medoids)
        else:
            nodes = dict(mz=consensus[1], intensity=consensus[2], indptr=consensus[0], rows=np.arange(40, dtype=np.int32))
        nodes["precursor_mz"] = case["precursor_mz"][medoids]
        stats = {}
        want = nc.network_ref(nodes, 0.05, 20.0, 0.1, 2, 4, stats)
        assert stats["edges"] >= 20 and stats["edges"] < stats["edges_before_top_k"], stats
        out = fc.representative_network(ds, medoids, 0.05, max_shift=20.0, min_cosine=0.1, min_matched_peaks=2, top_k=4,
                                        consensus=consensus, pipeline=pipe)
        assert nc.same_edges((out["a"], out["b"], out["similarity"], out["matched"]), want)
        pm = nodes["precursor_mz"]
        assert nc.same(out["delta_mz"], (pm[want[1]] - pm[want[0]]).astype(f32)) and (out["a"] < out["b"]).all()


# ---- main() ------------------------------------------------------------------------------------------------------------------------
NETWORK_ARGS = ["--network", "--network_min_cosine", "0.5", "--network_min_matched_peaks", "4", "--network_top_k", "2",
                "--network_max_shift", "60"]


def _write_families(path):
    """six templates of 30 peaks, each at four precursor shifts with about half of its peaks moving along, every such spectrum
    with two noisy copies at nearly its precursor (they cluster with it), charges 2 and 3 -> the MGF file"""
    from falcon_amd.ms_io import ms_io
    rng = np.random.default_rng(12)
    specs = []
    for t in range(6):
        mz, it = np.sort(rng.uniform(150.0, 850.0, 30)), rng.uniform(100.0, 1e4, 30)
        moves = rng.permutation(30) < 15
        for s in nc.ANALOGUE_SHIFTS[:4]:
            pmz = 940.0 + 3.0 * t + s
            for c in range(3):
                m = mz + moves * s + rng.normal(0.0, 0.002, 30)
                o = np.argsort(m)
                specs.append({"identifier": f"scan={len(specs) + 1}", "precursor_mz": pmz * (1.0 + rng.normal(0, 1e-6)),
                              "precursor_charge": 2 + t % 2, "retention_time": float(np.round(rng.uniform(0.0, 3600.0), 3)),
                              "mz": m[o], "intensity": (it * rng.uniform(0.9, 1.1, 30))[o].astype(np.float32)})
    ms_io.write_spectra(path, [specs[i] for i in rng.permutation(len(specs))])


def _expected_network(out, work, header):
    """the network file's text from the run's own partitions, the cluster CSV's labels and the exported representatives' titles"""
    from falcon_amd.ms_io import network_io
    lines = open(out + ".csv", newline="").read().split("\n")
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
        row_of = {str(t): i for i, t in enumerate(z["identifier"])}
        medoids = np.array([row_of[title_of[c + first]] for c in range(int(glob.max()) - first + 1)], np.int32)
        nodes = dict(mz=z["mz"], intensity=z["intensity"], indptr=z["indptr"], rows=medoids, precursor_mz=z["precursor_mz"][medoids])
        u, v, sim, matched = nc.network_ref(nodes, 0.05, 60.0, 0.5, 4, 2)
        pm = nodes["precursor_mz"].astype(f32)
        blocks.append((first, dict(charge=charge, first=first, a=u, b=v, similarity=sim, matched=matched, delta_mz=pm[v] - pm[u])))
    blocks = [b for _, b in sorted(blocks, key=lambda x: x[0])]
    f = io.StringIO(newline="")
    network_io.write_network(f, header, blocks)
    return f.getvalue(), blocks


@pytest.mark.parametrize("mode", [[], ["--exact"]], ids=["default", "exact"])
def test_main_writes_the_network(tmp_path, mode):
    from falcon_amd.falcon import main
    mgf, work = str(tmp_path / "in.mgf"), str(tmp_path / "work")
    _write_families(mgf)
    plain, full = str(tmp_path / "plain"), str(tmp_path / "full")
    common = ["--eps", "0.3", "--export_representatives", "--work_dir", work] + mode
    assert main([mgf, plain] + common) == 0
    assert main([mgf, full] + common + NETWORK_ARGS) == 0
    for ext in (".csv", ".mgf"):
        assert open(plain + ext, "rb").read() == open(full + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".network.csv")
    header = [l[2:] for l in open(full + ".csv", newline="").read().split("\n") if l.startswith("# ")]
    header += ["network = True", "network_min_cosine = 0.500", "network_min_matched_peaks = 4", "network_top_k = 2",
               "network_max_shift = 60.000"]
    text, blocks = _expected_network(full, work, header)
    assert len(blocks) == 2 and sum(len(b["a"]) for b in blocks) >= 12 and min(len(b["a"]) for b in blocks) >= 5
    assert open(full + ".network.csv", newline="").read() == text
    assert main([mgf, full] + common + NETWORK_ARGS) == 1                           # the file is there: refused without --overwrite


# ---- scratch hygiene -------------------------------------------------------------------------------------------------------------
def test_cases_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 (scratch filled with 0xFF before use, a slot that grows while a pointer into it is held fails) is
    read once per process: a fresh child runs the analogue, tile and large-side cases again"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "network_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
