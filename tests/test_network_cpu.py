"""The representative network without a GPU: the host build of csrc/netmatch.h against the numpy restatement
(tests/network_cases.py) on every case of the GPU tests, `network_io`'s bytes for hand-written edges, and the options' place in
`config` and in the run's files.  Every comparison with the restatement is on bits; every "at least" is asserted on the
restatement's statistics."""
import io

import numpy as np
import pytest

from tests import hostbuild_network as hb
from tests import network_cases as nc

needs_compiler = pytest.mark.skipif(not hb.have_compiler(), reason="no host C++ compiler")
f32 = np.float32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hb.build(tmp_path_factory.mktemp("network_host"))


@pytest.fixture(scope="module")
def analogue():
    nodes = nc.analogue_case()
    return nodes, nc.score_pairs(nodes, nc.ANALOGUE["fragment_tol"], nc.ANALOGUE["max_shift"])


def check(lib, nodes, tol, max_shift, min_cosine, min_matched, top_k, scored=None):
    """the host build == the restatement -> (edges, stats of the restatement)"""
    stats = {}
    scored = nc.score_pairs(nodes, tol, max_shift) if scored is None else scored
    want = nc.network_from(scored, min_cosine, min_matched, top_k, stats)
    got, counts = hb.network(lib, nodes, tol, max_shift, min_cosine, min_matched, top_k)
    assert nc.same_edges(got, want), (len(got[0]), len(want[0]))
    for k, v in counts.items():
        assert stats[k] == v, (k, stats[k], v)
    return want, stats


# ---- the header ----------------------------------------------------------------------------------------------------------------
@needs_compiler
def test_the_peak_limit_is_the_restatements(lib):
    from falcon_amd import _lib
    assert lib.t_max_peaks() == nc.MAX_PEAKS == _lib.NET_MAX_PEAKS


@needs_compiler
@pytest.mark.parametrize("top_k", [0, 1, 5])
def test_analogue_families(lib, analogue, top_k):
    nodes, scored = analogue
    assert len(nodes["rows"]) == 120
    a = nc.ANALOGUE
    _, stats = check(lib, nodes, a["fragment_tol"], a["max_shift"], a["min_cosine"], a["min_matched"], top_k, scored)
    assert stats["edges_before_top_k"] >= 300 and stats["refused_pairs"] >= 200 and stats["shift_only_edges"] >= 200, stats
    assert stats["greedy_pairs"] >= 200 and stats["rejected_cardinality"] >= 200, stats
    if top_k == 5:
        assert 0 < stats["edges"] <= stats["edges_before_top_k"] // 2, stats
    if top_k == 0:
        assert stats["edges"] == stats["edges_before_top_k"]


@needs_compiler
def test_the_analogue_case_does_not_depend_on_the_node_order(lib, analogue):
    nodes, scored = analogue
    a = nc.ANALOGUE
    want = nc.network_from(scored, a["min_cosine"], a["min_matched"], 5)
    perm = np.random.default_rng(2).permutation(120)            # new node v = old node perm[v]
    got, _ = hb.network(lib, nc.permute_nodes(nodes, perm), a["fragment_tol"], a["max_shift"], a["min_cosine"], a["min_matched"], 5)
    assert nc.same_edges(nc.map_back(got, perm), want)


TILE_CASES = [(n, band) for n in nc.TILE_SIZES for band in nc.TILE_BANDS]


@needs_compiler
@pytest.mark.parametrize("n,band", TILE_CASES, ids=[f"{n}-{b}" for n, b in TILE_CASES])
def test_tile_and_band_edges(lib, n, band):
    nodes, max_shift = nc.tile_case(n, band)
    want, stats = check(lib, nodes, 0.05, max_shift, 0.0, 0, 0)
    if n >= 63:
        assert stats["in_scope"] >= 100 and stats["edges"] >= stats["in_scope"] // 3, stats
    if band == "all":
        assert stats["in_scope"] == n * (n - 1) // 2
    if band == "equal" and n >= 63:                              # equal precursors: the node index orders the pair
        pmz = nodes["precursor_mz"]
        assert all(pmz[u] == pmz[v] for u, v in zip(want[0], want[1])) and stats["in_scope"] < n * (n - 1) // 2
    check(lib, nodes, 0.05, max_shift, 0.0, 0, 3)


@needs_compiler
def test_scope_at_one_ulp(lib):
    nodes, max_shift = nc.ulp_case()
    want, stats = check(lib, nodes, 0.05, max_shift, 0.0, 0, 0)
    pmz = nodes["precursor_mz"]
    p0, (inside, outside) = f32(500.0), nc.scope_edges(f32(500.0), max_shift)
    at = lambda x: set(np.flatnonzero(pmz == x).tolist())
    pairs = set(zip(want[0].tolist(), want[1].tolist()))
    linked = lambda s, t: all((min(u, v), max(u, v)) in pairs for u in s for v in t if u != v)
    apart = lambda s, t: not any((min(u, v), max(u, v)) in pairs for u in s for v in t)
    assert len(at(p0)) == 64 and len(at(inside)) == 3 and len(at(outside)) == 3
    assert linked(at(p0), at(inside)) and apart(at(p0), at(outside)) and linked(at(inside), at(outside))


@needs_compiler
def test_threshold_boundaries(lib, analogue):
    nodes, scored = analogue
    a = nc.ANALOGUE
    p = next(p for p in scored if p["matched"] >= 8 and 0.75 < p["sim"] < 0.999)
    has = lambda edges: (p["u"], p["v"]) in set(zip(edges[0].tolist(), edges[1].tolist()))
    s = float(p["sim"])
    up = float(np.nextafter(p["sim"], f32(2), dtype=f32))
    assert has(check(lib, nodes, a["fragment_tol"], a["max_shift"], s, 6, 0, scored)[0])
    assert not has(check(lib, nodes, a["fragment_tol"], a["max_shift"], up, 6, 0, scored)[0])
    assert has(check(lib, nodes, a["fragment_tol"], a["max_shift"], 0.7, p["matched"], 0, scored)[0])
    assert not has(check(lib, nodes, a["fragment_tol"], a["max_shift"], 0.7, p["matched"] + 1, 0, scored)[0])
    # a pair the cardinality prefilter rejects at exactly min_matched - 1
    q = next(q for q in scored if 2 <= min(q["hit_a"], q["hit_b"]) <= 20)
    h = min(q["hit_a"], q["hit_b"])
    assert nc.classify(q, h) != nc.REJECT and nc.classify(q, h + 1) == nc.REJECT
    check(lib, nodes, a["fragment_tol"], a["max_shift"], 0.0, h, 0, scored)
    check(lib, nodes, a["fragment_tol"], a["max_shift"], 0.0, h + 1, 0, scored)


@needs_compiler
@pytest.mark.parametrize("top_k", [0, 2, 5])
def test_ties(lib, top_k):
    nodes = nc.tie_case()
    want, stats = check(lib, nodes, 0.05, 50.0, 0.5, 3, top_k)
    twins = np.flatnonzero(nodes["precursor_mz"] == f32(600.0))
    assert len(twins) == 6 and stats["refused_pairs"] >= 15
    between = [(u, v, s) for u, v, s in zip(*want[:3]) if u in twins and v in twins]
    if top_k == 0:
        assert len(between) == 15 and len({nc.bits(np.array([s], f32))[0] for _, _, s in between}) == 1
    if top_k == 2:                                               # five equal edges a twin: the ranks go to the lower nodes
        low = sorted(twins.tolist())[:3]
        assert sorted((u, v) for u, v, _ in between) == [(low[0], low[1]), (low[0], low[2]), (low[1], low[2])]


@needs_compiler
def test_large_sides(lib):
    nodes = nc.strip_case()
    want, stats = check(lib, nodes, 0.05, 10.0, 0.3, 6, 0)
    assert stats["greedy_pairs"] >= 600 and stats["edges"] >= 300, stats
    assert (np.diff(nodes["indptr"])[nodes["rows"]] == 0).sum() == 2
    nodes = nc.lds_case()
    assert np.sort(np.diff(nodes["indptr"])[nodes["rows"]])[-64:].sum() > 3200
    want, stats = check(lib, nodes, 0.05, 10.0, 0.0, 0, 4)
    assert stats["edges_before_top_k"] >= 1000, stats


@needs_compiler
def test_the_peak_limit_counts_only_inside_the_scope(lib):
    nodes, max_shift = nc.limit_case(True)
    with pytest.raises(nc.Unsupported):
        nc.score_pairs(nodes, 0.05, max_shift)
    assert hb.network(lib, nodes, 0.05, max_shift, 0.0, 0, 0)[0] is None
    nodes, max_shift = nc.limit_case(False)
    want, stats = check(lib, nodes, 0.05, max_shift, 0.0, 0, 0)
    assert stats["in_scope"] == 6 and stats["greedy_pairs"] >= 1 and stats["edges"] >= 3, stats


# ---- network_io ----------------------------------------------------------------------------------------------------------------
def test_network_io_bytes():
    from falcon_amd.ms_io import network_io
    blocks = [dict(charge="2", first=0, a=np.array([0, 0], np.int32), b=np.array([1, 3], np.int32),
                   similarity=np.array([0.75, 1.0], f32), matched=np.array([6, 12], np.int32), delta_mz=np.array([14.0157, 0.0], f32)),
              dict(charge="3", first=4, a=np.zeros(0, np.int32), b=np.zeros(0, np.int32), similarity=np.zeros(0, f32),
                   matched=np.zeros(0, np.int32), delta_mz=np.zeros(0, f32)),
              dict(charge="None", first=9, a=np.array([1], np.int32), b=np.array([2], np.int32),
                   similarity=np.array([0.1 + 0.7], f32), matched=np.array([7], np.int32), delta_mz=np.array([-0.5], f32))]
    f = io.StringIO(newline="")
    network_io.write_network(f, ["falcon version x", "network = True"], blocks)
    assert f.getvalue() == ("# falcon version x\n# network = True\n#\n"
                            "cluster_a,cluster_b,precursor_charge,delta_mz,cosine,matched_peaks\n"
                            "0,1,2,14.0157,0.75,6\n0,3,2,0.0,1.0,12\n10,11,None,-0.5,0.8,7\n")


# ---- config ----------------------------------------------------------------------------------------------------------------------
def test_network_options_and_parse_errors(capsys):
    from falcon_amd.config import Config
    c = Config()
    c.parse("in.mgf out")
    assert c.network is False and (c.network_min_cosine, c.network_min_matched_peaks, c.network_top_k, c.network_max_shift) == \
        (0.7, 6, 10, 200.0)
    c.parse("in.mgf out --network --network_min_cosine 0.6 --network_min_matched_peaks 4 --network_top_k 0 --network_max_shift 50 "
            "--exact")
    assert c.network is True and (c.network_min_cosine, c.network_min_matched_peaks, c.network_top_k, c.network_max_shift) == \
        (0.6, 4, 0, 50.0)
    for bad, text in (("--network --assign_to reps.mgf", "--network does not combine with --assign_to"),
                      ("--network --distributed", "--network does not combine with --distributed"),
                      ("--network_min_cosine 1.5", "--network_min_cosine 1.5 is outside [0, 1]"),
                      ("--network_min_cosine -0.1", "is outside [0, 1]"),
                      ("--network_min_matched_peaks -1", "--network_min_matched_peaks -1 is negative"),
                      ("--network_top_k -2", "--network_top_k -2 is negative"),
                      ("--network_max_shift -1", "--network_max_shift -1.0 is negative")):
        with pytest.raises(SystemExit):
            c.parse("in.mgf out " + bad)
        assert text in capsys.readouterr().err, bad
    c.parse("in.mgf out --network_min_cosine 0 --network_max_shift 0 --network_min_matched_peaks 0")
    c.parse("in.mgf out --network_min_cosine 1")


def test_network_from_an_ini_file(tmp_path):
    from falcon_amd.config import Config
    ini = tmp_path / "falcon.ini"
    ini.write_text("network = true\nnetwork_top_k = 3\nnetwork_max_shift = 42.5\n")
    c = Config()
    c.parse(f"-c {ini} in.mgf out")
    assert c.network is True and c.network_top_k == 3 and c.network_max_shift == 42.5 and c.network_min_cosine == 0.7
    c.parse(f"-c {ini} in.mgf out --network_top_k 7")
    assert c.network_top_k == 7
    ini.write_text("network = true\ndistributed = true\n")
    with pytest.raises(SystemExit):
        c.parse(f"-c {ini} in.mgf out")
    c.parse("in.mgf out")
    assert c.network is False


def test_the_log_lists_the_options_and_the_cluster_csv_header_does_not():
    from falcon_amd import falcon
    from falcon_amd.config import config
    config.parse("in.mgf out")
    base = falcon._option_lines()
    assert not any("network" in l for l in base) and falcon._option_lines(header=True) == base
    header = falcon._header_lines()
    config.parse("in.mgf out --network --network_top_k 5")
    net = ["network = True", "network_min_cosine = 0.700", "network_min_matched_peaks = 6", "network_top_k = 5",
           "network_max_shift = 200.000"]
    assert falcon._option_lines() == base + net and falcon._network_lines() == net
    assert falcon._option_lines(header=True) == base and falcon._header_lines() == header
    config.parse("in.mgf out --cluster_summary --network")
    assert falcon._option_lines() == base + ["cluster_summary = True"] + falcon._network_lines()


def test_an_existing_network_file_stops_the_run_unless_overwrite(tmp_path):
    from falcon_amd import falcon
    from falcon_amd.config import config
    out = str(tmp_path / "run")
    open(out + ".network.csv", "w").close()
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'}")
    assert falcon._setup_work_dir() == (False, 0)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} --network")
    assert falcon._setup_work_dir() == (False, 1)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} --network --overwrite")
    assert falcon._setup_work_dir() == (False, 0)
    assert not (tmp_path / "run.network.csv").exists()
