"""Annotation propagation without a GPU: the host build of csrc/netpropagate.h against the numpy restatement
(tests/propagate_cases.py) on every case of the GPU tests, the restatement's own invariants, `annotation_io`'s bytes for a
two-block example, and the options' place in `config` and in the run's files.  Every comparison with the restatement is on
bits; every "at least" is asserted on the restatement's statistics (propagate_cases.expected)."""
import io

import numpy as np
import pytest

from tests import hostbuild_propagate as hb
from tests import propagate_cases as pc

needs_compiler = pytest.mark.skipif(not hb.have_compiler(), reason="no host C++ compiler")
f32, i32 = np.float32, np.int32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hb.build(tmp_path_factory.mktemp("propagate_host"))


# ---- the header ------------------------------------------------------------------------------------------------------------------
@needs_compiler
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_the_host_build_is_the_restatement(lib, name):
    g, seed, max_hops, min_score, _ = pc.CASES[name]
    want = pc.expected(name)
    got = hb.propagate(lib, g, seed, max_hops, min_score)
    assert pc.same(got, want), (got["n_reached"], want["n_reached"], got["n_levels"], want["n_levels"])


@needs_compiler
@pytest.mark.parametrize("name", sorted(pc.invalid_cases()))
def test_the_host_build_refuses_what_the_restatement_refuses(lib, name):
    g, seed, max_hops, min_score = pc.invalid_cases()[name]
    assert not pc.valid(g["n"], g["u"], g["v"], g["sim"], seed, max_hops, min_score)
    assert hb.propagate(lib, g, seed, max_hops, min_score) is None


def test_the_refused_inputs_are_the_ones_the_rule_names():
    assert sorted(pc.invalid_cases()) == ["loop", "max-hops-0", "max-hops-65", "max-hops-negative", "min-score-above-1",
                                          "min-score-nan", "min-score-negative", "seed-below-minus-1", "sim-inf", "sim-nan",
                                          "sim-negative", "u-far-outside", "u-negative", "v-is-n"]


@needs_compiler
def test_the_key_orders_as_the_rule_and_unpacks(tmp_path):
    from tests.hostbuild import compile_shim
    import ctypes as C
    shim = compile_shim(tmp_path, "propagate_key_shim", r"""
#include "netpropagate.h"
extern "C" unsigned long long t_key(float c, int32_t a) { return fal::prop_key(c, a); }
extern "C" float t_score(unsigned long long k) { return fal::prop_key_score(k); }
extern "C" int32_t t_parent(unsigned long long k) { return fal::prop_key_parent(k); }
""")
    shim.t_key.argtypes, shim.t_key.restype = [C.c_float, C.c_int32], C.c_uint64
    shim.t_score.argtypes, shim.t_score.restype = [C.c_uint64], C.c_float
    shim.t_parent.argtypes, shim.t_parent.restype = [C.c_uint64], C.c_int32
    cands = [(0.0, 5), (-0.0, 4), (1e-45, 2 ** 31 - 2), (0.75, 9), (0.75, 3), (0.75, 0), (1.0, 7), (3.0e38, 1), (float("inf"), 8)]
    keys = [shim.t_key(c, a) for c, a in cands]
    assert all(k != 0 for k in keys)
    # the rule's order: greater c first, equal c (the two zeros are equal) the lower parent
    assert sorted(range(len(cands)), key=lambda i: keys[i]) == sorted(range(len(cands)), key=lambda i: (cands[i][0], -cands[i][1]))
    for (c, a), k in zip(cands, keys):
        assert shim.t_parent(k) == a and f32(shim.t_score(k)).view(i32) == f32(abs(c) if c == 0 else c).view(i32)
    assert shim.t_key(0.0, 2 ** 31 - 2) == 0x80000001


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
# The tests of this part check the reference itself -- the numpy restatement and the case table of tests/propagate_cases.py -- not
# the library.
def _link_sims(g):
    """(a, b) -> the set of sims of the links between a and b, both directions"""
    sims = {}
    for a, b, s in zip(g["u"].tolist(), g["v"].tolist(), g["sim"]):
        sims.setdefault((a, b), set()).add(s)
        sims.setdefault((b, a), set()).add(s)
    return sims


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_every_reached_node_continues_its_parents_path(name):
    g, seed, max_hops, min_score, _ = pc.CASES[name]
    r = pc.expected(name)
    n = g["n"]
    annotated = seed >= 0
    assert np.array_equal(r["hops"] == 0, annotated) and (r["source"][annotated] == np.flatnonzero(annotated)).all()
    assert (r["parent"][annotated] == -1).all() and (r["score"][annotated] == 1).all()
    out = r["hops"] == -1
    assert (r["source"][out] == -1).all() and (r["parent"][out] == -1).all() and not r["score"][out].view(i32).any()
    reached = np.flatnonzero(r["hops"] >= 1)
    par = r["parent"][reached]
    assert np.array_equal(r["hops"][par], r["hops"][reached] - 1) and np.array_equal(r["source"][par], r["source"][reached])
    assert (seed[r["source"][~out]] >= 0).all() and r["hops"].max(initial=0) <= max_hops
    sims = _link_sims(g)
    with np.errstate(over="ignore"):
        for x, a in zip(reached.tolist(), par.tolist()):
            offers = {(f32(r["score"][a] * s) + f32(0)).view(i32) for s in sims[(a, x)]}          # (+ 0: a zero is +0)
            assert r["score"][x].view(i32) in offers and r["score"][x] >= f32(min_score), (name, x, a)
    assert r["n_reached"] == len(reached) and r["n_levels"] == r["hops"].max(initial=0)
    if min_score == 0:
        assert np.array_equal(r["hops"], pc.bfs_hops(n, g["u"], g["v"], seed, max_hops))
    else:
        bfs = pc.bfs_hops(n, g["u"], g["v"], seed, max_hops)
        assert ((r["hops"] >= bfs) | (r["hops"] == -1)).all()


def test_the_cases_are_the_ones_the_issue_names():
    for name, n, m, k, hops, floor in (("random-300", 300, 420, 12, 64, 0.0), ("random-300-hops-3", 300, 420, 12, 3, 0.0),
                                       ("random-300-min-0.6", 300, 420, 12, 64, 0.6), ("random-300-hops-3-min-0.6", 300, 420, 12, 3, 0.6),
                                       ("random-5000", 5000, 7000, 150, 64, 0.0), ("random-5000-hops-3", 5000, 7000, 150, 3, 0.0),
                                       ("random-5000-min-0.6", 5000, 7000, 150, 64, 0.6),
                                       ("random-5000-hops-3-min-0.6", 5000, 7000, 150, 3, 0.6)):
        g, seed, max_hops, min_score, _ = pc.CASES[name]
        assert (g["n"], int((seed >= 0).sum()), max_hops, min_score) == (n, k, hops, floor) and m - 5 <= len(g["u"]) <= m, name
        assert set(np.unique(g["sim"]).tolist()) == {0.75, 0.875, 1.0}
    for n in (63, 64, 65):
        assert pc.CASES[f"ring-n-{n}"][0]["n"] == n
    for m in (255, 256, 257):
        assert len(pc.CASES[f"ring-m-{m}"][0]["u"]) == m
    hub = pc.CASES["hub-of-seeds-300"]
    assert hub[0]["n"] == 300 and int((hub[1] >= 0).sum()) == 299 and hub[1][0] == -1 and (hub[0]["sim"] == f32(0.75)).all()
    # the statistics the issue asks for, on the restatement
    for name, ties, late in (("random-300", 5, 10), ("random-5000", 50, 300)):
        a, b = pc.expected(name), pc.expected(name + "-min-0.6")
        assert a["tied_sources"] >= ties and a["n_levels"] >= 7 and b["n_levels"] >= 7
        assert int(((b["hops"] > a["hops"]) & (a["hops"] >= 0)).sum()) >= late
        print(name, a["n_reached"], a["n_levels"], a["tied"], a["tied_sources"], int(((b["hops"] > a["hops"]) & (a["hops"] >= 0)).sum()))


def test_link_order_and_duplicates_change_nothing():
    for name in ("random-300", "random-300-min-0.6", "hub-of-seeds-300"):
        g, seed, max_hops, min_score, _ = pc.CASES[name]
        h = pc.shuffled(g, duplicates=40)
        assert len(h["u"]) == len(g["u"]) + 40
        assert pc.same(pc.propagate(h["n"], h["u"], h["v"], h["sim"], seed, max_hops, min_score), pc.expected(name))


def test_a_node_permutation_permutes_a_result_without_ties():
    # (a tie goes to the lowest parent: with ties the permuted graph may choose another one)
    g, seed = pc.chain(9), pc.seeds(9, [2])
    rng = np.random.default_rng(3)
    tree_u = np.array([int(rng.integers(0, b)) for b in range(1, 200)], i32)
    tree = pc.graph(200, tree_u, np.arange(1, 200), rng.uniform(0.7, 1.0, 199).astype(f32))
    for g, seed, max_hops in ((g, seed, 8), (tree, pc.seeds(200, [0, 50, 120]), 64)):
        want = pc.propagate(g["n"], g["u"], g["v"], g["sim"], seed, max_hops, 0.0)
        assert want["tied"] == 0 and want["n_reached"] >= 6
        h, s, perm = pc.permuted(g, seed)
        got = pc.propagate(h["n"], h["u"], h["v"], h["sim"], s, max_hops, 0.0)
        relabel = lambda x: np.where(x >= 0, perm[np.maximum(x, 0)], -1).astype(i32)
        assert np.array_equal(got["hops"][perm], want["hops"]) and np.array_equal(got["score"][perm].view(i32), want["score"].view(i32))
        assert np.array_equal(got["source"][perm], relabel(want["source"])) and np.array_equal(got["parent"][perm], relabel(want["parent"]))
        assert (got["n_reached"], got["n_levels"]) == (want["n_reached"], want["n_levels"])


# ---- annotation_io -----------------------------------------------------------------------------------------------------------------
def _blocks():
    text = lambda *x: np.array(x, dtype=str)
    lib = dict(library_id=text("CCMSLIB01", "CCMSLIB02"), name=text('Rutin, "natural"', "Quercetin"), library_file=text("lib.mgf", "lib.mgf"),
               adduct=text("[M+H]+", ""), smiles=text("C1=CC", "O=C(O)C"), inchikey=text("IKVR", ""))
    return [dict(lib, charge="2", first=0, n_families=2, cluster=np.array([0, 1, 3, 4], i32), hops=np.array([0, 1, 2, 0], i32),
                 source=np.array([0, 0, 0, 4], i32), via=np.array([-1, 0, 1, -1], i32), family=np.array([0, 0, 0, -1], i32),
                 score=np.array([1.0, 0.875, 0.1 + 0.7, 1.0], f32), delta_mz=np.array([0.0, 14.0157, -2.5, 0.0], f32),
                 library=np.array([0, 0, 0, 1], i32), library_cosine=np.array([0.91, 0.91, 0.91, 0.75], f32)),
            dict(lib, charge="None", first=5, n_families=1, cluster=np.array([2], i32), hops=np.array([1], i32), source=np.array([0], i32),
                 via=np.array([0], i32), family=np.array([0], i32), score=np.array([0.75], f32), delta_mz=np.array([1.5], f32),
                 library=np.array([1], i32), library_cosine=np.array([0.8], f32))]


def test_annotation_io_bytes_for_two_blocks(tmp_path):
    from falcon_amd.ms_io import annotation_io
    blocks = _blocks()
    f = io.StringIO(newline="")
    annotation_io.write_annotations(f, ["falcon version x", "library_propagate = True"], blocks)
    want = ("# falcon version x\n# library_propagate = True\n#\n"
            "cluster,precursor_charge,family,hops,source_cluster,via_cluster,path_score,delta_mz,library_id,name,library_file,"
            "library_cosine,adduct,smiles,inchikey\n"
            '0,2,0,0,0,,1.0,0.0,CCMSLIB01,"Rutin, ""natural""",lib.mgf,0.91,[M+H]+,C1=CC,IKVR\n'
            '1,2,0,1,0,0,0.875,14.0157,CCMSLIB01,"Rutin, ""natural""",lib.mgf,0.91,[M+H]+,C1=CC,IKVR\n'
            '3,2,0,2,0,1,0.8,-2.5,CCMSLIB01,"Rutin, ""natural""",lib.mgf,0.91,[M+H]+,C1=CC,IKVR\n'
            "4,2,-1,0,4,,1.0,0.0,CCMSLIB02,Quercetin,lib.mgf,0.75,,O=C(O)C,\n"
            "7,None,2,1,5,5,0.75,1.5,CCMSLIB02,Quercetin,lib.mgf,0.8,,O=C(O)C,\n")
    assert f.getvalue() == want
    annotation_io.write(str(tmp_path / "o"), ["falcon version x", "library_propagate = True"], blocks)
    assert (tmp_path / "o.annotations.csv").read_bytes() == want.encode()


# ---- config ------------------------------------------------------------------------------------------------------------------------
FULL = "--library lib.mgf --network --network_families"


def test_propagate_options_and_parse_errors(capsys):
    from falcon_amd.config import Config
    c = Config()
    c.parse("in.mgf out " + FULL)
    assert c.library_propagate is False and (c.library_propagate_hops, c.library_propagate_min_score) == (3, 0.0)
    c.parse(f"in.mgf out {FULL} --library_propagate --library_propagate_hops 64 --library_propagate_min_score 1 "
            "--network_max_family_size 0")
    assert c.library_propagate is True and (c.library_propagate_hops, c.library_propagate_min_score) == (64, 1.0)
    for bad, text in (("--library_propagate", "--library_propagate needs --library"),
                      ("--library_propagate --network --network_families", "--library_propagate needs --library"),
                      ("--library_propagate --library lib.mgf", "--library_propagate needs --network --network_families"),
                      ("--library_propagate --library lib.mgf --network", "--library_propagate needs --network --network_families"),
                      (FULL + " --library_propagate --assign_to reps.mgf", "does not combine with --assign_to"),
                      (FULL + " --library_propagate --distributed", "does not combine with --distributed"),
                      (FULL + " --library_propagate --library_propagate_hops 0", "--library_propagate_hops 0 is outside [1, 64]"),
                      (FULL + " --library_propagate --library_propagate_hops 65", "--library_propagate_hops 65 is outside [1, 64]"),
                      ("--library_propagate_hops -1", "--library_propagate_hops -1 is outside [1, 64]"),
                      (FULL + " --library_propagate --library_propagate_min_score -0.1",
                       "--library_propagate_min_score -0.1 is outside [0, 1]"),
                      (FULL + " --library_propagate --library_propagate_min_score 1.5",
                       "--library_propagate_min_score 1.5 is outside [0, 1]"),
                      ("--library_propagate_min_score nan", "--library_propagate_min_score nan is outside [0, 1]")):
        with pytest.raises(SystemExit):
            c.parse("in.mgf out " + bad)
        assert text in capsys.readouterr().err, bad


def test_propagate_from_an_ini_file(tmp_path):
    from falcon_amd.config import Config
    ini = tmp_path / "falcon.ini"
    ini.write_text("library = lib.mgf\nnetwork = true\nnetwork_families = true\nlibrary_propagate = true\nlibrary_propagate_hops = 5\n"
                   "library_propagate_min_score = 0.25\n")
    c = Config()
    c.parse(f"-c {ini} in.mgf out")
    assert c.library_propagate is True and c.library_propagate_hops == 5 and c.library_propagate_min_score == 0.25
    c.parse(f"-c {ini} in.mgf out --library_propagate_hops 7")
    assert c.library_propagate_hops == 7 and c.library_propagate_min_score == 0.25
    ini.write_text("library_propagate = true\n")
    with pytest.raises(SystemExit):
        c.parse(f"-c {ini} in.mgf out")
    ini.write_text("library = lib.mgf\nnetwork = true\nnetwork_families = true\nlibrary_propagate = true\nlibrary_propagate_hops = 70\n")
    with pytest.raises(SystemExit):
        c.parse(f"-c {ini} in.mgf out")
    c.parse("in.mgf out")
    assert c.library_propagate is False and c.library_propagate_hops == 3


def test_the_propagate_lines_follow_the_library_lines_only_with_the_flag():
    from falcon_amd import falcon
    from falcon_amd.config import config
    config.parse("in.mgf out")
    base, header = falcon._option_lines(), falcon._header_lines()
    assert falcon._propagate_lines() == []
    config.parse(f"in.mgf out {FULL} --library_propagate_hops 5")
    net, fam, lib = falcon._network_lines(), falcon._family_lines(), falcon._library_lines()
    assert (len(net), len(fam), len(lib)) == (5, 3, 6) and falcon._propagate_lines() == []
    assert lib == ["library = lib.mgf", "library_analog = False", "library_max_shift = 200.000", "library_min_cosine = 0.700",
                   "library_min_matched_peaks = 6", "library_top_n = 1"]
    assert falcon._option_lines() == base + net + fam + lib
    config.parse(f"in.mgf out {FULL} --library_propagate --library_propagate_hops 5 --library_propagate_min_score 0.25")
    prop = ["library_propagate = True", "library_propagate_hops = 5", "library_propagate_min_score = 0.250"]
    assert falcon._propagate_lines() == prop
    assert (falcon._network_lines(), falcon._family_lines(), falcon._library_lines()) == (net, fam, lib)
    assert falcon._option_lines() == base + net + fam + lib + prop
    assert falcon._option_lines(header=True) == base and falcon._header_lines() == header
    config.parse(f"in.mgf out --cluster_summary {FULL} --library_propagate")
    assert falcon._option_lines() == base + ["cluster_summary = True"] + net + fam + lib + falcon._propagate_lines()
    assert len(falcon._propagate_lines()) == 3


def test_an_existing_annotations_file_stops_the_run_unless_overwrite(tmp_path):
    from falcon_amd import falcon
    from falcon_amd.config import config
    out = str(tmp_path / "run")
    open(out + ".annotations.csv", "w").close()
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} {FULL}")
    assert falcon._setup_work_dir() == (False, 0)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} {FULL} --library_propagate")
    assert falcon._setup_work_dir() == (False, 1)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} {FULL} --library_propagate --overwrite")
    assert falcon._setup_work_dir() == (False, 0)
    assert not (tmp_path / "run.annotations.csv").exists()
