"""Molecular families without a GPU: the host build of csrc/netfamily.h against the numpy restatement (tests/family_cases.py) on
every case of the GPU tests, the restatement's own invariants, `network_io`'s bytes for a two-block example, and the options'
place in `config` and in the run's files.  Every comparison with the restatement is on bits; every "at least" is asserted on the
restatement's statistics (family_cases.expected)."""
import io

import numpy as np
import pytest

from tests import family_cases as fc
from tests import hostbuild_family as hb

needs_compiler = pytest.mark.skipif(not hb.have_compiler(), reason="no host C++ compiler")
f32, i32 = np.float32, np.int32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hb.build(tmp_path_factory.mktemp("family_host"))


# ---- the header ------------------------------------------------------------------------------------------------------------------
@needs_compiler
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_the_host_build_is_the_restatement(lib, name):
    g, max_size, delta, _ = fc.CASES[name]
    want = fc.expected(name)
    got = hb.families(lib, g, max_size, delta)
    assert fc.same(got, want) and got["n_cut"] == want["n_cut"], (got["n_families"], want["n_families"], got["n_rounds"], want["n_rounds"])


@needs_compiler
@pytest.mark.parametrize("name", sorted(fc.invalid_cases()))
def test_the_host_build_refuses_what_the_restatement_refuses(lib, name):
    g, max_size, delta = fc.invalid_cases()[name]
    assert not fc.valid(g["n"], g["u"], g["v"], g["sim"], max_size, delta)
    assert hb.families(lib, g, max_size, delta) is None


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
# The tests of this part check the reference itself -- the numpy restatement and the case table of tests/family_cases.py -- not
# the library: they need neither the header nor the options, and pass wherever family_cases.py is present.
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_no_surviving_component_is_above_the_cap_and_the_numbering_follows_the_roots(name):
    g, max_size, delta, _ = fc.CASES[name]
    res = fc.expected(name)
    alive = res["round"] == 0
    root = fc.components(g["n"], g["u"][alive], g["v"][alive])
    size = np.bincount(root, minlength=g["n"])[root]
    assert np.array_equal(size, res["size"]) and (max_size == 0 or size.max() <= max_size)
    assert np.array_equal(res["family"] >= 0, size >= 2)
    roots = np.flatnonzero((root == np.arange(g["n"])) & (size >= 2))
    assert np.array_equal(res["family"][roots], np.arange(len(roots))) and np.array_equal(res["family"], np.where(size >= 2, res["family"][root], -1))
    assert res["n_families"] == len(roots) and res["n_rounds"] == (res["round"].max() if len(alive) else 0) == len(res["cut_per_round"])
    # a cut edge's round is one in which its component was above the cap: cutting rounds are consecutive from 1
    assert sorted(set(res["round"].tolist()) - {0}) == list(range(1, res["n_rounds"] + 1))


def test_a_component_at_the_cap_is_untouched_and_one_above_it_is_cut():
    for k in (2, 3, 17, 64):
        g = fc.chain(k)
        at = fc.families(g["n"], g["u"], g["v"], g["sim"], k, 0.0)
        assert at["n_cut"] == 0 and at["n_rounds"] == 0 and at["n_families"] == 1 and (at["size"] == k).all()
        above = fc.families(g["n"], g["u"], g["v"], g["sim"], k - 1, 0.0)
        assert above["n_cut"] == 1 and above["round"][np.argmin(g["sim"])] == 1 and above["largest"] <= k - 1
    res = fc.expected("edge-values")              # both in one graph: sizes 4, 3, 4 under cap 3
    assert res["round"][3:5].tolist() == [0, 0] and res["round"][5:].tolist() == [1, 1, 1]


def test_node_permutation_and_edge_order_change_nothing():
    g, max_size, delta, _ = fc.CASES["random-300"]
    want = fc.expected("random-300")
    h, pick = fc.shuffled(g, duplicates=40)
    got = fc.families(h["n"], h["u"], h["v"], h["sim"], max_size, delta)
    assert np.array_equal(got["family"], want["family"]) and np.array_equal(got["size"], want["size"])
    assert np.array_equal(got["round"], want["round"][pick]) and got["n_rounds"] == want["n_rounds"]
    assert fc.same(got, fc.expected("duplicates-shuffled"))
    p, perm = fc.permuted(g)
    got = fc.expected("permuted")
    assert np.array_equal(got["round"], want["round"]) and np.array_equal(got["size"][perm], want["size"])
    assert fc.family_sets(got) == {frozenset(perm[list(s)].tolist()) for s in fc.family_sets(want)}
    assert got["n_families"] == want["n_families"] and got["n_rounds"] == want["n_rounds"]


def test_rounds_stay_below_the_stated_bound_with_a_positive_delta():
    for name in ("random-300", "random-5000", "star-cap-100"):
        g, _, delta, _ = fc.CASES[name]
        bound = int(np.floor((float(g["sim"].max()) - float(g["sim"].min())) / delta)) + 1
        assert 1 <= fc.expected(name)["n_rounds"] <= bound <= 16, (name, bound)


# ---- network_io --------------------------------------------------------------------------------------------------------------------
def _blocks():
    return [dict(charge="2", first=0, a=np.array([0, 2], i32), b=np.array([1, 3], i32), similarity=np.array([0.75, 1.0], f32),
                 matched=np.array([6, 12], i32), delta_mz=np.array([14.0157, 0.0], f32), family=np.array([0, 1], i32),
                 node_family=np.array([0, 0, 1, 1, -1], i32), node_size=np.array([2, 2, 2, 2, 1], i32), n_families=2),
            dict(charge="None", first=5, a=np.array([1], i32), b=np.array([2], i32), similarity=np.array([0.1 + 0.7], f32),
                 matched=np.array([7], i32), delta_mz=np.array([-0.5], f32), family=np.array([0], i32),
                 node_family=np.array([-1, 0, 0], i32), node_size=np.array([1, 2, 2], i32), n_families=1)]


def test_family_io_bytes_for_two_blocks():
    from falcon_amd.ms_io import network_io
    header = ["falcon version x", "network = True", "network_families = True"]
    f = io.StringIO(newline="")
    network_io.write_network_with_families(f, header, _blocks())
    assert f.getvalue() == ("# falcon version x\n# network = True\n# network_families = True\n#\n"
                            "cluster_a,cluster_b,precursor_charge,delta_mz,cosine,matched_peaks,family\n"
                            "0,1,2,14.0157,0.75,6,0\n2,3,2,0.0,1.0,12,1\n6,7,None,-0.5,0.8,7,2\n")
    f = io.StringIO(newline="")
    network_io.write_families(f, header, _blocks())
    assert f.getvalue() == ("# falcon version x\n# network = True\n# network_families = True\n#\n"
                            "cluster,precursor_charge,family,family_size\n"
                            "0,2,0,2\n1,2,0,2\n2,2,1,2\n3,2,1,2\n4,2,-1,1\n5,None,-1,1\n6,None,2,2\n7,None,2,2\n")


def test_write_network_is_what_it_was(tmp_path):
    from falcon_amd.ms_io import network_io
    network_io.write(str(tmp_path / "o"), ["h"], _blocks())
    assert (tmp_path / "o.network.csv").read_text() == ("# h\n#\ncluster_a,cluster_b,precursor_charge,delta_mz,cosine,matched_peaks\n"
                                                         "0,1,2,14.0157,0.75,6\n2,3,2,0.0,1.0,12\n6,7,None,-0.5,0.8,7\n")
    assert not (tmp_path / "o.families.csv").exists()
    network_io.write_with_families(str(tmp_path / "o"), ["h"], _blocks())
    assert (tmp_path / "o.network.csv").read_text().splitlines()[3].endswith("6,0")
    assert len((tmp_path / "o.families.csv").read_text().splitlines()) == 2 + 1 + 8


# ---- config ------------------------------------------------------------------------------------------------------------------------
def test_family_options_and_parse_errors(capsys):
    from falcon_amd.config import Config
    c = Config()
    c.parse("in.mgf out --network")
    assert c.network_families is False and (c.network_max_family_size, c.network_family_delta) == (100, 0.02)
    c.parse("in.mgf out --network --network_families --network_max_family_size 0 --network_family_delta 0")
    assert c.network_families is True and (c.network_max_family_size, c.network_family_delta) == (0, 0.0)
    for bad, text in (("--network_families", "--network_families needs --network"),
                      ("--network --network_families --assign_to reps.mgf", "--network does not combine with --assign_to"),
                      ("--network --network_families --distributed", "--network does not combine with --distributed"),
                      ("--network --network_families --network_max_family_size -1", "--network_max_family_size -1 is negative"),
                      ("--network_max_family_size -5", "--network_max_family_size -5 is negative"),
                      ("--network --network_families --network_family_delta -0.01", "--network_family_delta -0.01 is negative"),
                      ("--network_family_delta nan", "--network_family_delta nan is negative")):
        with pytest.raises(SystemExit):
            c.parse("in.mgf out " + bad)
        assert text in capsys.readouterr().err, bad


def test_families_from_an_ini_file(tmp_path):
    from falcon_amd.config import Config
    ini = tmp_path / "falcon.ini"
    ini.write_text("network = true\nnetwork_families = true\nnetwork_max_family_size = 30\nnetwork_family_delta = 0.05\n")
    c = Config()
    c.parse(f"-c {ini} in.mgf out")
    assert c.network_families is True and c.network_max_family_size == 30 and c.network_family_delta == 0.05
    c.parse(f"-c {ini} in.mgf out --network_max_family_size 7")
    assert c.network_max_family_size == 7 and c.network_family_delta == 0.05
    ini.write_text("network_families = true\n")
    with pytest.raises(SystemExit):
        c.parse(f"-c {ini} in.mgf out")
    c.parse("in.mgf out")
    assert c.network_families is False and c.network_max_family_size == 100


def test_the_family_lines_follow_the_network_lines_only_with_the_flag():
    from falcon_amd import falcon
    from falcon_amd.config import config
    config.parse("in.mgf out")
    base, header = falcon._option_lines(), falcon._header_lines()
    assert falcon._family_lines() == []
    config.parse("in.mgf out --network --network_max_family_size 30")
    net = falcon._network_lines()
    assert len(net) == 5 and falcon._family_lines() == [] and falcon._option_lines() == base + net
    config.parse("in.mgf out --network --network_families --network_max_family_size 30 --network_family_delta 0.05")
    fam = ["network_families = True", "network_max_family_size = 30", "network_family_delta = 0.050"]
    assert falcon._family_lines() == fam and falcon._network_lines() == net
    assert falcon._option_lines() == base + net + fam
    assert falcon._option_lines(header=True) == base and falcon._header_lines() == header
    config.parse("in.mgf out --cluster_summary --network --network_families")
    assert falcon._option_lines() == base + ["cluster_summary = True"] + net + falcon._family_lines()


def test_an_existing_families_file_stops_the_run_unless_overwrite(tmp_path):
    from falcon_amd import falcon
    from falcon_amd.config import config
    out = str(tmp_path / "run")
    open(out + ".families.csv", "w").close()
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} --network")
    assert falcon._setup_work_dir() == (False, 0)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} --network --network_families")
    assert falcon._setup_work_dir() == (False, 1)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} --network --network_families --overwrite")
    assert falcon._setup_work_dir() == (False, 0)
    assert not (tmp_path / "run.families.csv").exists()
