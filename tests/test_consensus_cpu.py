"""Consensus representatives without a GPU: the numpy restatement pinned to hand-computed clusters, the host build of
`csrc/consensus.h` (the header the kernels include) bit for bit against the restatement, and the two command-line options."""
import numpy as np
import pytest

from tests import consensus_cases as cc
from tests import hostbuild_consensus as hb


def _csr(spectra):
    mz = np.concatenate([np.asarray(s[0], np.float32) for s in spectra])
    it = np.concatenate([np.asarray(s[1], np.float32) for s in spectra])
    indptr = np.zeros(len(spectra) + 1, np.int64)
    np.cumsum([len(s[0]) for s in spectra], out=indptr[1:])
    return mz, it, indptr


def _one_cluster(spectra, medoid, tol, q):
    mz, it, indptr = _csr(spectra)
    ptr, omz, oit, st = cc.consensus_reference(mz, it, indptr, np.zeros(len(spectra), np.int32), np.array([medoid], np.int32), tol, q)
    assert ptr.tolist() == [0, len(omz)]
    return omz, oit, int(st[0])


def _same(a, literal):
    return np.array_equal(cc.bits(a), cc.bits(np.array(literal, np.float32)))


# ---- hand-computed clusters (all inputs exact in float32 unless said otherwise) --------------------------------------------
def test_shared_and_private_peak():
    """members {100 (0.5), 200 (0.25)} and {100.03125 (1)}, tolerance 0.05: groups {100, 100.03125} and {200}.
    q = 0.5: need = ceil(0.5 * 2) = 1, both kept.  Group 1: W = 1.5, M = 50 + 100.03125 = 150.03125, m/z = float32(100.0208333..)
    = 100.02083587646484, raw = 1.5 / 2 = 0.75; group 2: m/z 200, raw = 0.25 / 2 = 0.125.  N = 0.5625 + 0.015625 = 0.578125:
    0.75 / sqrt(N) = 0.98639392..., 0.125 / sqrt(N) = 0.16439898...
    q = 1: need = 2, the private peak's group (1 peak) is dropped: one peak, intensity 0.75 / sqrt(0.5625) = 1."""
    members = [([100.0, 200.0], [0.5, 0.25]), ([100.03125], [1.0])]
    mz, it, st = _one_cluster(members, 0, 0.05, 0.5)
    assert st == 0 and _same(mz, [100.02083587646484, 200.0]) and _same(it, [0.986393928527832, 0.16439898312091827])
    assert np.float32(150.03125 / 1.5) == mz[0] and np.float32(0.75 / np.sqrt(0.578125)) == it[0]
    mz, it, st = _one_cluster(members, 0, 0.05, 1.0)
    assert st == 0 and _same(mz, [100.02083587646484]) and _same(it, [1.0])


def test_zero_intensity_group():
    """{300 (0), 500 (1)} and {300.03125 (0), 500 (0.5)}: the group at 300 has W = 0, so its m/z is the plain mean 300.015625
    and its intensity 0; the group at 500: raw 0.75, N = 0.5625, intensity 1.  A cluster whose every peak is 0 keeps its
    groups with intensity 0 (N = 0) and is no fallback."""
    mz, it, st = _one_cluster([([300.0, 500.0], [0.0, 1.0]), ([300.03125, 500.0], [0.0, 0.5])], 1, 0.05, 0.5)
    assert st == 0 and _same(mz, [300.015625, 500.0]) and _same(it, [0.0, 1.0])
    mz, it, st = _one_cluster([([300.0], [0.0]), ([300.03125], [0.0])], 1, 0.05, 0.5)
    assert st == 0 and _same(mz, [300.015625]) and _same(it, [0.0])


def test_chain_of_three_peaks():
    """100, 100.04, 100.08 (float32: 100.04000091552734, 100.08000183105469) at tolerance 0.05: both gaps are 0.0400009 <= 0.05, so
    the three peaks chain into ONE group 0.08 wide.  q = 1, m = 3: need 3, support 3, kept; m/z = the intensity-weighted mean
    = 100.04000091552734, raw = 3 / 3 = 1, intensity 1."""
    members = [([100.0], [1.0]), ([100.04], [1.0]), ([100.08], [1.0])]
    mz, it, st = _one_cluster(members, 1, 0.05, 1.0)
    assert st == 0 and _same(mz, [100.04000091552734]) and _same(it, [1.0])
    # at tolerance 0.03 the chain breaks into three groups of one peak: need 3 > 1, nothing kept -> the medoid
    mz, it, st = _one_cluster(members, 1, 0.03, 1.0)
    assert st == cc.FALLBACK and _same(mz, [100.04]) and _same(it, [1.0])


def test_fallback_and_singleton():
    """disjoint members at q = 1: no group holds 2 peaks -> the medoid's peaks verbatim (not normalised, not sorted), status
    FALLBACK; a cluster of one member is that member, status 0"""
    members = [([100.0, 150.0], [0.6, 0.8]), ([120.0], [1.0])]
    mz, it, st = _one_cluster(members, 0, 0.05, 1.0)
    assert st == cc.FALLBACK and _same(mz, [100.0, 150.0]) and _same(it, [0.6, 0.8])
    mz, it, st = _one_cluster([([180.0, 120.0], [0.3, 0.0])], 0, 0.05, 0.25)
    assert st == 0 and _same(mz, [180.0, 120.0]) and _same(it, [0.3, 0.0])


def test_support_counts_peaks_not_members():
    """one member with two peaks inside the tolerance, another without any: m = 2, q = 1 -> need 2, support min(2, 2) = 2: kept"""
    mz, it, st = _one_cluster([([100.0, 100.03125], [0.5, 0.5]), ([], [])], 0, 0.05, 1.0)
    assert st == 0 and _same(mz, [100.015625]) and _same(it, [1.0])


# ---- the header the kernels include, built for the host ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not hb.have_compiler():
        pytest.skip("no host C++ compiler and no hipcc")
    return hb.build(tmp_path_factory.mktemp("cons"))


def _check(lib, part, tol, q):
    ref = cc.consensus_reference(part["mz"], part["intensity"], part["indptr"], part["labels"], part["medoids"], tol, q)
    got = hb.consensus(lib, part["mz"], part["intensity"], part["indptr"], part["labels"], part["medoids"], tol, q)
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[3], got[3])
    assert np.array_equal(cc.bits(ref[1]), cc.bits(got[1])), "m/z bits"
    assert np.array_equal(cc.bits(ref[2]), cc.bits(got[2])), "intensity bits"
    return ref


def test_host_build_pins_the_hand_cases(lib):
    from falcon_amd import _lib
    assert lib.t_cons_lds_peaks() == _lib.CONS_LDS_PEAKS
    mz, it, indptr = _csr([([100.0, 200.0], [0.5, 0.25]), ([100.03125], [1.0]), ([300.0], [0.0]), ([300.03125], [0.0])])
    got = hb.consensus(lib, mz, it, indptr, np.array([0, 0, 1, 1]), np.array([0, 3]), 0.05, 0.5)
    assert got[0].tolist() == [0, 2, 3] and got[3].tolist() == [0, 0]
    assert _same(got[1], [100.02083587646484, 200.0, 300.015625]) and _same(got[2], [0.986393928527832, 0.16439898312091827, 0.0])


@pytest.mark.parametrize("q", [0.01, 0.25, 0.5, 1.0])
@pytest.mark.parametrize("tol", [0.05, 0.0])
def test_host_build_equals_the_restatement_bit_for_bit(lib, tol, q):
    """cluster sizes 1 .. 300, duplicate m/z across and within members, members without peaks, zero-intensity groups"""
    rng = np.random.default_rng(int(q * 100) * 7 + int(tol * 100))
    sizes = np.concatenate([np.arange(1, 40), rng.integers(40, 301, 12), [300, 2, 1]])
    part = cc.make_partition(rng, sizes, peaks=(1, 12), p_empty=0.15, p_zero=0.1)
    ref = _check(lib, part, tol, q)
    kept = np.diff(ref[0])
    assert (kept > 0).any() and (ref[3] == 0).any()
    if q == 1.0 and tol == 0.0:
        assert (ref[3] == cc.FALLBACK).any()


def test_host_build_all_fallback_and_empty_clusters(lib):
    rng = np.random.default_rng(5)
    part = cc.make_partition(rng, [2, 3, 7, 40], peaks=(1, 6), disjoint=True)
    ref = _check(lib, part, 0.05, 1.0)
    assert (ref[3] == cc.FALLBACK).all()
    ip = part["indptr"]
    for c, med in enumerate(part["medoids"]):
        assert np.array_equal(ref[1][ref[0][c]:ref[0][c + 1]], part["mz"][ip[med]:ip[med + 1]])
    # every member empty: nothing to group -> the (empty) medoid, FALLBACK
    part = cc.make_partition(rng, [3, 1], p_empty=1.0)
    ref = _check(lib, part, 0.05, 0.25)
    assert ref[0].tolist() == [0, 0, 0] and ref[3].tolist() == [cc.FALLBACK, 0]


def test_restatement_does_not_depend_on_row_order_without_m_z_ties():
    """without equal m/z inside a cluster the pooled order is the m/z order alone: permuting the dataset rows changes no bit"""
    rng = np.random.default_rng(11)
    part = cc.make_partition(rng, [1, 2, 5, 30, 120], grid_jitter=False)
    perm = cc.permute_rows(part, rng)
    a = cc.consensus_reference(part["mz"], part["intensity"], part["indptr"], part["labels"], part["medoids"], 0.05, 0.25)
    b = cc.consensus_reference(perm["mz"], perm["intensity"], perm["indptr"], perm["labels"], perm["medoids"], 0.05, 0.25)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- the designed cases: each reaches its decision on the restatement alone, and the header agrees ---------------------------
def _reference(case):
    p = case["part"]
    return cc.consensus_reference(p["mz"], p["intensity"], p["indptr"], p["labels"], p["medoids"], case["tol"], case["q"])


@pytest.mark.parametrize("name", list(cc.DECISION_CASES))
def test_decision_case_shows_its_witness(name):
    from falcon_amd import _lib
    assert cc.CUT == _lib.CONS_LDS_PEAKS
    case = cc.DECISION_CASES[name]()
    case["witness"](_reference(case))


@pytest.mark.parametrize("name", list(cc.DECISION_CASES))
def test_host_build_equals_the_restatement_on_the_decision_cases(lib, name):
    case = cc.DECISION_CASES[name]()
    _check(lib, case["part"], case["tol"], case["q"])


def test_restatement_ignores_labels_and_medoids_outside_the_partition():
    """rows labelled -1 or >= n_clusters belong to no cluster whatever they hold; a medoid outside [0, n) copies nothing"""
    mz, it, indptr = _csr([([100.0], [1.0]), ([100.0], [1.0]), ([200.0], [1.0]), ([300.0], [1.0])])
    ref = cc.consensus_reference(mz, it, indptr, np.array([-1, 0, 5, 0], np.int32), np.array([4, 4, -1], np.int32), 0.05, 1.0)
    assert ref[0].tolist() == [0, 0, 0, 0] and ref[3].tolist() == [cc.FALLBACK] * 3        # {100}, {300}: no group of two
    ref = cc.consensus_reference(mz, it, indptr, np.array([-1, 0, 5, 0], np.int32), np.array([2, 4, -1], np.int32), 0.05, 0.5)
    assert ref[0].tolist() == [0, 2, 2, 2] and _same(ref[1], [100.0, 300.0]) and ref[3].tolist() == [0, cc.FALLBACK, cc.FALLBACK]


@pytest.mark.parametrize("builder", [cc.lds_turns, cc.flat_turns], ids=["lds_turns", "flat_turns"])
def test_turn_case_gathered_from_its_library_is_the_restatement_of_the_whole(builder):
    """at a nominal 2 CUs: the expected output gathered from the library's equals the restatement run on every cluster of the
    case, and the case meets its turn conditions"""
    part, pick, cond = builder(2)
    assert all(cond.values()), cond
    lib = (cc.lds_turns_library if builder is cc.lds_turns else cc.flat_turns_library)()[0]
    want = cc.gather_expected(_reference(dict(part=lib, tol=0.05, q=0.25)), pick)
    ref = _reference(dict(part=part, tol=0.05, q=0.25))
    assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[3], want[3])
    assert np.array_equal(cc.bits(ref[1]), cc.bits(want[1])) and np.array_equal(cc.bits(ref[2]), cc.bits(want[2]))
    assert (ref[3] == cc.FALLBACK).any() and (np.diff(ref[0]) > 1).any()


# ---- options ---------------------------------------------------------------------------------------------------------------
def _parse(args):
    from falcon_amd.config import Config
    c = Config()
    c.parse(args)
    return c


def test_option_defaults():
    c = _parse("in.mgf out")
    assert c.representatives == "medoid" and c.consensus_min_fraction == 0.25 and c.export_representatives is False
    c = _parse("in.mgf out --export_representatives --representatives consensus --consensus_min_fraction 0.5")
    assert c.representatives == "consensus" and c.consensus_min_fraction == 0.5


def test_options_from_ini(tmp_path):
    ini = tmp_path / "falcon.ini"
    ini.write_text("export_representatives = true\nrepresentatives = consensus\nconsensus_min_fraction = 0.4\n")
    c = _parse(f"in.mgf out -c {ini}")
    assert c.representatives == "consensus" and c.consensus_min_fraction == 0.4 and c.export_representatives is True
    c = _parse(f"in.mgf out -c {ini} --consensus_min_fraction 1.0")            # the command line wins
    assert c.consensus_min_fraction == 1.0
    ini.write_text("export_representatives = true\nrepresentatives = mean\n")
    with pytest.raises(SystemExit):
        _parse(f"in.mgf out -c {ini}")


@pytest.mark.parametrize("args", [
    "in.mgf out --representatives consensus",                                                    # nothing to export them to
    "in.mgf out --export_representatives --representatives consensus --consensus_min_fraction 0",
    "in.mgf out --export_representatives --representatives consensus --consensus_min_fraction 1.5",
    "in.mgf out --consensus_min_fraction -0.25",
    "in.mgf out --export_representatives --representatives mean",
])
def test_parse_errors(args, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(args)
    assert e.value.code == 2
    capsys.readouterr()


def test_option_lines_change_only_with_consensus():
    from falcon_amd import falcon
    from falcon_amd.config import config
    config.parse("in.mgf out --export_representatives")
    base = falcon._option_lines()
    assert len(base) == 28 and not any("consensus" in x or x.startswith("representatives") for x in base)
    config.parse("in.mgf out --export_representatives --representatives medoid --consensus_min_fraction 0.5")
    assert falcon._option_lines() == base
    config.parse("in.mgf out --export_representatives --representatives consensus")
    lines = falcon._option_lines()
    assert lines[:28] == base and lines[28:] == ["representatives = consensus", "consensus_min_fraction = 0.250"]
