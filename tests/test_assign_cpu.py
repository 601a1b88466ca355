"""Assigning new spectra to representatives, without a GPU: the numpy restatement `assign_cases.assign_ref` against cases
computed by hand, the host build of csrc/assignrep.h (the per-pair test, the window pre-filter and the key) against the
restatement, the `--assign_to` option, the library reader, and the scoring kernel's resources."""
import os

import numpy as np
import pytest

from tests import assign_cases as ac
from tests import hostbuild_assign as hb

f32 = np.float32
E = np.zeros(0, f32)


def unit(*xs):
    x = np.asarray(xs, np.float64)
    return (x / np.sqrt(np.sum(x * x))).astype(f32)


# ---- the restatement against hand-computed cases ----------------------------------------------------------------------------
A_MZ, B_MZ, C_MZ = [200.0, 300.0, 400.0], [200.0, 300.0, 500.0], [250.0, 350.0, 450.0]


def small_library():
    """three entries: A at 500.0, B at 500.004 (8 ppm above), C at 600.0"""
    return ac.side([A_MZ, B_MZ, C_MZ], [unit(1, 1, 1)] * 3, [500.0, 500.004, 600.0], [10.0, 20.0, 30.0])


def test_three_entry_library_and_five_queries():
    lib = small_library()
    q = ac.side([A_MZ,                      # 0: an exact copy of A, at A's precursor
                 B_MZ,                      # 1: B's peaks at A's precursor: A and B are candidates, B is nearer
                 C_MZ,                      # 2: C's peaks at C's precursor: one candidate
                 A_MZ,                      # 3: A's peaks at 550: no candidate
                 [200.0, 777.0, 888.0]],    # 4: shares one peak with A and B
                [unit(1, 1, 1)] * 5, [500.0, 500.0, 600.0, 550.0, 500.002], [10.0] * 5)
    row, dist, cand = ac.assign_ref(q, lib, 20.0, "ppm", None, 0.05, 0)
    third = f32(1.0 - float(f32(unit(1, 1, 1)[0]) * f32(unit(1, 1, 1)[0])))          # one matched peak of three
    two = f32(1.0 - 2 * float(f32(unit(1, 1, 1)[0]) * f32(unit(1, 1, 1)[0])))
    assert list(cand) == [2, 2, 1, 0, 2]
    assert list(row) == [0, 1, 2, -1, 0]                                              # query 4: A and B tie, A has the lower m/z
    assert dist[0] < 1e-6 and dist[1] < 1e-6 and dist[2] < 1e-6 and dist[3] == 1.0 and dist[4] == third
    # the copy scores its own peaks; against the other entry two of three peaks match
    assert ac.pair_dist(q, 0, lib, 1, 0.05, 0) == two
    assert dist.dtype == f32 and row.dtype == np.int32 and cand.dtype == np.int32


def test_ties_lower_precursor_then_lower_row():
    same = [A_MZ, A_MZ, A_MZ]
    lib = ac.side(same, [unit(1, 1, 1)] * 3, [500.004, 500.0, 500.004])
    q = ac.side([A_MZ], [unit(1, 1, 1)], [500.002])
    assert list(ac.assign_ref(q, lib, 20.0, "ppm", None, 0.05, 0)[0]) == [1]           # the lower m/z wins, not the lower row
    lib = ac.side(same, [unit(1, 1, 1)] * 3, [500.0, 500.0, 500.0])
    assert list(ac.assign_ref(q, lib, 20.0, "ppm", None, 0.05, 0)[0]) == [0]           # equal m/z: the lower row


@pytest.mark.parametrize("mode,tol", [("ppm", 20.0), ("Da", 0.05)])
def test_one_ulp_inside_and_outside_the_bound(mode, tol):
    l_pmz = f32(612.3456)
    lo_out, lo_in, hi_in, hi_out = ac.ulp_bounds(l_pmz, tol, mode)
    assert np.nextafter(lo_out, f32(np.inf), dtype=f32) == lo_in and np.nextafter(hi_in, f32(np.inf), dtype=f32) == hi_out
    bound = tol if mode == "Da" else tol * 1e-6 * float(l_pmz)
    ulp = float(np.spacing(l_pmz))                                       # the edge lies within two float32 steps of the bound
    assert abs(float(l_pmz) - float(lo_in)) == pytest.approx(bound, abs=2 * ulp)
    assert abs(float(hi_in) - float(l_pmz)) == pytest.approx(bound, abs=2 * ulp)
    lib = ac.side([A_MZ], [unit(1, 1, 1)], [l_pmz])
    q = ac.side([A_MZ] * 4, [unit(1, 1, 1)] * 4, [lo_out, lo_in, hi_in, hi_out])
    row, dist, cand = ac.assign_ref(q, lib, tol, mode, None, 0.05, 0)
    assert list(cand) == [0, 1, 1, 0] and list(row) == [-1, 0, 0, -1] and dist[0] == 1.0 and dist[3] == 1.0


def test_rt_exclusion_min_matches_and_no_candidate():
    lib = small_library()
    q = ac.side([A_MZ], [unit(1, 1, 1)], [500.0], [10.0])
    # RT: A (rt 10) stays, B (rt 20) is 10 away
    assert list(ac.assign_ref(q, lib, 20.0, "ppm", 5.0, 0.05, 0)[2]) == [1]
    assert list(ac.assign_ref(q, lib, 20.0, "ppm", 10.0, 0.05, 0)[2]) == [2]            # the bound is inclusive
    q2 = ac.side([A_MZ], [unit(1, 1, 1)], [500.0], [16.0])
    assert list(ac.assign_ref(q2, lib, 20.0, "ppm", 5.0, 0.05, 0)[0]) == [1]            # only B is left
    # min_matched_peaks: three matched peaks are enough for 3, not for 4 -- then d = 1, still a candidate
    row, dist, cand = ac.assign_ref(q, lib, 20.0, "ppm", None, 0.05, 3)
    assert row[0] == 0 and dist[0] < 1e-6
    row, dist, cand = ac.assign_ref(q, lib, 20.0, "ppm", None, 0.05, 4)
    assert list(row) == [0] and dist[0] == 1.0 and cand[0] == 2
    # no candidate / empty library / a spectrum without peaks
    far = ac.side([A_MZ], [unit(1, 1, 1)], [700.0])
    assert [list(x) for x in ac.assign_ref(far, lib, 20.0, "ppm", None, 0.05, 0)] == [[-1], [1.0], [0]]
    none = ac.side([], [], [])
    assert [list(x) for x in ac.assign_ref(q, none, 20.0, "ppm", None, 0.05, 0)] == [[-1], [1.0], [0]]
    bare = ac.side([E], [E], [500.0])
    row, dist, cand = ac.assign_ref(bare, lib, 20.0, "ppm", None, 0.05, 0)
    assert list(row) == [0] and dist[0] == 1.0 and cand[0] == 2


# ---- the host build of assignrep.h ------------------------------------------------------------------------------------------
needs_cc = pytest.mark.skipif(not hb.have_compiler(), reason="no host C++ compiler")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hb.build(tmp_path_factory.mktemp("assign_host"))


def random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    l = rng.uniform(200, 1500, n).astype(f32)
    # a third of the pairs far apart, the rest within a few tolerances of the bound
    ppm = np.where(rng.random(n) < 0.33, rng.uniform(-500, 500, n), rng.normal(0, 20, n))
    q = (l.astype(np.float64) * (1 + ppm * 1e-6)).astype(f32)
    return q, l, rng.uniform(0, 100, n).astype(f32), rng.uniform(0, 100, n).astype(f32)


@needs_cc
@pytest.mark.parametrize("mode,tol", [("ppm", 20.0), ("Da", 0.02), ("ppm", 5.0)])
def test_predicate_of_the_header_equals_the_restatement(lib, mode, tol):
    q, l, q_rt, l_rt = random_pairs(10000, 11)
    edges = [ac.ulp_bounds(x, tol, mode) for x in (f32(300.25), f32(612.3456), f32(1499.9))]
    q = np.concatenate([q, np.concatenate(edges).astype(f32)])
    l = np.concatenate([l, np.repeat([f32(300.25), f32(612.3456), f32(1499.9)], 4).astype(f32)])
    q_rt, l_rt = np.concatenate([q_rt, np.zeros(12, f32)]), np.concatenate([l_rt, np.zeros(12, f32)])
    for rt_tol in (None, 30.0):
        want = np.array([ac.is_candidate(a, b, tol, mode, rt_tol, c, d) for a, b, c, d in zip(q, l, q_rt, l_rt)])
        got = hb.candidates(lib, q, l, tol, mode, rt_tol, q_rt, l_rt)
        assert np.array_equal(got, want)
        assert 300 < want.sum() < len(want) - 1000                      # both answers occur
    assert list(hb.candidates(lib, q[-12:], l[-12:], tol, mode)) == [False, True, True, False] * 3


@needs_cc
@pytest.mark.parametrize("mode,tol", [("ppm", 20.0), ("Da", 0.02), ("ppm", 5.0), ("Da", 3.0)])
def test_window_of_the_header_holds_every_candidate(lib, mode, tol):
    """the pre-filter is a superset: whatever run of queries a tile holds, a candidate's precursor lies inside its range"""
    q, l, _, _ = random_pairs(10000, 12)
    ok = hb.candidates(lib, q, l, tol, mode)
    for k in np.flatnonzero(ok):
        lo, hi = hb.window(lib, q[k], q[k], tol, mode)
        assert lo <= float(l[k]) <= hi
    for x in (f32(300.25), f32(612.3456), f32(1499.9)):
        lo_out, lo_in, hi_in, hi_out = ac.ulp_bounds(x, tol, mode)
        for qq in (lo_in, hi_in):
            lo, hi = hb.window(lib, qq, qq, tol, mode)
            assert lo <= float(x) <= hi
    # ... and not much wider than the rule (the walk is priced by it)
    lo, hi = hb.window(lib, 600.0, 600.0, tol, mode)
    width = tol if mode == "Da" else 600.0 * tol * 1e-6
    assert (hi - lo) <= 2 * width * 1.001
    assert hb.window(lib, 600.0, 600.0, 1e6, "ppm") is None and hb.window(lib, -1.0, 600.0, 20.0, "ppm") is None


@needs_cc
def test_key_order_round_trip_and_empty_key(lib):
    rng = np.random.default_rng(13)
    d = np.concatenate([rng.random(10000).astype(f32), rng.choice([0.0, 1.0, 0.25], 2000).astype(f32), [f32(0.0), f32(1.0)]])
    pos = rng.integers(0, 2 ** 31 - 1, len(d)).astype(np.uint32)
    pos[:3000] = rng.integers(0, 8, 3000)                                  # equal (d, pos) pairs occur
    keys = hb.pack(lib, d, pos)
    d2, pos2 = hb.unpack(lib, keys)
    assert np.array_equal(d2.view(np.uint32), d.view(np.uint32)) and np.array_equal(pos2, pos)
    # the order of the keys is the restatement's lexsort on (d, rank)
    assert np.array_equal(np.sort(keys), keys[np.lexsort((pos, d))])
    empty = np.uint64(lib.t_empty_key())
    assert (keys < empty).all() and hb.pack(lib, [1.0], [2 ** 32 - 1])[0] < empty
    assert hb.pack(lib, [-0.0], [5])[0] == hb.pack(lib, [0.0], [5])[0]


def same(got, ref):
    return (np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.int32), ref[1].view(np.int32))
            and np.array_equal(got[2], ref[2]))


@needs_cc
@pytest.mark.parametrize("name", list(ac.TEMPLATE_PARAMS))
def test_host_walk_equals_the_restatement_on_the_template_spectra(lib, name):
    """the kernels' walk (sorted sides, tiles, pre-filter range, per-pair test, key minimum) through the header on the host"""
    q, l = ac.template_split()
    st = {}
    ref = ac.assign_ref(q, l, *ac.TEMPLATE_PARAMS[name], stats=st)
    for tile in (64, 7):
        *got, err, walked = hb.assign(lib, q, l, *ac.TEMPLATE_PARAMS[name], tile=tile)
        assert same(got, ref) and not err and walked >= st["pairs"]
    assert st["solver_pairs"] >= 100 and st["solver_winners"] >= 10


@needs_cc
def test_host_walk_on_edges_ties_and_unsupported_pairs(lib):
    for nq, nl in ((1, 1), (65, 64), (130, 200), (70, 0), (0, 70)):
        q, l = ac.ladder_case(nq, nl)
        for tol, mode, rt in ((20.0, "ppm", None), (0.01, "Da", 25.0), (2e6, "ppm", None)):
            *got, err, walked = hb.assign(lib, q, l, tol, mode, rt, 0.05, 0)
            assert same(got, ac.assign_ref(q, l, tol, mode, rt, 0.05, 0)) and not err
        # the range is a pre-filter, not the whole library: a 20 ppm window on a 5 ppm ladder
        walked = hb.assign(lib, q, l, 20.0, "ppm", None, 0.05, 0, tile=1)[4]
        assert walked <= 10 * nq
    q, l = ac.tie_case()
    assert same(hb.assign(lib, q, l, 20.0, "ppm", None, 0.05, 0)[:3], ac.assign_ref(q, l, 20.0, "ppm", None, 0.05, 0))
    q, l, tol = ac.unsupported_case(inside=True)
    assert hb.assign(lib, q, l, 20.0, "ppm", None, tol, 0)[3]
    q, l, tol = ac.unsupported_case(inside=False)
    *got, err, _ = hb.assign(lib, q, l, 20.0, "ppm", None, tol, 0)
    assert not err and same(got, ac.assign_ref(q, l, 20.0, "ppm", None, tol, 0))


# ---- the option ----------------------------------------------------------------------------------------------------------------
def test_assign_to_parses_one_and_several_files_and_refuses_distributed(capsys):
    from falcon_amd.config import Config
    c = Config()
    c.parse(["in.mgf", "out"])
    assert c.assign_to is None
    c.parse(["in.mgf", "out", "--assign_to", "a.mgf"])
    assert c.assign_to == ["a.mgf"] and c.input_filenames == ["in.mgf"] and c.output_filename == "out"
    c.parse(["in1.mgf", "in2.mgf", "out", "--assign_to", "a.mgf", "b.mgf", "--eps", "0.2"])
    assert c.assign_to == ["a.mgf", "b.mgf"] and c.input_filenames == ["in1.mgf", "in2.mgf"] and c.eps == 0.2
    with pytest.raises(SystemExit):
        c.parse(["in.mgf", "out", "--assign_to", "a.mgf", "--distributed"])
    assert "--assign_to does not combine with --distributed" in capsys.readouterr().err


def test_the_option_line_appears_only_when_chosen():
    from falcon_amd import falcon
    from falcon_amd.config import config
    config.parse(["in.mgf", "out"])
    plain = falcon._option_lines()
    assert not any("assign_to" in l for l in plain)
    config.parse(["in.mgf", "out", "--assign_to", "a.mgf", "b.mgf"])
    lines = falcon._option_lines()
    assert lines[:len(plain)] == plain and lines[len(plain):] == ["assign_to = a.mgf b.mgf"]


# ---- the library reader --------------------------------------------------------------------------------------------------------
def write_reps(path, ids, title="rep", drop_cluster=None, bad=None):
    from falcon_amd.ms_io import mgf_io
    specs = [{"identifier": f"{title}{k}", "precursor_mz": 500.0 + k, "precursor_charge": 2, "retention_time": 1.5 * k,
              "mz": np.array([200.0, 300.0 + k]), "intensity": np.array([0.6, 0.8], f32), "cluster": c}
             for k, c in enumerate(ids)]
    mgf_io.write_spectra(str(path), specs)
    if drop_cluster is not None or bad is not None:
        text = open(path).read()
        if drop_cluster is not None:
            text = text.replace(f"CLUSTER={ids[drop_cluster]}\n", "", 1)
        if bad is not None:
            text = text.replace(f"CLUSTER={ids[bad]}\n", "CLUSTER=seven\n", 1)
        open(path, "w").write(text)
    return specs


def test_library_reader_returns_the_ids_and_get_spectra_is_unchanged(tmp_path):
    from falcon_amd.ms_io import mgf_io
    fn = tmp_path / "a.mgf"
    write_reps(fn, [7, 0, 42])
    plain = list(mgf_io.get_spectra(str(fn)))
    got = list(mgf_io.get_library_spectra(str(fn)))
    assert [s["cluster"] for s in got] == [7, 0, 42]
    assert len(plain) == 3 and all("cluster" not in s for s in plain)
    for a, b in zip(plain, got):
        assert set(b) == set(a) | {"cluster"}
        for k in a:
            assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]
    # several files, in order
    fn2 = tmp_path / "b.mgf"
    write_reps(fn2, [43, 44], title="more")
    both = mgf_io.read_library([str(fn), str(fn2)])
    assert [s["cluster"] for s in both] == [7, 0, 42, 43, 44] and both[3]["filename"] == str(fn2)


def test_missing_bad_and_duplicate_cluster_ids_raise(tmp_path):
    from falcon_amd.ms_io import mgf_io
    a, b, c, d = (tmp_path / n for n in ("a.mgf", "b.mgf", "c.mgf", "d.mgf"))
    write_reps(a, [1, 2, 3])
    write_reps(b, [4, 2], title="other")
    with pytest.raises(mgf_io.MgfLibraryError, match=r"b\.mgf.*other1.*CLUSTER=2.*a\.mgf"):
        mgf_io.read_library([str(a), str(b)])
    write_reps(c, [5, 6, 7], drop_cluster=1)
    with pytest.raises(mgf_io.MgfLibraryError, match=r"c\.mgf: entry 2 \(TITLE=rep1\) has no CLUSTER="):
        mgf_io.read_library([str(c)])
    write_reps(d, [5, 6, 7], bad=2)
    with pytest.raises(mgf_io.MgfLibraryError, match=r"d\.mgf: entry 3 .*CLUSTER=seven is not an integer"):
        mgf_io.read_library([str(d)])
    write_reps(d, [5, 5])
    with pytest.raises(mgf_io.MgfLibraryError, match="repeats CLUSTER=5"):
        mgf_io.read_library([str(d)])


# ---- kernel resources ----------------------------------------------------------------------------------------------------------
LDS_BYTES = 53264           # DESIGN.md "Assigning to representatives": 2 sides x 3,200 peaks x 8 B + the staging tables


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from tests import isa_lint as L
    if not os.path.exists(L.HIPCC):
        pytest.skip("hipcc not available")
    return L.compile_to_asm("assignrep.hip", tmp_path_factory.mktemp("isa"))


def test_scoring_kernel_uses_no_scratch_and_the_stated_lds(asm):
    from tests import isa_lint as L
    scratch = {k: v for k, v in L.kernel_meta(asm, "private_segment_fixed_size").items() if "assign_" in k}
    assert sum("assign_score_kernel" in k for k in scratch) == 1 and len(scratch) == 3, sorted(scratch)
    assert [v for k, v in scratch.items() if "assign_score_kernel" in k] == [0]
    assert [v for k, v in scratch.items() if "assign_unpack_kernel" in k] == [0]
    lds = [v for k, v in L.kernel_meta(asm, "group_segment_fixed_size").items() if "assign_score_kernel" in k]
    assert len(lds) == 1 and 51200 <= lds[0] <= LDS_BYTES
    assert 3 * lds[0] <= 160 * 1024                                      # three workgroups per compute unit
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    assert f"{LDS_BYTES:,} B" in design


def test_no_lds_dma_in_the_assign_kernels(asm):
    from tests import isa_lint as L
    for name, body in L.kernels(asm).items():
        if "assign_" in name:
            assert not any("global_load_lds" in s or (s.startswith("buffer_load") and " lds" in s) for s in body), name
