"""Library search without a GPU: the host build of csrc/libsearch.h + csrc/netmatch.h against the numpy restatement
(tests/library_cases.py) on every case of the GPU tests, the window's superset property and the orientation at the float32 steps,
the annotation-library reader, `library_io`'s bytes, and the options' place in `config` and in the run's files.  Every comparison
with the restatement is on bits; every "at least" is asserted on the restatement's statistics."""
import io

import numpy as np
import pytest

from tests import hostbuild_library as hb
from tests import library_cases as lc
from tests import network_cases as nc

needs_compiler = pytest.mark.skipif(not hb.have_compiler(), reason="no host C++ compiler")
f32 = np.float32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hb.build(tmp_path_factory.mktemp("library_host"))


def check(lib, q, l, tol, r, min_cosine, min_matched, top_n, scored=None):
    """the host build == the restatement -> (hits, stats of the restatement)"""
    stats = {}
    scored = lc.score_pairs(q, l, tol, r) if scored is None else scored
    want = lc.hits_from(scored, min_cosine, min_matched, top_n, stats)
    got, counts = hb.search(lib, q, l, tol, r, min_cosine, min_matched, top_n)
    assert lc.same_hits(got, want), (len(got[0]), len(want[0]))
    assert counts.pop("outside_window") == 0
    for k, v in counts.items():
        assert stats[k] == v, (k, stats[k], v)
    return want, stats


# ---- analogue families ---------------------------------------------------------------------------------------------------------
@needs_compiler
@pytest.mark.parametrize("top_n", [0, 1, 3])
def test_analogue_families_both_orientations(lib, top_n):
    q, l = lc.analogue_case()
    a = lc.ANALOGUE
    r = lc.rule(True, max_shift=a["max_shift"])
    want, stats = check(lib, q, l, a["fragment_tol"], r, a["min_cosine"], a["min_matched"], top_n)
    assert len(q["rows"]) == 60 and len(l["rows"]) == 60
    assert stats["query_is_a"] >= 300 and stats["library_is_a"] >= 300, stats
    assert stats["greedy_pairs"] >= 100 and stats["rejected_cardinality"] >= 100 and stats["refused_pairs"] >= 100, stats
    assert stats["hits_below"] >= 10 and stats["hits_above"] >= 10 and stats["hits_near"] >= 10, stats
    if top_n == 0:
        assert stats["hits"] == stats["hits_before_top_n"] >= 150
    else:
        assert 0 < stats["hits"] < stats["hits_before_top_n"] and np.bincount(want[0]).max() == top_n
        d = np.diff(want[2].astype(np.float64))
        assert ((d <= 0) | (np.diff(want[0]) > 0)).all()                 # a query's hits fall in similarity


@needs_compiler
def test_analogue_families_exact_mode_is_the_plain_cosine(lib):
    q, l = lc.analogue_case()
    a = lc.ANALOGUE
    for r in (lc.rule(False, 100.0, False), lc.rule(False, 0.05, True)):
        scored = lc.score_pairs(q, l, a["fragment_tol"], r)
        assert len(scored) >= 30 and all(p["sim"] == p["sim_zero"] and p["matched"] == p["matched_zero"] for p in scored)
        _, stats = check(lib, q, l, a["fragment_tol"], r, a["min_cosine"], a["min_matched"], 0, scored)
        assert stats["hits"] >= 20 and stats["hits_below"] == stats["hits_above"] == 0, stats


@needs_compiler
def test_the_result_does_not_depend_on_the_order_of_either_side(lib):
    q, l = lc.analogue_case()
    a = lc.ANALOGUE
    r = lc.rule(True, max_shift=a["max_shift"])
    want = lc.search_ref(q, l, a["fragment_tol"], r, a["min_cosine"], a["min_matched"], 3)
    rng = np.random.default_rng(2)
    qp, lp = rng.permutation(60), rng.permutation(60)
    got, _ = hb.search(lib, lc.permute_side(q, qp), lc.permute_side(l, lp), a["fragment_tol"], r, a["min_cosine"], a["min_matched"], 0)
    back = lc.map_back(got, qp, lp)
    all_hits = lc.search_ref(q, l, a["fragment_tol"], r, a["min_cosine"], a["min_matched"], 0)
    assert lc.same_hits(back, all_hits)
    # distinct similarities inside every query: the first three do not depend on the library's numbering either
    got3, _ = hb.search(lib, lc.permute_side(q, qp), lc.permute_side(l, lp), a["fragment_tol"], r, a["min_cosine"], a["min_matched"], 3)
    assert lc.same_hits(lc.map_back(got3, qp, lp), want)


# ---- tiles, bands, scope ---------------------------------------------------------------------------------------------------------
TILE_CASES = [(nq, nl, band) for nq in lc.TILE_NQ for nl in lc.TILE_NL for band in lc.TILE_BANDS]


@needs_compiler
@pytest.mark.parametrize("nq,nl,band", TILE_CASES, ids=[f"{a}x{b}-{c}" for a, b, c in TILE_CASES])
def test_tile_edges(lib, nq, nl, band):
    q, l, max_shift = lc.tile_case(nq, nl, band)
    _, stats = check(lib, q, l, 0.05, lc.rule(True, max_shift=max_shift), 0.0, 0, 0)
    if band == "all":
        assert stats["in_scope"] == nq * nl
    if nq >= 63 and nl >= 64:
        assert stats["in_scope"] >= 100 and stats["hits"] >= stats["in_scope"] // 3, stats
        assert stats["query_is_a"] >= 50 and stats["library_is_a"] >= (0 if band == "equal" else 50), stats
        if band != "all":
            assert stats["in_scope"] < nq * nl


@needs_compiler
@pytest.mark.parametrize("mode", sorted(lc.ULP_RULES))
def test_scope_at_one_ulp_on_both_sides(lib, mode):
    q, l, r = lc.ulp_case(mode)
    want, stats = check(lib, q, l, 0.05, r, 0.0, 0, 0)
    assert stats["hits"] == stats["in_scope"]
    p0 = f32(500.0)
    lo_out, lo_in, hi_in, hi_out = lc.scope_ends(p0, r)
    lp, qp = l["precursor_mz"], q["precursor_mz"]
    pairs = set(zip(want[0].tolist(), want[1].tolist()))
    at = lambda x: set(np.flatnonzero(lp == x).tolist())
    for x in np.flatnonzero(qp == p0):
        assert all((x, y) in pairs for y in at(lo_in) | at(hi_in) | at(p0)) and not any((x, y) in pairs for y in at(lo_out) | at(hi_out))
    assert len(at(lo_in)) == len(at(hi_out)) == 3 and len(at(p0)) == 70
    assert not any(y in at(f32(300.0)) | at(f32(800.0)) for _, y in pairs)
    # the binary-searched range of the queries' tile: a superset that begins behind the far entries and ends inside a chunk
    lo, hi = hb.window(lib, qp.min(), qp.max(), r)
    ls = np.sort(lp).astype(np.float64)
    first, end = int(np.searchsorted(ls, lo, "left")), int(np.searchsorted(ls, hi, "right"))
    assert first == 10 and 76 <= end - first <= 82 and (end - first) % 64 != 0
    assert all(lo <= float(lp[y]) <= hi for _, y in pairs)


@needs_compiler
def test_the_window_is_a_superset_and_the_orientation_is_antisymmetric(lib):
    rng = np.random.default_rng(3)
    rules = list(lc.ULP_RULES.values()) + [lc.rule(True, max_shift=0.0), lc.rule(False, 0.0, True), lc.rule(False, 0.0, False),
                                           lc.rule(False, 2e6, False)]
    for r in rules:
        for pq in [f32(500.0), f32(137.03), f32(1999.9)] + list(rng.uniform(100.0, 2000.0, 5).astype(f32)):
            if r["analog"] or r["tol_is_da"] or 0 < r["precursor_tol"] < 1e6:
                ends = lc.scope_ends(pq, r) if (r["max_shift"] if r["analog"] else r["precursor_tol"]) > 0 else ()
            else:
                ends = ()
            w = hb.window(lib, pq, pq, r)
            for pl in list(ends) + [pq, np.nextafter(pq, f32(0)), np.nextafter(pq, f32(1e9))]:
                inside = lc.in_scope(pq, pl, r)
                assert bool(lib.t_in_scope(float(pq), float(pl), int(r["analog"]), r["precursor_tol"], int(r["tol_is_da"]),
                                           r["max_shift"])) == inside
                if inside and w is not None:
                    assert w[0] <= float(pl) <= w[1], (r, pq, pl, w)
    assert hb.window(lib, 500.0, 500.0, lc.rule(False, 2e6, False)) is None
    for pa, pb in ((500.0, 500.5), (500.0, float(np.nextafter(f32(500.0), f32(600)))), (137.03, 910.2)):
        assert lib.t_query_is_a(pa, pb) == 1 and lib.t_query_is_a(pb, pa) == 0
        assert lib.t_shift(1, pa, pb) == f32(f32(pa) - f32(pb)) < 0 and lib.t_shift(0, pa, pb) == 0.0
    assert lib.t_query_is_a(500.0, 500.0) == 1 and lib.t_shift(1, 500.0, 500.0) == 0.0           # equal precursors: the query is a


@needs_compiler
@pytest.mark.parametrize("top_n", [0, 2, 5])
def test_ties(lib, top_n):
    q, l = lc.tie_case()
    want, stats = check(lib, q, l, 0.05, lc.rule(True, max_shift=50.0), 0.5, 3, top_n)
    qt, lt = np.flatnonzero(q["precursor_mz"] == f32(600.0)), np.flatnonzero(l["precursor_mz"] == f32(600.0))
    assert len(qt) == 6 and len(lt) == 6 and stats["refused_pairs"] >= 30
    for x in qt:
        mine = [(y, s) for xq, y, s in zip(*want[:3]) if xq == x and y in lt]
        if top_n == 0:
            assert len(mine) == 6 and len({nc.bits(np.array([s], f32))[0] for _, s in mine}) == 1
        if top_n == 2:                                           # six equal hits a twin: the ranks go to the lower library indices
            assert [y for y, _ in mine] == sorted(lt.tolist())[:2]


# ---- large sides -------------------------------------------------------------------------------------------------------------------
@needs_compiler
def test_sides_above_a_strip(lib):
    q, l = lc.strip_case()
    _, stats = check(lib, q, l, 0.05, lc.rule(True, max_shift=10.0), 0.3, 6, 0)
    assert stats["greedy_pairs"] >= 300 and stats["hits"] >= 150 and stats["library_is_a"] >= 50 and stats["query_is_a"] >= 50, stats


@needs_compiler
@pytest.mark.parametrize("which", lc.LDS_SIDES)
def test_sides_above_the_lds_capacity(lib, which):
    q, l = lc.lds_case(which)
    peaks = lambda s: np.sort(np.diff(s["indptr"])[s["rows"]])[-64:].sum()
    assert (peaks(q) > 3200) == (which != "library") and (peaks(l) > 3200) == (which != "query")
    _, stats = check(lib, q, l, 0.05, lc.rule(True, max_shift=10.0), 0.0, 0, 4)
    assert stats["hits_before_top_n"] >= 300 and stats["hits"] == 4 * len(q["rows"]), stats


@needs_compiler
def test_the_peak_limit_counts_only_inside_the_scope(lib):
    q, l, max_shift = lc.limit_case(True)
    r = lc.rule(True, max_shift=max_shift)
    with pytest.raises(nc.Unsupported):
        lc.score_pairs(q, l, 0.05, r)
    assert hb.search(lib, q, l, 0.05, r, 0.0, 0, 0)[0] is None
    q, l, max_shift = lc.limit_case(False)
    _, stats = check(lib, q, l, 0.05, lc.rule(True, max_shift=max_shift), 0.0, 0, 0)
    assert stats["in_scope"] == 12 and stats["greedy_pairs"] >= 1 and stats["hits"] >= 6, stats


# ---- the reader --------------------------------------------------------------------------------------------------------------------
LIBRARY_TEXT = """# a GNPS-style library
BEGIN IONS
PEPMASS=315.1234
CHARGE=1+
MSLEVEL=2
IONMODE=Positive
NAME=Caffeine, "1,3,7-trimethylxanthine" M+H
SMILES=CN1C=NC2=C1C(=O)N(C(=O)N2C)C
INCHIKEY=RYYVLZVUVIJVGH-UHFFFAOYSA-N
ADDUCT=M+H
SPECTRUMID=CCMSLIB00000001
TITLE=ignored when there is a SPECTRUMID
110.07 12.5
138.066 100
195.0877 55.25
END IONS

BEGIN IONS
PEPMASS=0
NAME=no precursor
100.0 1.0
END IONS

BEGIN IONS
PEPMASS=401.5 1200.0
CHARGE=0
COMPOUND_NAME=chargeless compound
TITLE=entry-three
100.5 3
200.25 4
END IONS

BEGIN IONS
NAME=no pepmass at all
100.0 1.0
END IONS

BEGIN IONS
PEPMASS=500.0
NAME=bad peak
100.0 1.0
abc 2.0
END IONS

BEGIN IONS
PEPMASS=not-a-number
NAME=unparsable
100.0 1.0
END IONS

BEGIN IONS
PEPMASS=222.2
CHARGE=2-
150.0 9
END IONS
"""


def test_the_annotation_library_reader(tmp_path):
    from falcon_amd.ms_io import mgf_io
    fn = str(tmp_path / "gnps_like.mgf")
    open(fn, "w").write(LIBRARY_TEXT)
    counts = {}
    specs = mgf_io.read_annotation_library([fn], counts)
    assert counts == dict(entries=7, skipped=4) and len(specs) == 3
    a, b, c = specs
    assert a["identifier"] == "CCMSLIB00000001" and a["name"] == 'Caffeine, "1,3,7-trimethylxanthine" M+H'
    assert a["precursor_mz"] == 315.1234 and a["precursor_charge"] == 1 and a["filename"] == fn
    assert (a["adduct"], a["smiles"], a["inchikey"], a["ionmode"]) == ("M+H", "CN1C=NC2=C1C(=O)N(C(=O)N2C)C",
                                                                       "RYYVLZVUVIJVGH-UHFFFAOYSA-N", "Positive")
    assert a["mz"].tolist() == [110.07, 138.066, 195.0877] and a["intensity"].tolist() == [12.5, 100.0, 55.25]
    assert b["identifier"] == "entry-three" and b["name"] == "chargeless compound" and b["precursor_charge"] == 0
    assert b["precursor_mz"] == 401.5 and (b["adduct"], b["smiles"], b["inchikey"], b["ionmode"]) == ("", "", "", "")
    assert c["identifier"] == "gnps_like.mgf:7" and c["name"] == "" and c["precursor_charge"] == -2          # neither id nor title
    two = mgf_io.read_annotation_library([fn, fn])
    assert len(two) == 6 and [s["identifier"] for s in two[3:]] == [s["identifier"] for s in specs]
    # the readers beside it are what they were: they want a TITLE (and the representatives' reader a CLUSTER id)
    assert [s["identifier"] for s in mgf_io.get_spectra(fn)] == ["ignored when there is a SPECTRUMID", "entry-three"]
    with pytest.raises(mgf_io.MgfLibraryError):
        mgf_io.read_library([fn])


# ---- library_io ------------------------------------------------------------------------------------------------------------------
def test_library_io_bytes():
    from falcon_amd.ms_io import library_io
    text = lambda *a: np.array(a, dtype=str)
    lib = dict(library_id=text("CCMSLIB1", "x:2", "CCMSLIB3"), name=text('Caffeine, "1,3,7" M+H', "plain", ""),
               library_file=text("a.mgf", "a.mgf", "b.mgf"), adduct=text("M+H", "", "M+Na"), smiles=text("C,N", "", ""),
               inchikey=text("KEY-1", "", "KEY-3"), library_precursor_mz=np.array([195.0877, 401.5, 0.1 + 0.7], f32))
    blocks = [dict(lib, charge="2", first=0, cluster=np.array([0, 0, 3], np.int32), library=np.array([2, 0, 1], np.int32),
                   similarity=np.array([1.0, 0.75, 0.8125], f32), matched=np.array([12, 6, 7], np.int32),
                   delta_mz=np.array([0.0, 14.0157, -0.5], f32)),
              dict(lib, charge="3", first=4, cluster=np.zeros(0, np.int32), library=np.zeros(0, np.int32), similarity=np.zeros(0, f32),
                   matched=np.zeros(0, np.int32), delta_mz=np.zeros(0, f32)),
              dict(lib, charge="None", first=9, cluster=np.array([1], np.int32), library=np.array([0], np.int32),
                   similarity=np.array([0.1 + 0.7], f32), matched=np.array([9], np.int32), delta_mz=np.array([1e-3], f32))]
    f = io.StringIO(newline="")
    library_io.write_hits(f, ["falcon version x", "library = a.mgf b.mgf"], blocks)
    assert f.getvalue() == (
        "# falcon version x\n# library = a.mgf b.mgf\n#\n"
        "cluster,precursor_charge,rank,library_id,name,library_file,library_precursor_mz,delta_mz,cosine,matched_peaks,adduct,smiles,"
        "inchikey\n"
        "0,2,1,CCMSLIB3,,b.mgf,0.8,0.0,1.0,12,M+Na,,KEY-3\n"
        '0,2,2,CCMSLIB1,"Caffeine, ""1,3,7"" M+H",a.mgf,195.0877,14.0157,0.75,6,M+H,"C,N",KEY-1\n'
        "3,2,1,x:2,plain,a.mgf,401.5,-0.5,0.8125,7,,,\n"
        '10,None,1,CCMSLIB1,"Caffeine, ""1,3,7"" M+H",a.mgf,195.0877,0.001,0.8,9,M+H,"C,N",KEY-1\n')


# ---- config ----------------------------------------------------------------------------------------------------------------------
def test_library_options_and_parse_errors(capsys):
    from falcon_amd.config import Config
    c = Config()
    c.parse("in.mgf out")
    assert c.library is None and c.library_analog is False
    assert (c.library_max_shift, c.library_min_cosine, c.library_min_matched_peaks, c.library_top_n) == (200.0, 0.7, 6, 1)
    c.parse("in.mgf out --library a.mgf b.mgf --library_analog --library_max_shift 50 --library_min_cosine 0.6 "
            "--library_min_matched_peaks 4 --library_top_n 0 --network --exact")
    assert c.library == ["a.mgf", "b.mgf"] and c.library_analog is True
    assert (c.library_max_shift, c.library_min_cosine, c.library_min_matched_peaks, c.library_top_n) == (50.0, 0.6, 4, 0)
    for bad, text in (("--library a.mgf --assign_to reps.mgf", "--library does not combine with --assign_to"),
                      ("--library a.mgf --distributed", "--library does not combine with --distributed"),
                      ("--library_analog", "--library_analog needs --library"),
                      ("--library a.mgf --library_min_cosine 1.5", "--library_min_cosine 1.5 is outside [0, 1]"),
                      ("--library_min_cosine -0.1", "is outside [0, 1]"),
                      ("--library_min_matched_peaks -1", "--library_min_matched_peaks -1 is negative"),
                      ("--library_top_n -2", "--library_top_n -2 is negative"),
                      ("--library_max_shift -1", "--library_max_shift -1.0 is negative")):
        with pytest.raises(SystemExit):
            c.parse("in.mgf out " + bad)
        assert text in capsys.readouterr().err, bad
    c.parse("in.mgf out --library a.mgf --library_min_cosine 0 --library_max_shift 0 --library_min_matched_peaks 0")
    c.parse("in.mgf out --library a.mgf --library_min_cosine 1")


def test_library_from_an_ini_file(tmp_path):
    from falcon_amd.config import Config
    ini = tmp_path / "falcon.ini"
    ini.write_text("library = a.mgf b.mgf\nlibrary_analog = true\nlibrary_top_n = 3\nlibrary_max_shift = 42.5\n")
    c = Config()
    c.parse(f"-c {ini} in.mgf out")
    assert c.library == ["a.mgf", "b.mgf"] and c.library_analog is True and c.library_top_n == 3 and c.library_max_shift == 42.5
    assert c.library_min_cosine == 0.7
    c.parse(f"-c {ini} in.mgf out --library_top_n 7")
    assert c.library_top_n == 7
    ini.write_text("library = a.mgf\ndistributed = true\n")
    with pytest.raises(SystemExit):
        c.parse(f"-c {ini} in.mgf out")
    ini.write_text("library_analog = true\n")
    with pytest.raises(SystemExit):
        c.parse(f"-c {ini} in.mgf out")
    c.parse("in.mgf out")
    assert c.library is None


def test_the_log_lists_the_options_and_the_cluster_csv_header_does_not():
    from falcon_amd import falcon
    from falcon_amd.config import config
    config.parse("in.mgf out")
    base = falcon._option_lines()
    assert not any("library" in l for l in base) and falcon._option_lines(header=True) == base
    header = falcon._header_lines()
    config.parse("in.mgf out --library a.mgf b.mgf --library_analog --library_top_n 5")
    lib = ["library = a.mgf b.mgf", "library_analog = True", "library_max_shift = 200.000", "library_min_cosine = 0.700",
           "library_min_matched_peaks = 6", "library_top_n = 5"]
    assert falcon._option_lines() == base + lib and falcon._library_lines() == lib
    assert falcon._option_lines(header=True) == base and falcon._header_lines() == header
    config.parse("in.mgf out --network --library a.mgf")
    assert falcon._option_lines() == base + falcon._network_lines() + falcon._library_lines()


def test_an_existing_library_file_stops_the_run_unless_overwrite(tmp_path):
    from falcon_amd import falcon
    from falcon_amd.config import config
    out = str(tmp_path / "run")
    open(out + ".library.csv", "w").close()
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'}")
    assert falcon._setup_work_dir() == (False, 0)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} --library a.mgf")
    assert falcon._setup_work_dir() == (False, 1)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} --library a.mgf --overwrite")
    assert falcon._setup_work_dir() == (False, 0)
    assert not (tmp_path / "run.library.csv").exists()
