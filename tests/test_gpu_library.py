"""Library search on the device (`fal_library_search`) against the numpy restatement of tests/library_cases.py: every comparison
is on bits, in values and order; every "at least" is asserted on the restatement's statistics.  Analogue families searched in
both orientations (the greedy kernels' pair count against the count from the inputs), the self-search that reproduces the
network, tile edges, the scope at one ulp on both sides of a query, ties, large sides and the peak limit, `max_hits`, the order
of either side, the public function and `main()` with `--library`.

The strip case lists more large-sided pairs than the list of its one tile holds before the host has seen a count: it takes the
second run.  No test overflows the small-sided list or the hit buffer (4 M entries)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import library_cases as lc
from tests import network_cases as nc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIDE = ("mz", "intensity", "indptr", "rows", "precursor_mz")


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def gpu_hits(ctx, q, l, tol, r, min_cosine, min_matched, top_n, max_hits=None):
    out = ctx.library_search(*(q[k] for k in SIDE), *(l[k] for k in SIDE), tol, r["precursor_tol"], r["tol_is_da"], r["analog"],
                             r["max_shift"], min_cosine, min_matched, top_n, max_hits=max_hits)
    return tuple(t.cpu().numpy() for t in out)


def check(ctx, q, l, tol, r, min_cosine, min_matched, top_n, scored=None):
    """the device == the restatement, the greedy kernels' pairs included -> (hits, stats of the restatement)"""
    stats = {}
    scored = lc.score_pairs(q, l, tol, r) if scored is None else scored
    want = lc.hits_from(scored, min_cosine, min_matched, top_n, stats)
    got = gpu_hits(ctx, q, l, tol, r, min_cosine, min_matched, top_n)
    assert lc.same_hits(got, want), (len(got[0]), len(want[0]))
    assert ctx.counter(14) == stats["greedy_pairs"], (ctx.counter(14), stats)
    return want, stats


# ---- analogue families ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def analogue():
    q, l = lc.analogue_case()
    a = lc.ANALOGUE
    r = lc.rule(True, max_shift=a["max_shift"])
    return q, l, r, lc.score_pairs(q, l, a["fragment_tol"], r)


def check_analogue(ctx, analogue, top_n):
    q, l, r, scored = analogue
    a = lc.ANALOGUE
    _, stats = check(ctx, q, l, a["fragment_tol"], r, a["min_cosine"], a["min_matched"], top_n, scored)
    assert stats["query_is_a"] >= 300 and stats["library_is_a"] >= 300 and stats["greedy_pairs"] >= 100, stats
    assert stats["hits_below"] >= 10 and stats["hits_above"] >= 10 and stats["hits_near"] >= 10, stats
    assert ctx.counter(14) > 0
    return stats


@pytest.mark.parametrize("top_n", [0, 1, 3])
def test_analogue_families_both_orientations(ctx, analogue, top_n):
    check_analogue(ctx, analogue, top_n)


@pytest.mark.parametrize("top_n", [0, 1, 3])
@pytest.mark.parametrize("form", ["ppm", "da"])
def test_analogue_families_exact_mode(ctx, form, top_n):
    q, l = lc.analogue_case()
    a = lc.ANALOGUE
    r = lc.rule(False, 100.0, False) if form == "ppm" else lc.rule(False, 0.05, True)
    _, stats = check(ctx, q, l, a["fragment_tol"], r, a["min_cosine"], a["min_matched"], top_n)
    assert stats["hits"] >= 20 and stats["hits_below"] == stats["hits_above"] == 0 and stats["greedy_pairs"] >= 10, stats


def test_self_search_reproduces_the_network(ctx):
    nodes = nc.analogue_case()
    a = nc.ANALOGUE
    assert len(set(nodes["precursor_mz"].tolist())) == 120
    u, v, sim, matched = (t.cpu().numpy() for t in ctx.network_edges(*(nodes[k] for k in SIDE), a["fragment_tol"], a["max_shift"],
                                                                     a["min_cosine"], a["min_matched"], 0))
    assert len(u) >= 300
    got = gpu_hits(ctx, nodes, nodes, a["fragment_tol"], lc.rule(True, max_shift=a["max_shift"]), a["min_cosine"], a["min_matched"], 0)
    other = got[0] != got[1]
    own = {int(x) for x in got[0][~other]}
    assert own == {int(x) for x, n in enumerate(np.diff(nodes["indptr"])[nodes["rows"]]) if n >= a["min_matched"]}
    have = {(int(x), int(y)): (nc.bits(np.array([s], f32))[0], int(m)) for x, y, s, m in zip(*(g[other] for g in got))}
    want = {}
    for x, y, s, m in zip(u, v, sim, matched):
        want[(int(x), int(y))] = want[(int(y), int(x))] = (nc.bits(np.array([s], f32))[0], int(m))
    assert have == want and len(have) == 2 * len(u) == int(other.sum())


def test_the_result_does_not_depend_on_the_order_of_either_side(ctx, analogue):
    q, l, r, scored = analogue
    a = lc.ANALOGUE
    rng = np.random.default_rng(2)
    qp, lp = rng.permutation(60), rng.permutation(60)
    for top_n in (0, 3):
        want = lc.hits_from(scored, a["min_cosine"], a["min_matched"], top_n)
        got = gpu_hits(ctx, lc.permute_side(q, qp), lc.permute_side(l, lp), a["fragment_tol"], r, a["min_cosine"], a["min_matched"], top_n)
        assert lc.same_hits(lc.map_back(got, qp, lp), want)


# ---- tiles, bands, scope ---------------------------------------------------------------------------------------------------------
TILE_CASES = [(nq, nl, band) for nq in lc.TILE_NQ for nl in lc.TILE_NL for band in lc.TILE_BANDS]


def check_tile(ctx, nq, nl, band):
    q, l, max_shift = lc.tile_case(nq, nl, band)
    _, stats = check(ctx, q, l, 0.05, lc.rule(True, max_shift=max_shift), 0.0, 0, 0)
    if nq >= 63 and nl >= 64:
        assert stats["in_scope"] >= 100 and stats["hits"] >= stats["in_scope"] // 3, stats


@pytest.mark.parametrize("nq,nl,band", TILE_CASES, ids=[f"{a}x{b}-{c}" for a, b, c in TILE_CASES])
def test_tile_edges(ctx, nq, nl, band):
    check_tile(ctx, nq, nl, band)


@pytest.mark.parametrize("mode", sorted(lc.ULP_RULES))
def test_scope_at_one_ulp_on_both_sides(ctx, mode):
    q, l, r = lc.ulp_case(mode)
    _, stats = check(ctx, q, l, 0.05, r, 0.0, 0, 0)
    assert stats["hits"] == stats["in_scope"] and 4 * 70 + 3 * 6 <= stats["in_scope"] <= 4 * 76, stats
    check(ctx, q, l, 0.05, r, 0.0, 0, 3)


@pytest.mark.parametrize("top_n", [0, 2, 5])
def test_ties(ctx, top_n):
    q, l = lc.tie_case()
    _, stats = check(ctx, q, l, 0.05, lc.rule(True, max_shift=50.0), 0.5, 3, top_n)
    assert stats["refused_pairs"] >= 30
    check(ctx, q, l, 0.05, lc.rule(False, 0.0, True), 0.5, 3, top_n)          # equal precursors only: the query is a


# ---- large sides -------------------------------------------------------------------------------------------------------------------
def check_large(ctx):
    q, l = lc.strip_case()
    _, stats = check(ctx, q, l, 0.05, lc.rule(True, max_shift=10.0), 0.3, 6, 0)
    assert stats["greedy_pairs"] >= 300 and stats["hits"] >= 150, stats           # (more large pairs than 4,096 / 16: the second run)
    for which in lc.LDS_SIDES:
        q, l = lc.lds_case(which)
        _, stats = check(ctx, q, l, 0.05, lc.rule(True, max_shift=10.0), 0.0, 0, 4)
        assert stats["hits_before_top_n"] >= 300, stats


def test_sides_above_a_strip_and_above_the_lds_capacity(ctx):
    check_large(ctx)


def test_the_peak_limit_counts_only_inside_the_scope_and_the_context_stays_usable(ctx):
    from falcon_amd._lib import FalconHipError
    q, l, max_shift = lc.limit_case(True)
    with pytest.raises(FalconHipError, match="code -5.*more than 4096 peaks"):
        gpu_hits(ctx, q, l, 0.05, lc.rule(True, max_shift=max_shift), 0.0, 0, 0)
    q, l, max_shift = lc.limit_case(False)
    _, stats = check(ctx, q, l, 0.05, lc.rule(True, max_shift=max_shift), 0.0, 0, 0)
    assert stats["in_scope"] == 12 and stats["greedy_pairs"] >= 1 and stats["hits"] >= 6, stats


def test_a_row_outside_either_csr_is_an_error(ctx):
    from falcon_amd._lib import FalconHipError
    q, l, max_shift = lc.tile_case(65, 65, "all")
    r = lc.rule(True, max_shift=max_shift)
    for side in ("q", "l"):
        s = q if side == "q" else l
        bad = dict(s, rows=s["rows"].copy())
        bad["rows"][7] = len(s["indptr"]) - 1
        with pytest.raises(FalconHipError, match="code -1.*outside"):
            gpu_hits(ctx, bad if side == "q" else q, bad if side == "l" else l, 0.05, r, 0.0, 0, 0)
    check(ctx, q, l, 0.05, r, 0.0, 0, 0)


# ---- max_hits ----------------------------------------------------------------------------------------------------------------------
def test_max_hits_and_an_empty_side(ctx, analogue):
    import torch
    q, l, r, scored = analogue
    a = lc.ANALOGUE
    want = lc.hits_from(scored, a["min_cosine"], a["min_matched"], 3)
    m_true = len(want[0])
    types = (torch.float32, torch.float32, torch.int64, torch.int32, torch.float32)
    dq = [ctx.to_dev(q[k], t) for k, t in zip(SIDE, types)]
    dl = [ctx.to_dev(l[k], t) for k, t in zip(SIDE, types)]

    def call(room, nq=60, nl=60):
        out = [ctx.empty((max(room, 1),), t) for t in (torch.int32, torch.int32, torch.float32, torch.int32)]
        for t in out:
            t.fill_(-7)
        m = C.c_int64(-1)
        rc = ctx.lib.fal_library_search(ctx._h, *(ctx._p(t) for t in dq[:3]), len(q["indptr"]) - 1, ctx._p(dq[3]), ctx._p(dq[4]), nq,
                                        *(ctx._p(t) for t in dl[:3]), len(l["indptr"]) - 1, ctx._p(dl[3]), ctx._p(dl[4]), nl,
                                        a["fragment_tol"], 20.0, 0, 1, a["max_shift"], a["min_cosine"], a["min_matched"], 3,
                                        *(ctx._p(t) for t in out), room, C.byref(m))
        ctx.sync()
        return rc, m.value, tuple(t.cpu().numpy() for t in out)

    rc, m, out = call(m_true - 1)
    assert rc == -1 and m == m_true and all((o == -7).all() for o in out)           # FAL_EINVAL, nothing written
    rc, m, out = call(m)
    assert rc == 0 and m == m_true and lc.same_hits(tuple(o[:m] for o in out), want)
    for nq, nl in ((0, 60), (60, 0), (0, 0)):
        rc, m, out = call(4, nq, nl)
        assert rc == 0 and m == 0 and all((o == -7).all() for o in out) and ctx.counter(14) == 0
    # the wrapper asks again with the room the library reported
    assert lc.same_hits(gpu_hits(ctx, q, l, a["fragment_tol"], r, a["min_cosine"], a["min_matched"], 3, max_hits=3), want)


# ---- scratch hygiene -------------------------------------------------------------------------------------------------------------
def test_cases_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 (scratch filled with 0xFF before use, a slot that grows while a pointer into it is held fails) is
    read once per process: a fresh child runs the analogue, tile and large-side cases again"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "library_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the public function -----------------------------------------------------------------------------------------------------------
def test_cluster_library_search_with_medoid_and_consensus_peaks(ctx):
    from falcon_amd.cluster import cluster as fc
    from tests import consensus_cases as cc
    from tests import memberscore_cases as mc
    case, _ = mc.tile_case(130, "interleaved", seed=3)
    rng = np.random.default_rng(4)
    n_members = len(case["labels"])
    # many small clusters of the same spectra, so that the representatives and the library are related: labels = row mod 40
    labels = (np.arange(n_members) % 40).astype(np.int32)
    medoids = np.array([rng.choice(np.flatnonzero(labels == c)) for c in range(40)], np.int32)
    pmz = (500.0 + rng.uniform(0.0, 30.0, n_members)).astype(f32)
    ds = fc.SpectrumDataset(pmz, case["retention_time"], case["mz"], case["intensity"], case["indptr"])
    # the library: 50 of the members as spectra of a CSR of their own, at precursors near their own
    pick = rng.choice(n_members, 50, replace=False)
    members = dict(mz=case["mz"], intensity=case["intensity"], indptr=case["indptr"], rows=np.arange(n_members, dtype=np.int32))
    l_side = nc.make_nodes([nc.peaks(members, int(v)) for v in pick], (pmz[pick] + rng.uniform(-8.0, 8.0, 50)).astype(f32))
    lds = fc.SpectrumDataset(l_side["precursor_mz"], None, l_side["mz"], l_side["intensity"], l_side["indptr"])
    pipe = fc.ClusterPipeline(ctx)
    cons = cc.consensus_reference(case["mz"], case["intensity"], case["indptr"], labels, medoids, 0.05, 0.25)[:3]
    for consensus in (None, cons):
        if consensus is None:
            q = dict(mz=case["mz"], intensity=case["intensity"], indptr=case["indptr"], rows=medoids)
        else:
            q = dict(mz=consensus[1], intensity=consensus[2], indptr=consensus[0], rows=np.arange(40, dtype=np.int32))
        q["precursor_mz"] = pmz[medoids]
        for r, mode, top_n in ((lc.rule(True, max_shift=20.0), "ppm", 3), (lc.rule(False, 3.0, True), "Da", 1),
                               (lc.rule(False, 4000.0, False), "ppm", 1)):
            stats = {}
            want = lc.search_ref(q, l_side, 0.05, r, 0.1, 2, top_n, stats)
            assert stats["hits"] >= 15 and stats["hits"] < stats["hits_before_top_n"], stats
            out = fc.library_search(ds, medoids, lds, 0.05, r["precursor_tol"], mode, analog=r["analog"], max_shift=r["max_shift"],
                                    min_cosine=0.1, min_matched_peaks=2, top_n=top_n, consensus=consensus, pipeline=pipe)
            assert lc.same_hits((out["cluster"], out["library"], out["similarity"], out["matched"]), want)
            assert nc.same(out["delta_mz"], (q["precursor_mz"][want[0]] - l_side["precursor_mz"][want[1]]).astype(f32))


# ---- main() ------------------------------------------------------------------------------------------------------------------------
LIBRARY_ARGS = ["--library_min_cosine", "0.5", "--library_min_matched_peaks", "4", "--library_top_n", "2", "--library_max_shift", "60"]
PLANTED = 14.0157


def _write_run_and_library(mgf, lib_mgf):
    """six templates of 30 peaks (charges 2 and 3 in turn), each with two noisy copies at nearly its precursor (they cluster with
    it) -> the input MGF; and the GNPS-style library: for templates 0-3 the analogue at +14.0157 (about half of the peaks move
    along) with the template's charge, for templates 4 and 5 the compound itself at the template's precursor without a charge,
    one unrelated entry, and one entry without a precursor"""
    from falcon_amd.ms_io import ms_io
    rng = np.random.default_rng(12)
    specs, lines = [], []
    for t in range(6):
        mz, it = np.sort(rng.uniform(150.0, 850.0, 30)), rng.uniform(100.0, 1e4, 30)
        moves = rng.permutation(30) < 15
        pmz, charge = 940.0 + 3.0 * t, 2 + t % 2
        for c in range(3):
            m = mz + rng.normal(0.0, 0.002, 30)
            o = np.argsort(m)
            specs.append({"identifier": f"scan={len(specs) + 1}", "precursor_mz": pmz * (1.0 + rng.normal(0, 1e-6)),
                          "precursor_charge": charge, "retention_time": float(np.round(rng.uniform(0.0, 3600.0), 3)),
                          "mz": m[o], "intensity": (it * rng.uniform(0.9, 1.1, 30))[o].astype(np.float32)})
        shift = PLANTED if t < 4 else 0.0
        lm = mz + moves * shift
        o = np.argsort(lm)
        lines += ["BEGIN IONS", f"PEPMASS={pmz + shift:.4f}"] + ([f"CHARGE={charge}+"] if t < 4 else ["CHARGE=0"] if t == 4 else [])
        lines += [f'NAME=Compound {t}, "form {t}" M+H', f"SPECTRUMID=CCMSLIB{t:08d}", "ADDUCT=M+H", f"INCHIKEY=KEY-{t}", "IONMODE=Positive"]
        lines += [f"{a:.4f} {b:.2f}" for a, b in zip(lm[o], (0.01 * it)[o])] + ["END IONS", ""]
    um = np.sort(rng.uniform(150.0, 850.0, 30))
    lines += ["BEGIN IONS", "PEPMASS=946.0", "NAME=unrelated", "TITLE=decoy"] + [f"{a:.4f} 10.0" for a in um] + ["END IONS", ""]
    lines += ["BEGIN IONS", "PEPMASS=0", "NAME=no precursor", "100.0 1.0", "END IONS", ""]
    ms_io.write_spectra(mgf, [specs[i] for i in rng.permutation(len(specs))])
    open(lib_mgf, "w").write("\n".join(lines))


def _expected_library(out, work, header, analog):
    """the library file's text from the run's own partitions, the cluster CSV's labels, the exported representatives' titles and
    the libraries the run left in its work directory"""
    import io
    import json
    from falcon_amd.ms_io import library_io
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
        ref = np.load(os.path.join(work, "spectra", f"reference_charge_{charge}.npz"))
        glob = np.array([cluster_of[str(i)] for i in z["identifier"]], np.int64)
        first = int(glob.min())
        row_of = {str(t): i for i, t in enumerate(z["identifier"])}
        medoids = np.array([row_of[title_of[c + first]] for c in range(int(glob.max()) - first + 1)], np.int32)
        q = dict(mz=z["mz"], intensity=z["intensity"], indptr=z["indptr"], rows=medoids, precursor_mz=z["precursor_mz"][medoids])
        l = dict(mz=ref["mz"], intensity=ref["intensity"], indptr=ref["indptr"], rows=np.arange(len(ref["precursor_mz"]), dtype=np.int32),
                 precursor_mz=ref["precursor_mz"])
        c, r, sim, matched = lc.search_ref(q, l, 0.05, lc.rule(analog, 20.0, False, 60.0), 0.5, 4, 2)
        b = dict(charge=charge, first=first, cluster=c, library=r, similarity=sim, matched=matched,
                 delta_mz=(q["precursor_mz"].astype(f32)[c] - l["precursor_mz"].astype(f32)[r]).astype(f32),
                 library_precursor_mz=ref["precursor_mz"])
        b.update({k: ref[k] for k in ("library_id", "name", "library_file", "adduct", "smiles", "inchikey")})
        blocks.append((first, b, ref))
    blocks.sort(key=lambda x: x[0])
    f = io.StringIO(newline="")
    library_io.write_hits(f, header, [b for _, b, _ in blocks])
    return f.getvalue(), [b for _, b, _ in blocks], [ref for _, _, ref in blocks]


@pytest.mark.parametrize("analog", [False, True], ids=["exact", "analog"])
def test_main_writes_the_library_hits(tmp_path, analog):
    import csv
    from falcon_amd.falcon import main
    mgf, lib_mgf, work = str(tmp_path / "in.mgf"), str(tmp_path / "gnps_like.mgf"), str(tmp_path / "work")
    _write_run_and_library(mgf, lib_mgf)
    plain, full = str(tmp_path / "plain"), str(tmp_path / "full")
    common = ["--eps", "0.3", "--export_representatives", "--work_dir", work, "--network", "--network_min_cosine", "0.5"]
    flags = ["--library", lib_mgf] + (["--library_analog"] if analog else []) + LIBRARY_ARGS
    assert main([mgf, plain] + common) == 0
    assert main([mgf, full] + common + flags) == 0
    for ext in (".csv", ".mgf", ".network.csv"):
        assert open(plain + ext, "rb").read() == open(full + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".library.csv")
    header = [l[2:] for l in open(full + ".csv", newline="").read().split("\n") if l.startswith("# ")]
    header += [f"library = {lib_mgf}", f"library_analog = {analog}", "library_max_shift = 60.000", "library_min_cosine = 0.500",
               "library_min_matched_peaks = 4", "library_top_n = 2"]
    text, blocks, refs = _expected_library(full, work, header, analog)
    got = open(full + ".library.csv", newline="").read()
    assert got == text
    # the chargeless entries (templates 4 and 5, the decoy) are offered to both charges, every other entry to its own alone
    assert len(refs) == 2
    for charge, ref in zip(("2", "3"), refs):
        ids = set(ref["library_id"].tolist())
        mine = {f"CCMSLIB{t:08d}" for t in range(4) if str(2 + t % 2) == charge}
        assert ids == mine | {"CCMSLIB00000004", "CCMSLIB00000005", "decoy"}, (charge, ids)
    # the right compounds: every cluster holds copies of one template; its precursor names it
    table = list(csv.DictReader(l for l in got.split("\n") if l and not l.startswith("#")))
    named = {}
    for row in table:
        t = int(round((float(row["library_precursor_mz"]) + float(row["delta_mz"]) - 940.0) / 3.0))
        named.setdefault(t, []).append((row["name"], row["library_id"], float(row["delta_mz"]), int(row["rank"])))
    want = {4: ('Compound 4, "form 4" M+H', "CCMSLIB00000004"), 5: ('Compound 5, "form 5" M+H', "CCMSLIB00000005")}
    if analog:
        want.update({t: (f'Compound {t}, "form {t}" M+H', f"CCMSLIB{t:08d}") for t in range(4)})
    assert sorted(named) == sorted(want), named
    for t, hits in named.items():
        best = [h for h in hits if h[3] == 1]                   # (one a cluster: a template's copies may make two clusters)
        assert best and all(h[:2] == want[t] and abs(h[2] + (PLANTED if t < 4 else 0.0)) < 0.01 for h in best), (t, hits)
    assert all(row["adduct"] == "M+H" and row["inchikey"].startswith("KEY-") for row in table if row["rank"] == "1")
    assert main([mgf, full] + common + flags) == 1                                  # the file is there: refused without --overwrite
