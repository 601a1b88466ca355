"""Consensus representatives on the GPU: `Context.consensus_spectra` (`fal_consensus_spectra`) bit for bit against the numpy
restatement of tests/consensus_cases.py, the quality property (a consensus is at least as close to its cluster's members as the
medoid is), and `main()` with `--representatives consensus`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import consensus_cases as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cut():
    from falcon_amd import _lib
    return _lib.CONS_LDS_PEAKS


# ---- the cases: name -> (partition, fragment_tol, min_fraction) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    """~20 k spectra in shuffled dataset order: cluster sizes 1 .. 2,000, one cluster of 5,000 members x 50 peaks (250,000 pooled
    peaks), clusters of exactly cut - 1, cut and cut + 1 pooled peaks, members without peaks, zero-intensity groups, duplicate
    m/z across and inside members"""
    rng = np.random.default_rng(2024)
    cut = _cut()
    assert cut == 4096, "the three clusters around the cut below are written for 4,096"
    sizes = [5000, 65, 64, 241, 2000, 1500, 1000, 700, 500, 300, 200] + list(range(1, 100)) + [2] * 300 + [1] * 2800
    over = {0: dict(fixed_peaks=50, n_template=60), 1: dict(fixed_peaks=63), 2: dict(fixed_peaks=64), 3: dict(fixed_peaks=17)}
    part = cc.make_partition(rng, sizes, peaks=(1, 12), p_empty=0.05, p_zero=0.05, overrides=over)
    pooled = _pooled(part)
    assert pooled[:4].tolist() == [250000, cut - 1, cut, cut + 1] and 19000 < len(part["labels"]) < 21000
    return part


@functools.lru_cache(maxsize=None)
def _no_ties():
    """no two equal m/z inside a cluster (continuous jitter, and a peak that still meets another one's float32 value moves to
    the next float32 until none does), one cluster above the cut"""
    rng = np.random.default_rng(77)
    part = cc.make_partition(rng, [900, 1, 2, 3, 40, 250, 1, 17], peaks=(3, 12), grid_jitter=False)
    lab_of_peak = np.repeat(part["labels"], np.diff(part["indptr"]))
    while True:
        order = np.lexsort((part["mz"], lab_of_peak))              # by cluster, then m/z
        x, lab = part["mz"][order], lab_of_peak[order]
        dup = order[1:][(x[1:] == x[:-1]) & (lab[1:] == lab[:-1])]
        if not len(dup):
            break
        part["mz"][dup] = np.nextafter(part["mz"][dup], np.float32(np.inf))
    assert _pooled(part)[0] > _cut()
    return part


CASES = {
    "mixed": lambda: (_mixed(), 0.05, 0.25),
    "mixed_q001": lambda: (_mixed(), 0.05, 0.01),
    "mixed_q05": lambda: (_mixed(), 0.05, 0.5),
    "mixed_tol0_q1": lambda: (_mixed(), 0.0, 1.0),
    "all_fallback": lambda: (cc.make_partition(np.random.default_rng(3), [2, 3, 9, 150, 700], peaks=(1, 9), disjoint=True), 0.05, 1.0),
    "zero_and_empty": lambda: (cc.make_partition(np.random.default_rng(4), [2] * 50 + [5] * 20 + [80, 400], p_empty=0.4, p_zero=0.5),
                               0.05, 0.5),
    "all_empty": lambda: (cc.make_partition(np.random.default_rng(5), [3, 1, 2], p_empty=1.0), 0.05, 0.25),
    "no_ties": lambda: (_no_ties(), 0.05, 0.25),
}


def _pooled(part):
    """pooled peaks of every cluster"""
    return np.bincount(np.repeat(part["labels"], np.diff(part["indptr"])), minlength=len(part["medoids"]))


def _gpu(ctx, part, tol, q, **kw):
    out = ctx.consensus_spectra(part["mz"], part["intensity"], part["indptr"], part["labels"], part["medoids"], tol, q, **kw)
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def _reference(name):
    part, tol, q = CASES[name]()
    return cc.consensus_reference(part["mz"], part["intensity"], part["indptr"], part["labels"], part["medoids"], tol, q)


def _equal(got, ref, part):
    assert np.array_equal(got[0], ref[0]), "indptr"
    assert np.array_equal(cc.bits(got[1]), cc.bits(ref[1])), "m/z bits"
    assert np.array_equal(cc.bits(got[2]), cc.bits(ref[2])), "intensity bits"
    assert np.array_equal(got[3] & ~cc.GLOBAL, ref[3]), "status"
    # the device-wide sort took exactly the clusters of 2+ members above the cut: the library says so per cluster
    pooled, members = cc.pooled_sizes(part)                        # (rows whose label names no cluster count nowhere)
    big = (pooled > _cut()) & (members > 1)
    assert np.array_equal((got[3] & cc.GLOBAL) != 0, big), "which clusters took the device-wide sort"


def check_case(ctx, name):
    part, tol, q = CASES[name]()
    got = _gpu(ctx, part, tol, q)
    _equal(got, _reference(name), part)
    return got


def check_second_call_and_permutation(ctx):
    part, tol, q = CASES["no_ties"]()
    a, b = _gpu(ctx, part, tol, q), _gpu(ctx, part, tol, q)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
    # the same clusters with the dataset rows permuted: without m/z ties inside a cluster the pooled order is the m/z order
    # alone, so every cluster's peak list has the same bits
    perm = cc.permute_rows(part, np.random.default_rng(9))
    c = _gpu(ctx, perm, tol, q)
    _equal(c, cc.consensus_reference(perm["mz"], perm["intensity"], perm["indptr"], perm["labels"], perm["medoids"], tol, q), perm)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[3], c[3])
    # (a fallback or a single member copies the spectrum as it is: those lists are equal too)
    assert np.array_equal(cc.bits(a[1]), cc.bits(c[1])) and np.array_equal(cc.bits(a[2]), cc.bits(c[2]))


def check_undersized_cap(ctx):
    """nnz_cap below the output: the clusters that end behind it get CONS_CAPACITY and write nothing, the others are complete,
    indptr is the true one, and the guard region behind the outputs keeps its bytes"""
    import torch
    part, tol, q = CASES["mixed"]()
    ref = _reference("mixed")
    total = int(ref[0][-1])
    cap, guard = total // 2, 4096
    d = {k: ctx.to_dev(part[k]) for k in ("mz", "intensity", "indptr", "labels", "medoids")}
    nc, n = len(part["medoids"]), len(part["labels"])
    out_ptr = ctx.empty((nc + 1,), torch.int64)
    status = ctx.empty((nc,), torch.int32)
    out_mz = torch.full((cap + guard,), -7.0, dtype=torch.float32, device=ctx.tdev)
    out_it = torch.full((cap + guard,), -7.0, dtype=torch.float32, device=ctx.tdev)
    from falcon_amd._lib import check
    check(ctx.lib.fal_consensus_spectra(ctx._h, ctx._p(d["mz"]), ctx._p(d["intensity"]), ctx._p(d["indptr"]), n, ctx._p(d["labels"]),
                                        ctx._p(d["medoids"]), nc, tol, q, cap, ctx._p(out_ptr), ctx._p(out_mz), ctx._p(out_it),
                                        ctx._p(status)), "fal_consensus_spectra")
    ctx.sync()
    out_ptr, status, out_mz, out_it = (t.cpu().numpy() for t in (out_ptr, status, out_mz, out_it))
    assert np.array_equal(out_ptr, ref[0])
    fits = ref[0][1:] <= cap
    assert fits.any() and (~fits).any()
    assert np.array_equal((status & cc.CAPACITY) != 0, ~fits)
    assert np.array_equal(status & ~(cc.CAPACITY | cc.GLOBAL), ref[3])
    written = np.zeros(cap + guard, bool)
    for c in np.flatnonzero(fits):
        written[ref[0][c]:ref[0][c + 1]] = True
    w = np.flatnonzero(written)
    assert np.array_equal(cc.bits(out_mz[w]), cc.bits(ref[1][w])) and np.array_equal(cc.bits(out_it[w]), cc.bits(ref[2][w]))
    assert (out_mz[~written] == -7.0).all() and (out_it[~written] == -7.0).all(), "bytes outside the clusters that fit were written"


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(CASES))
def test_consensus_equals_the_restatement_bit_for_bit(ctx, name):
    got = check_case(ctx, name)
    part, _, q = CASES[name]()
    if name.startswith("mixed"):
        assert got[3][0] & cc.GLOBAL and not got[3][1] & cc.GLOBAL and not got[3][2] & cc.GLOBAL and got[3][3] & cc.GLOBAL
        assert ((got[3] & cc.GLOBAL) != 0).sum() >= 5                   # 5,000 x 50, cut + 1, and the clusters of 1,000+ members
    if name == "all_fallback":
        assert (got[3] & cc.FALLBACK).all()
    if name == "zero_and_empty":
        assert (got[2] == 0).any() and (np.diff(part["indptr"]) == 0).any()


def test_second_call_and_row_permutation(ctx):
    check_second_call_and_permutation(ctx)


def test_undersized_capacity_is_reported_and_nothing_is_written_outside(ctx):
    check_undersized_cap(ctx)


def test_public_function_takes_host_and_device_datasets(ctx):
    from falcon_amd.cluster.cluster import ClusterPipeline, SpectrumDataset, consensus_spectra
    part, tol, q = CASES["zero_and_empty"]()
    n = len(part["labels"])
    ds = SpectrumDataset(np.zeros(n, np.float32), None, part["mz"], part["intensity"], part["indptr"])
    pipe = ClusterPipeline(ctx)
    host = consensus_spectra(ds, part["labels"], part["medoids"], tol, q, pipeline=pipe)
    dev = consensus_spectra(ds.to_device(ctx.tdev), ctx.to_dev(part["labels"]), ctx.to_dev(part["medoids"]), tol, q, pipeline=pipe)
    _equal(host, _reference("zero_and_empty"), part)
    for x, y in zip(host, dev):
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
    with pytest.raises(ValueError):
        consensus_spectra(ds, part["labels"], part["medoids"], tol, 0.0, pipeline=pipe)


def test_wrapper_refuses_an_undersized_capacity(ctx):
    from falcon_amd._lib import FalconHipError
    part, tol, q = CASES["zero_and_empty"]()
    with pytest.raises(FalconHipError):
        _gpu(ctx, part, tol, q, nnz_cap=int(_reference("zero_and_empty")[0][-1]) - 1)


def test_cli_consensus_step_accepts_clusters_above_the_lds_cut(ctx):
    """`falcon._consensus` (what `main()` calls per charge) on the mixed partition, whose largest clusters take the device-wide
    sort: that status bit is information, not an error, and the peaks are the restatement's"""
    from falcon_amd import falcon
    from falcon_amd.config import config
    config.parse("in.mgf out --export_representatives --representatives consensus")
    part, _, _ = CASES["mixed"]()
    assert (_pooled(part) > _cut()).sum() >= 5
    ptr, mz, it = falcon._consensus(ctx, part, "2", part["labels"], part["medoids"])
    ref = _reference("mixed")                                       # fragment_tol 0.05, min_fraction 0.25: the CLI's defaults
    assert np.array_equal(ptr, ref[0]) and np.array_equal(cc.bits(mz), cc.bits(ref[1])) and np.array_equal(cc.bits(it), cc.bits(ref[2]))
    config.parse("in.mgf out --export_representatives")
    assert falcon._consensus(ctx, part, "2", part["labels"], part["medoids"]) is None


def test_every_case_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 (scratch filled with 0xFF before use, a slot that grows while a pointer into it is held fails) is
    read once per process: a fresh child runs every case, the second call / permutation and the capacity case again"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "consensus_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- quality ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["ann", "exact"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_consensus_is_at_least_as_close_to_the_members_as_the_medoid(ctx, seed, exact):
    """spectra drawn from 8 templates (15 % of the peaks dropped, jitter, intensity noise, 5 noise peaks): for every cluster of 3+
    members the mean matched-peak cosine of the consensus to the members is not below the medoid's to the other members, and no
    cluster falls back.  (eps 0.35: spectra of one template score 0.8 - 0.9 against each other, of two templates ~0.)"""
    from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset, consensus_spectra
    from oracle.falcon_oracle import cosine_fast
    d = cc.template_spectra(seed)
    ds = SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
    pipe = ClusterPipeline(ctx)
    p = AnnParams(eps=0.35, exact=True, mz_interval=0) if exact else AnnParams(eps=0.35)
    from falcon_amd.cluster.cluster import generate_clusters
    labels, medoids = generate_clusters(ds, "complete", 0.35, 0, 20.0, "ppm", None, 0.05, 2 ** 15, ann=p, pipeline=pipe)
    ptr, mz, it, status = consensus_spectra(ds, labels, medoids, 0.05, pipeline=pipe)
    ip = d["indptr"]
    spec = lambda r: (d["mz"][ip[r]:ip[r + 1]], d["intensity"][ip[r]:ip[r + 1]])
    seen = 0
    for c in np.flatnonzero(np.bincount(labels, minlength=len(medoids)) >= 3):
        rows = np.flatnonzero(labels == c)
        cons = np.mean([cosine_fast(mz[ptr[c]:ptr[c + 1]], it[ptr[c]:ptr[c + 1]], *spec(r), 0.05)[0] for r in rows])
        med = np.mean([cosine_fast(*spec(medoids[c]), *spec(r), 0.05)[0] for r in rows if r != medoids[c]])
        print(f"seed {seed} exact {exact} cluster {c}: {len(rows)} members, consensus {cons:.4f}, medoid {med:.4f}")
        assert not status[c] & cc.FALLBACK
        assert cons >= med, (c, cons, med)
        seen += 1
    assert seen >= 4


# ---- CLI --------------------------------------------------------------------------------------------------------------------
def _entries(path):
    """MGF entries as (header lines, peak lines)"""
    out, head, peaks = [], None, None
    for line in open(path).read().splitlines():
        if line == "BEGIN IONS":
            head, peaks = [], []
        elif line == "END IONS":
            out.append((head, peaks))
        elif line and head is not None:
            (head if "=" in line and not line[0].isdigit() else peaks).append(line)
    return out


def _split_csv(path):
    lines = open(path).read().splitlines()
    return [l for l in lines if l.startswith("#")], [l for l in lines if not l.startswith("#")]


@pytest.mark.parametrize("mode", [[], ["--exact"]], ids=["ann", "exact"])
def test_main_writes_consensus_representatives(tmp_path, mode):
    from falcon_amd import synth
    from falcon_amd.falcon import main
    from falcon_amd.ms_io import ms_io
    d = synth.generate(3000, seed=33)
    specs = []
    for i in range(3000):
        a, b = d["indptr"][i], d["indptr"][i + 1]
        specs.append({"identifier": f"scan={i}", "precursor_mz": float(d["precursor_mz"][i]),
                      "precursor_charge": int(d["precursor_charge"][i]), "retention_time": float(d["retention_time"][i]),
                      "mz": d["mz"][a:b].astype(np.float64), "intensity": d["intensity"][a:b]})
    mgf = str(tmp_path / "in.mgf")
    ms_io.write_spectra(mgf, specs)
    med, con, work = str(tmp_path / "med"), str(tmp_path / "con"), tmp_path / "work"
    common = ["--eps", "0.3", "--export_representatives", "--work_dir", str(work)] + mode
    assert main([mgf, med] + common) == 0
    assert main([mgf, con] + common + ["--representatives", "consensus"]) == 0
    h1, b1 = _split_csv(med + ".csv")
    h2, b2 = _split_csv(con + ".csv")
    assert b1 == b2 and len(b1) > 2000
    assert h2[-1] == "#" and h1 == h2[:-3] + ["#"]
    assert h2[-3:-1] == ["# representatives = consensus", "# consensus_min_fraction = 0.250"]
    e1, e2 = _entries(med + ".mgf"), _entries(con + ".mgf")
    assert len(e1) == len(e2) > 100
    assert [h for h, _ in e1] == [h for h, _ in e2]                     # TITLE / PEPMASS / CHARGE / RTINSECONDS / CLUSTER, in order
    assert all([x.split("=")[0] for x in h] == ["TITLE", "PEPMASS", "CHARGE", "RTINSECONDS", "CLUSTER"] for h, _ in e1)
    # the restatement from the work directory's partitions and the CSV's labels
    table = {r.split(",")[1]: int(r.split(",")[5]) for r in b1[1:]}
    expected = {}
    for charge in (2, 3):
        z = np.load(work / "spectra" / f"spectra_charge_{charge}.npz")
        glob = np.array([table[str(i)] for i in z["identifier"]])
        lab = (glob - glob.min()).astype(np.int32)
        title_of = {}
        for h, _ in e1:
            c = int(h[4].split("=")[1])
            if glob.min() <= c <= glob.max():
                title_of[c - glob.min()] = h[0].split("=", 1)[1]
        row_of = {str(t): i for i, t in enumerate(z["identifier"])}
        medoids = np.array([row_of[title_of[c]] for c in range(lab.max() + 1)], np.int32)
        ptr, mz, it, st = cc.consensus_reference(z["mz"], z["intensity"], z["indptr"], lab, medoids, 0.05, 0.25)
        sizes = np.bincount(lab)
        for c in range(len(medoids)):
            expected[int(c + glob.min())] = ([f"{a} {b}" for a, b in zip(mz[ptr[c]:ptr[c + 1]], it[ptr[c]:ptr[c + 1]])], sizes[c])
    assert len(expected) == len(e2)
    merged = 0
    for (h, p_med), (_, p_con) in zip(e1, e2):
        want, size = expected[int(h[4].split("=")[1])]
        assert p_con == want, h
        if size == 1:
            assert p_con == p_med
        else:
            merged += 1
    assert merged > 10
