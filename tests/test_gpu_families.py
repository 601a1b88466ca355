"""Molecular families on the device (`fal_network_families`) against the numpy restatement of tests/family_cases.py: every
comparison is on bits, every "at least" is asserted on the restatement's statistics (family_cases.expected does that before it
hands a result out).  Trivial graphs, random graphs with and without ties, a long chain, a star, two cliques, equal sims, edge
order and duplicates, node order, every refused input, counter 13, the public function and `main()` with `--network_families`."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import family_cases as fc

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


def gpu_families(ctx, g, max_size, delta):
    family, size, rnd, n_families, n_rounds = ctx.network_families(g["u"], g["v"], g["sim"], g["n"], max_size, delta)
    return dict(family=family.cpu().numpy(), size=size.cpu().numpy(), round=rnd.cpu().numpy(), n_families=n_families,
                n_rounds=n_rounds, n_cut=ctx.counter(13))


def check_case(ctx, name):
    """the device == the restatement, counter 13 included"""
    g, max_size, delta, _ = fc.CASES[name]
    want = fc.expected(name)
    got = gpu_families(ctx, g, max_size, delta)
    print(name, {k: v for k, v in got.items() if not isinstance(v, np.ndarray)}, "restatement:", want["n_families"], want["n_rounds"],
          want["n_cut"], "largest", want["largest_before"], "->", want["largest"])
    assert fc.same(got, want), (name, got["n_families"], want["n_families"], got["n_rounds"], want["n_rounds"])
    assert got["n_cut"] == want["n_cut"], (name, got["n_cut"], want["n_cut"])
    return got


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_the_device_is_the_restatement(ctx, name):
    check_case(ctx, name)


def test_the_cases_are_the_ones_the_issue_names():
    """a check of the case table in tests/family_cases.py, not of the library: the sizes, caps and deltas the other tests rely on"""
    for n in (1, 2, 255, 256, 257):
        assert fc.CASES[f"empty-{n}"][0]["n"] == n and len(fc.CASES[f"empty-{n}"][0]["u"]) == 0
    for name, nodes, edges, cap, delta in (("random-300", 300, 450, 20, 0.02), ("random-300-delta-0", 300, 450, 20, 0.0),
                                           ("random-300-grid", 300, 450, 20, 0.0), ("random-5000", 5000, 7000, 100, 0.02),
                                           ("chain-cap-0", 3000, 2999, 0, 0.02), ("chain-cap-3000", 3000, 2999, 3000, 0.0),
                                           ("chain-cap-2999", 3000, 2999, 2999, 0.0), ("chain-cap-64", 3000, 2999, 64, 0.0),
                                           ("star-cap-0", 2001, 2000, 0, 0.02), ("star-cap-100", 2001, 2000, 100, 0.02),
                                           ("cliques-cap-10", 20, 91, 10, 0.02), ("cliques-cap-19", 20, 91, 19, 0.02),
                                           ("cliques-cap-20", 20, 91, 20, 0.02)):
        g, max_size, d, _ = fc.CASES[name]
        assert (g["n"], len(g["u"]), max_size, d) == (nodes, edges, cap, delta), name
    # ties on the grid: at most 7 distinct sims
    assert len(np.unique(fc.CASES["random-300-grid"][0]["sim"])) <= 7


def test_edge_order_duplicates_and_node_order_change_nothing(ctx):
    g, max_size, delta, _ = fc.CASES["random-300"]
    base = check_case(ctx, "random-300")
    h, pick = fc.shuffled(g, duplicates=40)
    got = check_case(ctx, "duplicates-shuffled")
    assert np.array_equal(got["family"], base["family"]) and np.array_equal(got["size"], base["size"])
    assert np.array_equal(got["round"], base["round"][pick]) and got["n_rounds"] == base["n_rounds"]
    _, perm = fc.permuted(g)
    got = check_case(ctx, "permuted")
    assert np.array_equal(got["round"], base["round"]) and np.array_equal(got["size"][perm], base["size"])
    assert fc.family_sets(got) == {frozenset(perm[list(s)].tolist()) for s in fc.family_sets(base)}


def raw_call(ctx, g, max_size, delta):
    """the C entry point with marked outputs -> (rc, outputs on the host, n_families, n_rounds)"""
    import torch
    u, v, sim = ctx.to_dev(g["u"], torch.int32), ctx.to_dev(g["v"], torch.int32), ctx.to_dev(g["sim"], torch.float32)
    n, m = g["n"], len(g["u"])
    out = [ctx.empty((max(k, 1),), torch.int32) for k in (n, n, m)]
    for t in out:
        t.fill_(MARK)
    nf, nr = C.c_int64(MARK), C.c_int64(MARK)
    rc = ctx.lib.fal_network_families(ctx._h, ctx._p(u), ctx._p(v), ctx._p(sim), m, n, int(max_size), float(delta),
                                      *(ctx._p(t) for t in out), C.byref(nf), C.byref(nr))
    ctx.sync()
    return rc, [t.cpu().numpy() for t in out], nf.value, nr.value


@pytest.mark.parametrize("name", sorted(fc.invalid_cases()))
def test_a_refused_input_writes_nothing_and_the_context_stays_usable(ctx, name):
    g, max_size, delta = fc.invalid_cases()[name]
    assert not fc.valid(g["n"], g["u"], g["v"], g["sim"], max_size, delta)
    rc, out, nf, nr = raw_call(ctx, g, max_size, delta)
    assert rc == -1 and all((o == MARK).all() for o in out) and (nf, nr) == (MARK, MARK), (rc, nf, nr)      # FAL_EINVAL
    from falcon_amd._lib import FalconHipError
    with pytest.raises(FalconHipError, match="code -1.*fal_network_families"):
        gpu_families(ctx, g, max_size, delta)
    check_case(ctx, "cliques-cap-10")


def test_no_nodes_is_a_no_op_and_counter_13_is_the_last_calls(ctx):
    assert check_case(ctx, "random-300")["n_cut"] == ctx.counter(13) >= 100
    rc, out, nf, nr = raw_call(ctx, fc.empty(0), 100, 0.02)
    assert rc == 0 and all((o == MARK).all() for o in out) and (nf, nr) == (0, 0) and ctx.counter(13) == 0
    assert check_case(ctx, "cliques-cap-19")["n_cut"] == ctx.counter(13) == 1
    assert check_case(ctx, "cliques-cap-20")["n_cut"] == ctx.counter(13) == 0
    rc, out, nf, nr = raw_call(ctx, dict(fc.empty(0), u=np.zeros(1, i32), v=np.ones(1, i32), sim=np.ones(1, f32)), 100, 0.02)
    assert rc == -1                                                                # an edge between no nodes


# ---- the public function -----------------------------------------------------------------------------------------------------------
def test_network_families_of_the_analogue_network(ctx):
    from falcon_amd.cluster import cluster as fcl
    from tests import network_cases as nc
    nodes = nc.analogue_case()
    a = nc.ANALOGUE
    n_rows = len(nodes["indptr"]) - 1
    pm_row = np.full(n_rows, 300.0, f32)
    pm_row[nodes["rows"]] = nodes["precursor_mz"]
    ds = fcl.SpectrumDataset(pm_row, np.zeros(n_rows, f32), nodes["mz"], nodes["intensity"], nodes["indptr"])
    pipe = fcl.ClusterPipeline(ctx)
    net = fcl.representative_network(ds, nodes["rows"], a["fragment_tol"], a["max_shift"], a["min_cosine"], a["min_matched"], 5,
                                     pipeline=pipe)
    dev = fcl.representative_network(ds, nodes["rows"], a["fragment_tol"], a["max_shift"], a["min_cosine"], a["min_matched"], 5,
                                     pipeline=pipe, on_device=True)
    assert set(net) == set(dev) == {"a", "b", "similarity", "matched", "delta_mz"}
    assert all(nc.same(net[k], dev[k].cpu().numpy()) for k in net) and len(net["a"]) >= 100
    # (the analogues' links all lie between 0.993 and 0.999: a delta of 0.02 would dissolve every component in one round)
    want = fc.families(120, net["a"], net["b"], net["similarity"], 6, 0.002)
    print({k: v for k, v in want.items() if not isinstance(v, np.ndarray)})
    assert want["largest_before"] >= 10 and want["n_cut"] >= 10 and want["n_families"] >= 8 and want["n_rounds"] >= 2
    keep = want["round"] == 0
    for network in (net, dev):
        out = fcl.network_families(network, 120, max_size=6, delta=0.002, pipeline=pipe)
        assert all(isinstance(out[k], np.ndarray) and nc.same(out[k], net[k][keep]) for k in net)
        assert nc.same(out["family"], want["family"][net["a"][keep]]) and nc.same(out["family"], want["family"][net["b"][keep]])
        assert nc.same(out["node_family"], want["family"]) and nc.same(out["node_size"], want["size"])
        assert (out["n_families"], out["n_rounds"], out["n_cut"]) == (want["n_families"], want["n_rounds"], want["n_cut"])
    uncapped = fcl.network_families(net, 120, max_size=0, pipeline=pipe)
    assert uncapped["n_cut"] == 0 and len(uncapped["a"]) == len(net["a"]) and uncapped["node_size"].max() == want["largest_before"]


# ---- main() ------------------------------------------------------------------------------------------------------------------------
NETWORK_ARGS = ["--network", "--network_min_cosine", "0.5", "--network_min_matched_peaks", "4", "--network_top_k", "4",
                "--network_max_shift", "60"]
NETWORK_LINES = ["network = True", "network_min_cosine = 0.500", "network_min_matched_peaks = 4", "network_top_k = 4",
                 "network_max_shift = 60.000"]
FAMILY_ARGS = ["--network_families", "--network_max_family_size", "3"]
CHAIN_STEPS = (0.95, 0.95, 0.915)


def _write_chains(path):
    """six templates, each at four precursor shifts with about half of its peaks moving along; three peaks join the spectrum at
    every shift, sized so that the cosine of a variant and the next is CHAIN_STEPS (that of variants further apart is the
    product of the steps between them: 0.9025, 0.869, 0.826).  With --network_top_k 4 the variants of a template are one component
    of at least four clusters -- more where the clustering splits a variant's copies; those clusters are linked at nearly 1.
    Under the cap of 3 and the default delta the rounds take the links at 0.826, at 0.869, then those at 0.9025 and 0.915:
    variants 0 to 2 stay a family, or, with a split variant among them, lose their links at 0.95 too and the split variant's
    clusters stay one.  Every variant with two noisy copies at nearly its precursor (they cluster with
    it), charges 2 and 3 -> the MGF file"""
    from falcon_amd.ms_io import ms_io
    from tests import network_cases as nc
    rng = np.random.default_rng(12)
    specs = []
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
            for c in range(3):
                m = (mz + moves * s + rng.normal(0.0, 0.002, 30))[has]
                o = np.argsort(m)
                specs.append({"identifier": f"scan={len(specs) + 1}", "precursor_mz": pmz * (1.0 + rng.normal(0, 1e-6)),
                              "precursor_charge": 2 + t % 2, "retention_time": float(np.round(rng.uniform(0.0, 3600.0), 3)),
                              "mz": m[o], "intensity": (it * rng.uniform(0.97, 1.03, 30))[has][o].astype(np.float32)})
    ms_io.write_spectra(path, [specs[i] for i in rng.permutation(len(specs))])


def _expected_blocks(out, work):
    """the network's blocks from the run's own partitions, the cluster CSV's labels and the exported representatives' titles (as
    tests/test_gpu_network.py's _expected_network, at NETWORK_ARGS)"""
    import json
    from tests import network_cases as nc
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
        u, v, sim, matched = nc.network_ref(nodes, 0.05, 60.0, 0.5, 4, 4)
        pm = nodes["precursor_mz"].astype(f32)
        blocks.append(dict(charge=charge, first=first, a=u, b=v, similarity=sim, matched=matched, delta_mz=pm[v] - pm[u]))
    return sorted(blocks, key=lambda b: b["first"])


def _expected_network(out, work, header):
    """the text of today's writer"""
    from falcon_amd.ms_io import network_io
    f = io.StringIO(newline="")
    network_io.write_network(f, header, _expected_blocks(out, work))
    return f.getvalue()


def _expected_files(out, work, header):
    """both files' text: the links rebuilt from the run's own partitions, the families of every charge by the restatement
    -> (network text, families text, per-charge results)"""
    from falcon_amd.ms_io import network_io
    blocks = _expected_blocks(out, work)
    csv_rows = [l.split(",") for l in open(out + ".csv", newline="").read().split("\n") if l and not l.startswith("#")][1:]
    last = max(int(r[5]) for r in csv_rows)
    results = []
    for k, b in enumerate(blocks):
        n = (blocks[k + 1]["first"] if k + 1 < len(blocks) else last + 1) - b["first"]
        res = fc.families(n, b["a"], b["b"], b["similarity"], 3, 0.02)
        keep = res["round"] == 0
        for col in ("a", "b", "similarity", "matched", "delta_mz"):
            b[col] = b[col][keep]
        b.update(family=res["family"][b["a"]], node_family=res["family"], node_size=res["size"], n_families=res["n_families"])
        results.append(res)
    f, g = io.StringIO(newline=""), io.StringIO(newline="")
    network_io.write_network_with_families(f, header, blocks)
    network_io.write_families(g, header, blocks)
    return f.getvalue(), g.getvalue(), results


@pytest.mark.parametrize("mode", [[], ["--exact"]], ids=["default", "exact"])
def test_main_writes_the_families(tmp_path, mode):
    from falcon_amd.falcon import main
    mgf, work = str(tmp_path / "in.mgf"), str(tmp_path / "work")
    _write_chains(mgf)
    plain, net, full = str(tmp_path / "plain"), str(tmp_path / "net"), str(tmp_path / "full")
    common = ["--eps", "0.3", "--export_representatives", "--work_dir", work] + mode
    assert main([mgf, plain] + common) == 0
    assert main([mgf, net] + common + NETWORK_ARGS) == 0
    assert main([mgf, full] + common + NETWORK_ARGS + FAMILY_ARGS) == 0
    for ext in (".csv", ".mgf"):
        assert open(plain + ext, "rb").read() == open(full + ext, "rb").read(), ext
    assert not os.path.exists(net + ".families.csv") and not os.path.exists(plain + ".families.csv")
    header = [l[2:] for l in open(full + ".csv", newline="").read().split("\n") if l.startswith("# ")]
    header += NETWORK_LINES
    assert open(net + ".network.csv", newline="").read() == _expected_network(net, work, header)            # today's writer's text
    header += ["network_families = True", "network_max_family_size = 3", "network_family_delta = 0.020"]
    net_text, fam_text, results = _expected_files(full, work, header)
    print([{k: v for k, v in r.items() if not isinstance(v, np.ndarray)} for r in results])
    assert len(results) == 2
    for r in results:                      # every charge: a component above the cap, cut into at least two families
        assert r["largest_before"] > 3 and r["n_cut"] >= 1 and r["n_families"] >= 2 and r["largest"] <= 3, r
    assert open(full + ".network.csv", newline="").read() == net_text
    assert open(full + ".families.csv", newline="").read() == fam_text
    assert main([mgf, full] + common + NETWORK_ARGS + FAMILY_ARGS) == 1          # the files are there: refused without --overwrite
    os.remove(full + ".network.csv")
    assert main([mgf, full] + common + NETWORK_ARGS + FAMILY_ARGS) == 1          # the families file alone refuses too


# ---- scratch hygiene -------------------------------------------------------------------------------------------------------------
def test_cases_again_under_debug_poison():
    """FALCON_DEBUG_POISON=1 (scratch filled with 0xFF before use, a slot that grows while a pointer into it is held fails) is
    read once per process: a fresh child runs the cases again, a small one first"""
    env = dict(os.environ, FALCON_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "family_poison_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
