"""Exact mode under `shard=(rank, world)`, every rank in turn in ONE process (a rank's share is a function of (rank, world)
alone, no collective is involved): `ClusterPipeline.run_many`, `PartitionRunner.run` on host-resident partitions and
`distributed.run_sharded` must give the single-GPU exact partition with the same medoid row for every cluster."""
import numpy as np
import pytest

from tests.test_gpu_exact import _spectra

pytestmark = pytest.mark.gpu
ARGS = dict(tol=20.0, mode="ppm", frag=0.05, batch=2 ** 15)


def _params(linkage, t=0.35, min_matches=2, mz_interval=1.0, exact=True):
    from falcon_amd.cluster.cluster import AnnParams, resolve_params
    return resolve_params(linkage, t, min_matches, AnnParams(eps=t, exact=exact, mz_interval=mz_interval))


def _datasets(device=True, per=60):
    """two partitions (charge-like), many buckets each: clusters of several templates, chained spectra"""
    import torch
    from falcon_amd.cluster.cluster import SpectrumDataset
    out = []
    for seed, centres in ((17, [450.0, 451.5, 500.0, 620.0, 800.0, 801.2, 1200.0]), (31, [430.2, 555.0, 556.3, 910.0, 1010.0])):
        d = _spectra(5, per, centres, seed=seed, jitter=0.01, chained=4)
        cols = (d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])
        if device:
            cols = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in cols]
        out.append(SpectrumDataset(*cols))
    return out


def _clusters(labels, medoids):
    """{frozenset(dataset rows): medoid row} of every cluster (groups of one included)"""
    labels, medoids = np.asarray(labels), np.asarray(medoids)
    assert labels.min() == 0 and labels.max() + 1 == len(medoids)
    o = np.argsort(labels, kind="stable")
    cuts = np.flatnonzero(np.diff(labels[o])) + 1
    out = {}
    for grp in np.split(o, cuts):
        c = int(labels[grp[0]])
        assert int(medoids[c]) in set(grp.tolist())
        out[frozenset(grp.tolist())] = int(medoids[c])
    return out


def _single(pipe, datasets, p, rt_tol):
    outs = [pipe.run(ds, ARGS["tol"], ARGS["mode"], rt_tol, ARGS["frag"], ARGS["batch"], p) for ds in datasets]
    return [(l.cpu().numpy(), m.cpu().numpy()) for l, m in outs]


def _merge(per_rank, sizes):
    """per_rank[r] = (outs, lasts) of rank r -> per partition (labels by dataset row, medoid rows); every row on one rank"""
    from falcon_amd import distributed as fdist
    merged = []
    for j, n in enumerate(sizes):
        shards, seen = [], np.zeros(n, np.int64)
        for outs, lasts in per_rank:
            rows = lasts[j]["rows"].cpu().numpy()
            lab, med = (t.cpu().numpy() for t in outs[j])
            assert len(rows) == len(lab)
            seen[rows] += 1
            shards.append((rows, lab, rows[med.astype(np.int64)].astype(np.int32)))
        assert (seen == 1).all()                                              # every row on exactly one rank
        merged.append(fdist.merge_shards(n, shards))
    return merged


@pytest.fixture(scope="module")
def pipe():
    from falcon_amd.cluster.cluster import ClusterPipeline
    return ClusterPipeline(device=0)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mz_interval", [1.0, 0.0])
@pytest.mark.parametrize("linkage,rt_tol", [("complete", None), ("average", 30.0)])
def test_run_many_sharded_exact_equals_one_gpu(pipe, world, mz_interval, linkage, rt_tol):
    datasets = _datasets()
    p = _params(linkage, mz_interval=mz_interval)
    single = _single(pipe, datasets, p, rt_tol)
    per_rank = []
    for r in range(world):
        outs = pipe.run_many(datasets, ARGS["tol"], ARGS["mode"], rt_tol, ARGS["frag"], ARGS["batch"], p, shard=(r, world))
        per_rank.append((outs, [dict(l) for l in pipe.lasts]))
        assert sum(int(o[0].numel()) for o in outs) > 0                        # every rank gets real work
    merged = _merge(per_rank, [len(ds) for ds in datasets])
    for (sl, sm), (ml, mm) in zip(single, merged):
        want = _clusters(sl, sm)
        assert sum(len(k) > 1 for k in want) > 10                             # a non-trivial clustering
        assert _clusters(ml, mm) == want                                      # same partition, same medoid rows


@pytest.mark.parametrize("mz_interval", [1.0, 0.0])
def test_partition_runner_host_resident_exact(pipe, mz_interval):
    from falcon_amd.cluster.cluster import PartitionRunner
    # (large enough that the fixed uploads -- the 64 KiB window owner table of `window_select` per partition -- stay small
    # next to the peaks)
    host = _datasets(device=False, per=800)
    p = _params("complete", mz_interval=mz_interval)
    single = _single(pipe, host, p, None)
    total = sum(sum(np.asarray(t).nbytes for t in ds.columns() if t is not None) for ds in host)
    per_rank = []
    for r in range(2):
        runner = PartitionRunner(0, 2)
        try:
            outs = runner.run(host, ARGS["tol"], ARGS["mode"], None, ARGS["frag"], ARGS["batch"], p, shard=(r, 2))
            lasts = runner.lasts
            ctxs = [pl.ctx for pl in runner.pipelines] + ([runner._planner.ctx] if hasattr(runner, "_planner") else [])
            h2d = sum(c.h2d_bytes for c in ctxs)
        finally:
            runner.close()
        assert 0 < h2d <= 0.6 * total, (h2d, total)                          # a rank uploads its own rows' peaks only
        per_rank.append((outs, lasts))
    merged = _merge(per_rank, [len(ds) for ds in host])
    for (sl, sm), (ml, mm) in zip(single, merged):
        assert _clusters(ml, mm) == _clusters(sl, sm)


@pytest.mark.parametrize("exact", [True, False])
def test_partition_runner_world_one_through_gather_partitions(pipe, exact):
    """one rank (the CLI's `--distributed` at world size 1): the runner takes the unsharded path, and `gather_partitions`
    must hand its results back unchanged"""
    from falcon_amd import distributed as fdist
    from falcon_amd.cluster.cluster import PartitionRunner
    host = _datasets(device=False)
    p = _params("complete", exact=exact) if exact else _params("complete", t=0.35, min_matches=0, exact=False)
    single = _single(pipe, host, p, None)
    runner = PartitionRunner(0, 2)
    try:
        outs = runner.run(host, ARGS["tol"], ARGS["mode"], None, ARGS["frag"], ARGS["batch"], p, shard=(0, 1))
        merged = fdist.gather_partitions(outs, runner.lasts, [len(ds) for ds in host], pipe.ctx.tdev)
    finally:
        runner.close()
    for (sl, sm), (ml, mm) in zip(single, merged):
        assert np.array_equal(ml, sl) and np.array_equal(mm, sm)


def _one_peptide_per_bucket():
    """300 spectra of one peptide in each of two buckets: every pair has d <= 0.073, so complete linkage at 0.3 makes one
    cluster per bucket -- the nearest-neighbour graph stores n_neighbors pairs per row and cannot"""
    from falcon_amd.cluster.cluster import SpectrumDataset
    d = _spectra(1, 300, [600.0, 700.0], seed=11, drop=0.0, it_noise=0.3)
    return SpectrumDataset(d["precursor_mz"], d["retention_time"], d["mz"], d["intensity"], d["indptr"])


def test_run_sharded_exact_is_not_the_nearest_neighbour_answer(pipe):
    from falcon_amd import distributed as fdist
    ds = _one_peptide_per_bucket()
    p = _params("complete", t=0.3, min_matches=0, mz_interval=0.0)
    lab, med = _single(pipe, [ds], p, None)[0]
    assert len(med) == 2
    want = _clusters(lab, med)
    assert sorted(len(k) for k in want) == [300, 300]
    ann = _params("complete", t=0.3, min_matches=0, mz_interval=0.0, exact=False)     # the same data, nearest-neighbour path
    a_lab, a_med = _single(pipe, [ds], ann, None)[0]
    assert _clusters(a_lab, a_med) != want
    shards = [fdist.run_sharded(pipe, ds, ARGS["tol"], ARGS["mode"], None, ARGS["frag"], ARGS["batch"], p, rank=r,
                                world_size=2, local_only=True) for r in range(2)]
    assert all(len(s[0]) == 300 for s in shards)                              # one bucket per rank
    assert _clusters(*fdist.merge_shards(len(ds), shards)) == want


def test_wrapper_refuses_a_row_order_beyond_its_outputs(pipe):
    """a subset passed with dataset rows as `order` would make the kernel write labels_out[row] past an n_sub-row buffer: the
    wrapper rejects it on the host; the compact CSR of the same subset (order = arange) runs"""
    import torch
    from falcon_amd.cluster.cluster import ClusterPipeline
    ds = _datasets()[0]
    c = pipe.ctx
    n = len(ds)
    rows = torch.arange(n // 2, n, dtype=torch.int64, device=c.tdev)           # the upper half of the dataset's rows
    order, mzs = c.sort_by_precursor(ds.precursor_mz[rows])
    rows = rows[order]
    splits = np.array([0, len(rows)], np.int64)
    with pytest.raises(ValueError, match="row_order"):
        c.cluster_exact(ds.mz, ds.intensity, ds.indptr, rows, splits, 0.05, 0, 0.3, "complete", mzs, None, 20.0, "ppm", None)
    sub = ClusterPipeline._take_rows(c, ds, rows)
    assert int(sub.indptr[-1]) == int((ds.indptr[rows + 1] - ds.indptr[rows]).sum())
    local = torch.arange(len(rows), dtype=torch.int64, device=c.tdev)
    lab, med, _, _ = c.cluster_exact(sub.mz, sub.intensity, sub.indptr, local, splits, 0.05, 0, 0.3, "complete", mzs, None,
                                     20.0, "ppm", None)
    assert lab.numel() == len(rows) and int(lab.min()) == 0 and int(lab.max()) + 1 == med.numel()
