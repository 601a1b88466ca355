"""Exact mode on several GPUs, the host side: the cost model that prices pairs (`distributed.exact_bucket_costs` /
`exact_window_costs`), the deals built on it (`_restrict`, `plan_shards`), the compact CSR of a host-resident subset, the
labels-only gather of a multi-partition result at world size 1, the shared parameter resolution and the `--distributed`
switch of the CLI.  No GPU: the pipeline methods run against a stand-in context on CPU tensors."""
import numpy as np
import pytest

from falcon_amd import distributed as fdist
from falcon_amd.cluster.cluster import AnnParams, ClusterPipeline, SpectrumDataset, n_list_rule, resolve_params


def test_exact_costs_are_pairs_plus_the_row_term():
    w = fdist.EXACT_ROW_UNITS
    got = fdist.exact_bucket_costs(np.array([0, 1, 2, 10, 300]))
    assert np.array_equal(got, [0.0, w, 1 + 2 * w, 45 + 10 * w, 300 * 299 / 2 + 300 * w])
    # windows: ceil(count / batch_size) buckets of count / chunks rows
    b = 32768
    got = fdist.exact_window_costs(np.array([[0, 10, b, 2 * b + 2]]), b)
    assert got.shape == (1, 4)
    size = (2 * b + 2) / 3
    np.testing.assert_allclose(got[0], [0.0, 45 + 10 * w, b * (b - 1) / 2 + b * w, 3 * size * (size - 1) / 2 + (2 * b + 2) * w])
    # a window under batch_size costs what its one bucket costs
    c = np.arange(0, 2000, 7)
    np.testing.assert_allclose(fdist.exact_window_costs(c, b), fdist.exact_bucket_costs(c))


def _job(seed=0):
    """a few large buckets among many small ones"""
    rng = np.random.default_rng(seed)
    return rng.permutation(np.concatenate([[3000, 2800, 2600, 2400], rng.integers(20, 400, 600)]))


def _loads(owner, costs, world):
    return np.bincount(owner, weights=costs, minlength=world)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_exact_deal_is_deterministic_and_balanced(world):
    sizes = _job()
    costs = fdist.exact_bucket_costs(sizes)
    owner = fdist.shard_units(costs, world)
    assert np.array_equal(owner, fdist.shard_units(fdist.exact_bucket_costs(sizes.copy()), world))
    assert owner.shape == sizes.shape and owner.min() >= 0 and owner.max() < world      # one owner per bucket
    loads = _loads(owner, costs, world)
    assert loads.min() > 0 and loads.max() <= 1.03 * loads.mean(), loads / loads.mean()
    # the nearest-neighbour cost model prices the same buckets differently (the IVF buckets probe n_probe of their lists):
    # its deal of this job is another one, and under the exact costs it is worse
    ann = fdist.shard_units(fdist.bucket_costs(sizes, n_list_rule(sizes, 16), 16), world)
    assert not np.array_equal(owner, ann)
    assert _loads(ann, costs, world).max() > loads.max()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_exact_window_deal_of_a_job(world):
    rng = np.random.default_rng(1)
    counts = rng.integers(0, 1500, (2, 900))
    counts[0, [100, 400, 700]] = [6000, 9000, 12000]                     # a few large windows among many small ones
    costs = fdist.exact_window_costs(counts, 32768)
    a, b = fdist.deal_job(list(costs), world), fdist.deal_job(list(costs), world)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert [len(x) for x in a] == [900, 900] and all(x.min() >= 0 and x.max() < world for x in a)
    loads = np.bincount(np.concatenate(a), weights=np.concatenate(costs), minlength=world)
    assert loads.max() <= 1.05 * loads.mean(), loads / loads.mean()


# ------------------------------------------------------------------------------------------------------- pipeline pieces
class _CpuCtx:
    """the bits of `device.Context` the host logic of `_restrict` / `plan_shards` / `_take_rows` calls, on CPU tensors"""
    def __init__(self, counts=None):
        import torch
        self.tdev = torch.device("cpu")
        self.counts = counts

    def to_dev(self, a, dtype=None):
        import torch
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(dtype) if dtype is not None else t

    def window_counts(self, pmzs, mz_interval):
        return self.counts


def _state(splits):
    import torch
    n = int(splits[-1])
    return dict(order=torch.arange(n, dtype=torch.int64).flip(0), mzs=torch.arange(n, dtype=torch.float32), rts=None,
                splits=np.asarray(splits, np.int64), n_list=n_list_rule(np.diff(splits), 16))


def test_restrict_deals_exact_buckets_on_pair_costs():
    sizes = _job(2)
    splits = np.concatenate([[0], np.cumsum(sizes)])
    pipe = ClusterPipeline.__new__(ClusterPipeline)
    c = _CpuCtx()
    p_exact = AnnParams(exact=True)
    want = fdist.shard_units(fdist.exact_bucket_costs(sizes), 4)
    rows_seen = []
    for r in range(4):
        sub = pipe._restrict(c, _state(splits), p_exact, (r, 4))
        assert np.array_equal(sub["buckets"], np.flatnonzero(want == r))
        assert np.array_equal(np.diff(sub["splits"]), sizes[want == r])
        rows_seen.append(sub["rows"].numpy())
    rows = np.concatenate(rows_seen)
    assert np.array_equal(np.sort(rows), np.arange(splits[-1]))            # every row on exactly one rank


def test_plan_shards_prices_exact_windows():
    counts = np.random.default_rng(3).integers(0, 3000, (2, 300))
    counts[1, 5] = 50000

    class _Ds:
        precursor_mz = None

        def on_host(self):
            return False
    pipe = ClusterPipeline.__new__(ClusterPipeline)
    got = pipe.plan_shards(_CpuCtx(counts), [_Ds(), _Ds()], 32768, AnnParams(exact=True), 4, tol=(20.0, "ppm"))
    want = fdist.deal_job(list(fdist.exact_window_costs(counts, 32768)), 4)
    ann = pipe.plan_shards(_CpuCtx(counts), [_Ds(), _Ds()], 32768, AnnParams(), 4, tol=(20.0, "ppm"))
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert not all(np.array_equal(x, y) for x, y in zip(got, ann))


def test_take_rows_of_a_host_dataset_is_a_compact_csr():
    import torch
    rng = np.random.default_rng(4)
    cnt = rng.integers(0, 9, 50)
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    mz = rng.random(indptr[-1]).astype(np.float32)
    it = rng.random(indptr[-1]).astype(np.float32)
    ds = SpectrumDataset(rng.random(50).astype(np.float32), None, mz, it, indptr)
    rows = torch.tensor([7, 3, 49, 0, 22], dtype=torch.int64)
    sub = ClusterPipeline._take_rows(_CpuCtx(), ds, rows)
    ip = sub.indptr.numpy()
    assert ip[0] == 0 and len(ip) == len(rows) + 1
    for i, r in enumerate(rows.tolist()):
        assert np.array_equal(sub.mz.numpy()[ip[i]:ip[i + 1]], mz[indptr[r]:indptr[r + 1]])
        assert np.array_equal(sub.intensity.numpy()[ip[i]:ip[i + 1]], it[indptr[r]:indptr[r + 1]])


def test_gather_partitions_at_world_size_one():
    """labels by dataset row and medoid rows from a rank's subset contract (world size 1: no collective)"""
    import torch
    rows0 = torch.tensor([4, 0, 2, 1, 3], dtype=torch.int64)               # subset positions -> dataset rows
    lab0 = torch.tensor([0, 1, 0, 1, 2], dtype=torch.int32)
    med0 = torch.tensor([2, 1, 4], dtype=torch.int32)                      # positions into the subset
    outs = [(lab0, med0), (torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))]
    lasts = [{"rows": rows0}, {"rows": torch.zeros(0, dtype=torch.int64)}]
    (l0, m0), (l1, m1) = fdist.gather_partitions(outs, lasts, [5, 0], torch.device("cpu"))
    assert np.array_equal(l0, [1, 1, 0, 2, 0]) and np.array_equal(m0, [2, 0, 3])
    assert len(l1) == 0 and len(m1) == 0


def test_gather_partitions_of_an_unsharded_run():
    """world size 1: `PartitionRunner.run(shard=(0, 1))` runs `ClusterPipeline.run`, whose `last` has no "rows" and whose
    labels / medoids are by dataset row already -- the result passes through unchanged"""
    import torch
    lab = torch.tensor([1, 0, 1, 2, 0], dtype=torch.int32)
    med = torch.tensor([4, 2, 3], dtype=torch.int32)                       # dataset rows
    last = {"order": torch.tensor([1, 4, 0, 2, 3]), "splits": np.array([0, 5])}   # what `_exact` / `_graph` leave
    empty = (torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    (l0, m0), (l1, m1) = fdist.gather_partitions([(lab, med), empty], [last, dict(last)], [5, 0], torch.device("cpu"))
    assert np.array_equal(l0, lab.numpy()) and np.array_equal(m0, med.numpy())
    assert len(l1) == 0 and len(m1) == 0
    with pytest.raises(ValueError, match="no \"rows\""):
        fdist.gather_partitions([(lab[:3], med)], [last], [5], torch.device("cpu"))


def test_resolve_params_is_the_single_rule():
    p = resolve_params("average", 0.3, 2, AnnParams(eps=0.3, exact=True))
    assert p.exact and p.clustering == "hierarchical" and p.linkage == "average" and p.rescore and p.min_matches == 2
    q = resolve_params("complete", 0.1, 5, None)
    assert q.clustering == "dbscan" and not q.rescore and q.min_matches == 0
    with pytest.raises(ValueError, match="differ"):
        resolve_params("complete", 0.2, 0, AnnParams(eps=0.1))
    with pytest.raises(ValueError, match="dbscan"):
        resolve_params("complete", 0.1, 0, AnnParams(exact=True, clustering="dbscan"))
    with pytest.raises(ValueError, match="only applies"):
        resolve_params("single", 0.1, 0, AnnParams())


def test_distributed_switch_parses_and_stays_out_of_the_header():
    from falcon_amd.config import config
    from falcon_amd.falcon import _option_lines
    config.parse(["in.mgf", "out"])
    assert config.distributed is False
    plain = _option_lines()
    config.parse(["in.mgf", "out", "--distributed", "--exact"])
    assert config.distributed is True
    lines = _option_lines()
    assert not any("distributed" in line for line in lines)
    config.parse(["in.mgf", "out", "--exact"])
    assert _option_lines() == lines and len(lines) == len(plain)
