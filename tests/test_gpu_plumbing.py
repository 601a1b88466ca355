"""The helpers every stage goes through, each against plain numpy (tests/plumbing_cases.py) on both sides of its internal
thresholds: the device-wide exclusive scan (`device_scan_i32` / `device_scan_i64`, through the public entry points that call
it), `fal_sort_by_precursor`, `fal_gather_f32`, `fal_precursor_splits`, `fal_window_counts` and `fal_window_select`.

The scan has three forms (sortutil.hip `device_scan_t`): block sums + the fused apply up to 4,096 blocks of 1,024 elements,
inside which a block index above 1,024 (n > 1,049,600) takes a second round of the front-sum loop; and, past 4,194,304
elements, block sums -> the one-workgroup `exclusive_scan_kernel` -> `scan_apply_kernel` -> a copy of the total.

Not reachable at a size a test may have, and therefore not covered here: int32 inputs whose sum passes 2^31 (more than 2 G
output elements), and the int64 `cap` scan of `fal_decode_peaks` above 4,096 blocks, which needs more than 4 M zlib arrays.
The accumulation type is int64 in all three forms by inspection (`int64_t v`, `int64_t ws[]`, `int64_t* block_sums`)."""
import base64

import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import plumbing_cases as pc

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _np(t):
    return t.cpu().numpy()


def _same_f32(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# =========================================================================== scans
# ---- int32 flags: fal_window_select (flags -> scan -> compaction; the returned length is out[n], the total) ----------------
@pytest.fixture(scope="module")
def select_case(ctx):
    import torch
    pmz, owner = pc.select_input(max(pc.scan_lengths()), seed=5)
    owners = {"half": owner, "all": np.zeros(len(owner), np.int32), "none": np.ones(len(owner), np.int32)}
    return pmz, ctx.to_dev(pmz, torch.float32), pc.window_slot(pmz, 1.0), owners


@pytest.mark.parametrize("n", pc.scan_lengths())
def test_scan_i32_flags_through_window_select(ctx, select_case, n):
    """a wrong prefix anywhere moves a row: rows = the flagged positions compacted by the scan"""
    pmz, d_pmz, slot, owners = select_case
    assert 150 < len(np.unique(slot)) <= 200 and 0.4 < (owners["half"] == 0).mean() < 0.6
    for name, owner in owners.items():
        want_rows, want_mz = pc.window_select_ref(pmz[:n], 1.0, owner, 0, slot=slot[:n])
        rows, mz = ctx.window_select(d_pmz[:n], 1.0, owner, 0)
        assert rows.numel() == len(want_rows), (name, n, rows.numel(), len(want_rows))
        assert np.array_equal(_np(rows), want_rows), (name, n)
        assert _same_f32(_np(mz), want_mz), (name, n)
    assert len(pc.window_select_ref(pmz[:n], 1.0, owners["all"], 0, slot=slot[:n])[0]) == n
    assert len(pc.window_select_ref(pmz[:n], 1.0, owners["none"], 0, slot=slot[:n])[0]) == 0


# ---- int32 counts other than 0 / 1: fal_process_spectra with options that filter nothing --------------------------------------
PREP_SIZES = [1049601, 4194305]              # the fused form's second front-sum round; the three-launch form


@pytest.fixture(scope="module")
def counted_spectra(ctx):
    """max(PREP_SIZES) spectra of 0-3 peaks (m/z ascending inside a spectrum), on the device once; a shorter case is a prefix"""
    import torch
    n = max(PREP_SIZES)
    rng = np.random.default_rng(11)
    count = pc.small_counts(n, seed=11)
    indptr = pc.exclusive_scan_ref(count)
    nnz = int(indptr[-1])
    spec = np.repeat(np.arange(n, dtype=np.int64), count)
    within = np.arange(nnz, dtype=np.int64) - indptr[:-1][spec]
    mz = 100.0 + 300.0 * within + rng.uniform(0.0, 250.0, nnz)
    it = rng.uniform(0.1, 1000.0, nnz).astype(np.float32)
    dev = dict(mz=ctx.to_dev(mz, torch.float64), it=ctx.to_dev(it, torch.float32), indptr=ctx.to_dev(indptr, torch.int64),
               pmz=ctx.to_dev(np.full(n, 500.0), torch.float64), charge=ctx.to_dev(np.zeros(n, np.int32), torch.int32))
    return dict(count=count, indptr=indptr, spec=spec, mz32=mz.astype(np.float32), dev=dev)


@pytest.mark.parametrize("n", PREP_SIZES)
def test_scan_i32_counts_through_process_spectra(ctx, counted_spectra, n):
    cs, d = counted_spectra, counted_spectra["dev"]
    count = cs["count"][:n]
    want_ip = pc.exclusive_scan_ref(count)
    nnz = int(want_ip[-1])
    assert np.array_equal(want_ip, cs["indptr"][: n + 1]) and set(np.unique(count)) == {0, 1, 2, 3}
    valid, ip, omz, oit = ctx.process_spectra(d["mz"][:nnz], d["it"][:nnz], d["indptr"][: n + 1], d["pmz"][:n], d["charge"][:n],
                                              min_peaks=1, min_mz_range=0.0, mz_min=None, mz_max=None,
                                              remove_precursor_tolerance=None, min_intensity=None, max_peaks_used=None,
                                              scaling=None)
    assert np.array_equal(_np(valid), count >= 1)
    assert np.array_equal(_np(ip), want_ip)                                   # out_indptr = the scan of the counts, total included
    assert _same_f32(_np(omz), cs["mz32"][:nnz])                              # every peak at the offset the scan gave it
    oit = _np(oit).astype(np.float64)
    assert oit.shape == (nnz,) and np.isfinite(oit).all()
    norm2 = np.bincount(cs["spec"][:nnz], weights=oit * oit, minlength=n)
    assert np.abs(norm2[count >= 1] - 1.0).max() <= 1e-6                      # unit norm per spectrum (test_preprocess_cpu's bound)
    assert not norm2[count == 0].any()


# ---- int64 input: the per-spectrum peak counts of fal_decode_peaks -----------------------------------------------------------
DECODE_SIZES = [2000003, 4194305]            # (1,049,600, 4,194,304]: fused form, several front-sum rounds; the three-launch form
PAIR_COUNTS = [0, 1, 2, 4, 7, 3]             # values per array; twelve arrays, built in (m/z, intensity) pairs


@pytest.fixture(scope="module")
def shared_arrays():
    """a dozen uncompressed little-endian arrays that millions of spectra point at: m/z float64 ascending, intensity float32"""
    from falcon_amd import _lib
    from falcon_amd.ms_io.peak_payload import PeakChunk
    rng = np.random.default_rng(13)
    ch, mz_vals, it_vals = PeakChunk(), [], []
    for k in PAIR_COUNTS:
        mz = np.sort(rng.uniform(100.0, 2000.0, k))
        it = rng.uniform(1.0, 1e5, k).astype(np.float32)
        assert len(np.unique(mz)) == k
        r0 = ch.add_array(base64.b64encode(mz.astype("<f8").tobytes()), k, _lib.PEAK_F64)
        r1 = ch.add_array(base64.b64encode(it.astype("<f4").tobytes()), k, 0)
        assert r1 == r0 + 1
        mz_vals.append(mz)
        it_vals.append(it)
    payload, arrays, _ = ch.tables()
    choice = rng.integers(0, len(PAIR_COUNTS), max(DECODE_SIZES))
    return dict(payload=payload, arrays=arrays, choice=choice, mz=np.concatenate(mz_vals), it=np.concatenate(it_vals),
                off=pc.exclusive_scan_ref(np.array(PAIR_COUNTS))[:-1])


@pytest.mark.parametrize("n", DECODE_SIZES)
def test_scan_i64_through_decode_peaks(ctx, shared_arrays, n):
    sa = shared_arrays
    choice = sa["choice"][:n]
    spectra = np.stack([2 * choice, 2 * choice + 1], axis=1).astype(np.int64)
    count = np.asarray(PAIR_COUNTS, np.int64)[choice]
    want_ip = pc.exclusive_scan_ref(count)
    nnz = int(want_ip[-1])
    src = np.repeat(sa["off"][choice] - want_ip[:-1], count) + np.arange(nnz, dtype=np.int64)
    ip, mz, it, st = ctx.decode_peaks(sa["payload"], sa["arrays"], spectra)
    assert np.array_equal(_np(ip), want_ip)
    assert not _np(st).any()
    assert np.array_equal(_np(mz).view(np.int64), sa["mz"][src].view(np.int64))
    assert _same_f32(_np(it), sa["it"][src])


# =========================================================================== sort / gather
SORT_SIZES = [1, 2, 1000, 131071, 131072, 131073, 1500000]      # rocPRIM: merge sort below 131,072 keys, Onesweep from there on


@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_by_precursor_is_numpys_stable_argsort(ctx, n):
    wide = n >= 131073
    keys = pc.sort_keys(n, seed=n % 101, negatives=wide, nans=wide)
    want = np.argsort(keys, kind="stable")
    order, mzs = ctx.sort_by_precursor(keys)
    assert np.array_equal(_np(order), want)                                   # ties (-0.0 / +0.0 among them) keep input order
    assert _same_f32(_np(mzs), keys[want])
    # fal_gather_f32 with the same order (past 1,048,576 rows its capped grid of 4,096 x 256 threads strides): any bit pattern
    src = np.random.default_rng(n).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert _same_f32(_np(ctx.gather_f32(src, order)), src[want])


def test_gather_f32_repeated_rows_and_empty(ctx):
    import torch
    rng = np.random.default_rng(3)
    src = rng.standard_normal(1000).astype(np.float32)
    for n in (0, 1, 255, 256, 257, 1048576, 1048577, 1300001):
        idx = rng.integers(0, len(src), n).astype(np.int64)
        got = ctx.gather_f32(src, ctx.to_dev(idx, torch.int64))
        assert _same_f32(_np(got), src[idx]), n
    assert ctx.gather_f32(np.zeros(0, np.float32), ctx.empty((0,), torch.int64)).numel() == 0


# =========================================================================== fal_precursor_splits
K = pc.SPLITS_FIRST_READBACK
LADDER_BATCH = 64
RULES = [(0.0, False), (0.0, True), (1.0, False), (1.0, True)]


@pytest.fixture(scope="module")
def ladders():
    return {0: pc.gap_ladder(70001, 0), 1: pc.gap_ladder(70001, 1)}


def _splits_match(ctx, mz, tol, mode, batch, iv, chunk_last):
    got = ctx.precursor_splits(mz, tol, mode, batch, iv, chunk_last)
    want = fo.bucket_splits(mz, tol, mode, batch, iv, chunk_last)
    assert got.dtype == np.int64 and np.array_equal(got, want), (len(got), len(want))
    return want


@pytest.mark.parametrize("iv,chunk_last", RULES)
@pytest.mark.parametrize("tol,mode", [(20.0, "ppm"), (0.0045, "Da")])
def test_precursor_splits_second_readback(ctx, ladders, tol, mode, iv, chunk_last):
    """more than 65,536 gap positions: the rest comes back with a second pair of copies"""
    mz = ladders[0]
    assert len(pc.split_flag_positions(mz, tol, mode, iv)) > K
    want = _splits_match(ctx, mz, tol, mode, LADDER_BATCH, iv, chunk_last)
    assert len(want) > K + 1


@pytest.mark.parametrize("iv,chunk_last", RULES)
@pytest.mark.parametrize("n_flags", [K - 1, K, K + 1, K + 4])
def test_precursor_splits_at_the_readback_threshold(ctx, ladders, n_flags, iv, chunk_last):
    mz = pc.trim_to_flags(ladders[1], n_flags, 20.0, "ppm", iv)
    assert len(pc.split_flag_positions(mz, 20.0, "ppm", iv)) == n_flags
    _splits_match(ctx, mz, 20.0, "ppm", LADDER_BATCH, iv, chunk_last)
    _splits_match(ctx, mz, 20.0, "ppm", 3, iv, chunk_last)                    # a batch the ladder's short runs reach too


@pytest.mark.parametrize("iv,chunk_last", RULES)
def test_precursor_splits_degenerate_sizes(ctx, iv, chunk_last):
    for mz in ([], [500.0], [500.0, 500.001], [500.0, 500.5], [500.9, 501.0], [500.0, 500.0, 500.0]):
        mz = np.asarray(mz, np.float32)
        for batch in (1, 2, 64):
            _splits_match(ctx, mz, 20.0, "ppm", batch, iv, chunk_last)
            _splits_match(ctx, mz, 0.05, "Da", batch, iv, chunk_last)


# =========================================================================== fal_window_counts / fal_window_select
def _counts_match(ctx, parts, iv):
    got = ctx.window_counts(parts, iv)
    want = pc.window_counts_ref(parts, iv)
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, want.shape)     # the trimmed width included
    assert np.array_equal(got, want)
    return want


def _span(pmz, iv):
    s = pc.window_slot(pmz, iv)
    return int(s.max() - s.min() + 1)


def test_window_counts_lds_form(ctx):
    """interval 1.0 over 300 .. 1,500 m/z: ~1,200 occupied slots, counted in LDS bins"""
    pmz = np.random.default_rng(20).uniform(300.0, 1500.0, 100000).astype(np.float32)
    assert _span(pmz, 1.0) <= 12288
    want = _counts_match(ctx, [pmz], 1.0)
    assert want.shape == (1, 1500)


def test_window_counts_global_form_wraps(ctx):
    """interval 0.05 over 50 .. 2,000 m/z: the windows wrap around the table and span all of it, counted by global atomics"""
    pmz = np.random.default_rng(21).uniform(50.0, 2000.0, 100000).astype(np.float32)
    assert _span(pmz, 0.05) > 12288 and np.floor(pmz.astype(np.float64) / 0.05).max() > 2 * 16384
    want = _counts_match(ctx, [pmz], 0.05)
    assert want.shape[1] > 16000 and np.count_nonzero(want) > 16000


@pytest.mark.parametrize("span", [12287, 12288, 12289, 12290])
def test_window_counts_at_the_bin_limit(ctx, span):
    """kWindowBins = 12,288: the largest span counted in LDS, and the first one that is not"""
    rng = np.random.default_rng(span)
    lo = 100
    pmz = rng.uniform(lo, lo + span, 60000).astype(np.float32)
    pmz[:2] = [lo + 0.5, lo + span - 0.5]
    pmz = np.clip(pmz, lo + 0.25, lo + span - 0.25).astype(np.float32)
    rng.shuffle(pmz)
    assert _span(pmz, 1.0) == span
    # a second partition on the other side of the limit in the same launch: the form is chosen per partition
    other = rng.uniform(400.0, 900.0, 5000).astype(np.float32)
    _counts_match(ctx, [pmz, other], 1.0)


def _salt():
    edge = np.float32(819.2)
    return np.array([NAN, -1.0, -0.0, 0.0, INF, -INF, 3e38, edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1e9)),
                     16384.0, 16383.5, 16385.2, 500.0, np.nextafter(np.float32(500.0), np.float32(0))], np.float32)


@pytest.mark.parametrize("iv", [1.0, 0.05])
def test_window_counts_130_partitions(ctx, iv):
    """three rounds of the 64-partition launch, the last partial; empty partitions; one partition in a single window"""
    rng = np.random.default_rng(22)
    sizes = rng.integers(1, 50001, 130)
    sizes[[0, 64, 129]] = 0
    sizes[5], sizes[70] = 50000, 1
    parts = [rng.uniform(50.0, 2000.0, int(s)).astype(np.float32) for s in sizes]
    parts[33] = np.full(30000, 731.4, np.float32)
    parts[100] = np.concatenate([parts[100], _salt()])
    parts[128] = rng.uniform(300.0, 310.0, 777).astype(np.float32)            # the last round's only occupied partition but one
    want = _counts_match(ctx, parts, iv)
    assert want.sum(axis=1).tolist() == [len(p) for p in parts]
    assert np.count_nonzero(want[33]) == 1 and not want[[0, 64, 129]].any()


def test_window_counts_trimmed_width(ctx):
    assert ctx.window_counts([], 1.0).shape == (0, 0)
    empty = np.zeros(0, np.float32)
    assert _counts_match(ctx, [empty, empty], 1.0).shape == (2, 0)
    low = np.array([3.5, 0.25, 3.75], np.float32)
    assert _counts_match(ctx, [empty, low, np.array([1.5], np.float32)], 1.0).tolist() == [[0, 0, 0, 0], [1, 0, 0, 2], [0, 1, 0, 0]]
    assert _counts_match(ctx, [np.array([NAN, -3.0], np.float32)], 1.0).tolist() == [[2]]


@pytest.mark.parametrize("iv", [1.0, 0.05])
def test_window_special_values_counts_and_selection(ctx, iv):
    rng = np.random.default_rng(23)
    pmz = np.concatenate([rng.uniform(50.0, 2000.0, 5000).astype(np.float32), _salt(), _salt()])
    rng.shuffle(pmz)
    want = _counts_match(ctx, [pmz], iv)
    assert want.shape[1] == 16384                                             # +inf and 3e38 sit in the last slot
    owner = rng.integers(0, 3, want.shape[1]).astype(np.int32)
    seen = []
    for rank in range(3):
        want_rows, want_mz = pc.window_select_ref(pmz, iv, owner, rank)
        rows, mz = ctx.window_select(pmz, iv, owner, rank)
        assert np.array_equal(_np(rows), want_rows) and _same_f32(_np(mz), want_mz), rank
        seen.append(want_rows)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(len(pmz)))


@pytest.mark.parametrize("iv", [1.0, 0.05])
def test_window_deal_end_to_end(ctx, iv):
    """counts -> the deal the product derives from them (`distributed.window_costs` + `deal_job`, as
    `ClusterPipeline.plan_shards`) -> selection: every rank's rows ascending, the ranks' rows a partition of the dataset, no
    window on two ranks"""
    from falcon_amd import distributed as fdist
    world = 3
    rng = np.random.default_rng(24)
    parts = [rng.uniform(300.0, 1500.0, 60000).astype(np.float32), rng.normal(700.0, 80.0, 25000).astype(np.float32),
             np.zeros(0, np.float32), np.concatenate([rng.uniform(50.0, 2000.0, 9000).astype(np.float32), _salt()])]
    counts = ctx.window_counts(parts, iv)
    assert np.array_equal(counts, pc.window_counts_ref(parts, iv))
    costs = fdist.window_costs(counts, 2 ** 15, 16, iv, (20.0, "ppm"), 128, 64)
    owners = fdist.deal_job(list(costs), world)
    assert len(owners) == len(parts) and all(len(o) == counts.shape[1] for o in owners)
    assert any(len(np.unique(o)) == world for o in owners)                    # windows were dealt, not whole partitions
    for pmz, owner in zip(parts, owners):
        slot = pc.window_slot(pmz, iv)
        rank_of_row = np.full(len(pmz), -1, np.int64)
        for rank in range(world):
            want_rows, want_mz = pc.window_select_ref(pmz, iv, owner, rank, slot=slot)
            rows, mz = ctx.window_select(pmz, iv, owner, rank)
            rows = _np(rows)
            assert np.all(np.diff(rows) > 0)
            assert np.array_equal(rows, want_rows) and _same_f32(_np(mz), want_mz)
            assert np.all(rank_of_row[rows] == -1)                            # no row twice
            rank_of_row[rows] = rank
        assert np.all(rank_of_row >= 0)                                       # every row on a rank
        lo = np.full(pc.N_WINDOWS, world, np.int64)
        hi = np.full(pc.N_WINDOWS, -1, np.int64)
        np.minimum.at(lo, slot, rank_of_row)
        np.maximum.at(hi, slot, rank_of_row)
        assert np.all((lo == hi) | (hi == -1))                                # a window's rows all on one rank
