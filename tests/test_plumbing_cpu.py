"""The references of tests/plumbing_cases.py on hand-written values, and the properties of its input builders that
test_gpu_plumbing.py relies on.  The CPU suites replace `Context.window_counts` / `window_select` with fakes; this file is
what ties the contract of those fakes to a stated reference."""
import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import plumbing_cases as pc

NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("mz,slot", [(16383.5, 16383), (16384.0, 0), (16385.2, 1), (-1.0, 0), (-0.0, 0), (NAN, 0),
                                     (INF, 16383), (3e38, 16383), (0.0, 0), (0.999, 0), (1.0, 1), (-INF, 0)])
def test_window_slot_unit_interval(mz, slot):
    assert pc.window_slot(np.array([mz], np.float32), 1.0, 16384).tolist() == [slot]


@pytest.mark.parametrize("mz,slot", [(819.15, 16383), (819.2, 0), (1500.0, 30000 - 16384)])
def test_window_slot_small_interval_wraps(mz, slot):
    """interval 0.05: the table of 16,384 windows ends at 819.2 m/z, everything above wraps around (float32(819.15) =
    819.150024..., float32(819.2) = 819.200012...: both just above their decimal, so 16,383 and 16,384 -> 0)"""
    assert pc.window_slot(np.array([mz], np.float32), 0.05, 16384).tolist() == [slot]


def test_window_slot_large_quotient_goes_to_the_last_slot():
    # quotient >= 9e15: the last slot; just below: wrapped like any other window
    iv = 1e-12
    w_small = np.floor(np.float64(np.float32(8000.0)) / iv)
    assert w_small < 9.0e15
    assert pc.window_slot(np.array([8000.0, 9500.0], np.float32), iv, 16384).tolist() == [int(np.fmod(w_small, 16384.0)), 16383]


def test_window_slot_vector_matches_scalars():
    v = np.array([16383.5, NAN, 3.25, -2.0, INF, 40000.75, -0.0], np.float32)
    assert pc.window_slot(v, 1.0, 16384).tolist() == [16383, 0, 3, 0, 16383, 40000 - 2 * 16384, 0]
    assert pc.window_slot(np.zeros(0, np.float32), 1.0).shape == (0,)


def _parts(rng):
    return [rng.uniform(50, 2000, 3000).astype(np.float32), np.zeros(0, np.float32),
            np.full(17, 700.25, np.float32), np.array([NAN, -1.0, INF, 3e38, 819.2], np.float32)]


@pytest.mark.parametrize("iv", [1.0, 0.05])
def test_window_counts_ref_rows_sum_to_partition_sizes(iv):
    parts = _parts(np.random.default_rng(0))
    c = pc.window_counts_ref(parts, iv)
    assert c.dtype == np.int64 and c.shape[0] == len(parts)
    assert c.sum(axis=1).tolist() == [len(p) for p in parts]
    assert c[:, -1].any()                                                     # the width is trimmed to the last occupied slot
    assert c.shape[1] == 16384                                                # (+inf sits in the last slot)
    assert c[2].max() == 17 and np.count_nonzero(c[2]) == 1
    assert pc.window_counts_ref(parts[:3], 1.0).shape[1] == int(np.floor(parts[0].max())) + 1
    assert pc.window_counts_ref([parts[1]], 1.0).shape == (1, 0)
    assert pc.window_counts_ref([], 1.0).shape == (0, 0)


@pytest.mark.parametrize("iv", [1.0, 0.05])
def test_window_select_ref_partitions_the_rows(iv):
    rng = np.random.default_rng(1)
    pmz = np.concatenate(_parts(rng))
    rng.shuffle(pmz)
    width = pc.window_counts_ref([pmz], iv).shape[1]
    owner = rng.integers(0, 3, width).astype(np.int32)
    got = [pc.window_select_ref(pmz, iv, owner, r) for r in range(3)]
    rows = np.concatenate([g[0] for g in got])
    assert np.array_equal(np.sort(rows), np.arange(len(pmz)))                 # every row on exactly one rank
    slot = pc.window_slot(pmz, iv)
    for r, (rw, mz) in enumerate(got):
        assert rw.dtype == np.int64 and np.all(np.diff(rw) > 0)
        assert np.array_equal(mz.view(np.uint32), pmz[rw].view(np.uint32))
        assert np.all(owner[slot[rw]] == r)


def test_window_select_ref_pads_the_owner_table():
    pmz = np.array([1.5, 7.5, 2.5], np.float32)
    assert pc.window_select_ref(pmz, 1.0, np.array([0, 0, 1], np.int32), 1)[0].tolist() == [1, 2]     # slot 7 -> owner[-1]
    assert pc.window_select_ref(pmz, 1.0, np.zeros(0, np.int32), 0)[0].tolist() == []                # no owner: nobody's
    assert pc.window_select_ref(pmz, 1.0, np.zeros(0, np.int32), -1)[0].tolist() == [0, 1, 2]


def test_exclusive_scan_ref():
    assert pc.exclusive_scan_ref(np.array([3, 0, 2], np.int32)).tolist() == [0, 3, 3, 5]
    assert pc.exclusive_scan_ref(np.zeros(0, np.int32)).tolist() == [0]
    big = pc.exclusive_scan_ref(np.full(3, 2 ** 30, np.int32))
    assert big.dtype == np.int64 and big[-1] == 3 * 2 ** 30                   # accumulated in int64


def test_scan_lengths_sit_on_both_sides_of_every_edge():
    L = pc.scan_lengths()
    assert L == sorted(set(L)) and L[0] == 0
    for edge in (64, 1024, 1024 * 1025, 4096 * 1024):                         # wave, block, front-sum loop, three-launch form
        assert edge in L and edge + 1 in L
    assert any(1024 * 1025 < n <= 4096 * 1024 for n in L) and L[-1] > 4096 * 1024 + 1


LADDER_BATCH = 64


def test_gap_ladder_needs_the_second_readback():
    mz = pc.gap_ladder(70001, 0)
    assert mz.dtype == np.float32 and len(mz) == 70001
    assert np.all(np.diff(mz) >= 0) and 1400 < mz[-1] < 1700
    assert len(pc.split_flag_positions(mz, 20.0, "ppm", 0.0)) > pc.SPLITS_FIRST_READBACK
    plain = fo.bucket_splits(mz, 20.0, "ppm", LADDER_BATCH, 0.0, False)
    assert len(plain) > 65537
    ref = fo.get_precursor_mz_splits(mz, 20.0, "ppm", LADDER_BATCH)
    assert np.array_equal(plain, ref)                                         # both build rules off: the reference's rule
    # blocks on both sides of the batch size: the spliced runs are chunked, the rest is shorter than a batch
    gaps = np.concatenate([[0], pc.split_flag_positions(mz, 20.0, "ppm", 0.0), [len(mz)]])
    blocks = np.diff(gaps)
    assert (blocks >= LADDER_BATCH).sum() >= 2 and (blocks < LADDER_BATCH).sum() > 60000
    assert np.diff(plain).max() <= LADDER_BATCH or blocks[-1] >= LADDER_BATCH  # (only the last block may stay unchunked)
    assert len(plain) > len(gaps)                                             # chunking added boundaries
    both = fo.bucket_splits(mz, 20.0, "ppm", LADDER_BATCH, 1.0, True)
    assert len(both) > len(plain)                                             # window cuts inside gap-free runs
    assert not np.array_equal(pc.gap_ladder(70001, 1), mz)


@pytest.mark.parametrize("iv", [0.0, 1.0])
@pytest.mark.parametrize("k", [65536, 65537, 65540])
def test_trim_to_flags_is_exact(k, iv):
    mz = pc.trim_to_flags(pc.gap_ladder(70001, 1), k, 20.0, "ppm", iv)
    at = pc.split_flag_positions(mz, 20.0, "ppm", iv)
    assert len(at) == k and at[-1] == len(mz) - 1


def test_da_tolerance_scaled_to_the_ladder():
    """0.0045 Da lies between the ladder's two steps at every m/z (2 ppm of 1,600 = 0.0032; 30 ppm of 200 = 0.006)"""
    mz = pc.gap_ladder(70001, 0)
    assert np.array_equal(pc.split_flag_positions(mz, 0.0045, "Da", 0.0), pc.split_flag_positions(mz, 20.0, "ppm", 0.0))


def test_sort_keys_hold_ties_and_the_special_values():
    k = pc.sort_keys(131073, 3, negatives=True, nans=True)
    bits = k.view(np.uint32)
    assert len(np.unique(k[np.isfinite(k)])) < 2 * (131073 // 50) + 8
    for b in (0x00000000, 0x80000000, 0x7F800000, 0x7F7FFFFF, 0x7FC00000):
        assert (bits == b).any(), hex(b)
    assert ((k > 0) & (k < np.finfo(np.float32).tiny)).any() and (k < 0).sum() > 10000
    assert np.isnan(k).sum() == 7 and np.all(bits[np.isnan(k)] == 0x7FC00000)
    order = np.argsort(k, kind="stable")
    z = np.flatnonzero(k[order] == 0)
    assert len(z) >= 4 and np.all(np.diff(order[z]) > 0)                      # -0.0 and +0.0 tie: input order kept
    assert len(set(bits[order[z]].tolist())) == 2
    assert np.isnan(k[order[-7:]]).all()                                      # NaN last
    small = pc.sort_keys(2, 0)
    assert sorted(small.view(np.uint32).tolist()) == [0, 0x80000000]
