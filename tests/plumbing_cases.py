"""References and input builders shared by the plumbing tests (test_plumbing_cpu.py, test_gpu_plumbing.py): the device-wide
exclusive scan, the precursor windows the multi-GPU front end deals out, and the precursor ladder that takes
`fal_precursor_splits` past its first readback.  Plain numpy: no torch, no GPU."""
import numpy as np

N_WINDOWS = 1 << 14              # `Context.N_WINDOWS`: deal units the multi-GPU front end counts
SPLITS_FIRST_READBACK = 65536    # gap positions `fal_precursor_splits` brings back with its first copy


# --------------------------------------------------------------------------- references
def window_slot(pmz_f32, interval, n_windows=N_WINDOWS):
    """Slot of every spectrum in the table of `n_windows` deal units, as the comment of `window_of` (sortutil.hip) states it:
    w = floor(float64(float32 m/z) / interval); NaN and negative -> slot 0; +inf, or a quotient of 9e15 and more -> the last
    slot; windows beyond the table wrap around (w mod n_windows)."""
    mz = np.asarray(pmz_f32, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w = np.floor(mz / np.float64(interval))
        slot = np.where(w < n_windows, w, np.fmod(w, np.float64(n_windows)))
        slot = np.where(~(w < 9.0e15), np.float64(n_windows - 1), slot)
        slot = np.where(~(w >= 0.0), 0.0, slot)
    return slot.astype(np.int64)


def window_counts_ref(list_of_pmz, interval, n_windows=N_WINDOWS):
    """What `Context.window_counts` documents: int64 [n_parts, width], spectra per slot of every partition; width = 1 + the
    largest occupied slot over all partitions (0 when no partition holds a spectrum)."""
    full = np.zeros((len(list_of_pmz), n_windows), np.int64)
    for p, pmz in enumerate(list_of_pmz):
        if len(pmz):
            full[p] = np.bincount(window_slot(pmz, interval, n_windows), minlength=n_windows)
    occupied = np.flatnonzero(full.any(axis=0))
    width = int(occupied[-1]) + 1 if len(occupied) else 0
    return full[:, :width]


def window_select_ref(pmz, interval, owner, rank, n_windows=N_WINDOWS, slot=None):
    """The spectra whose slot `owner` gives to `rank` -> ascending dataset rows (int64) and their float32 m/z.  `owner` covers
    the counted slots only and is padded as `Context.window_select` pads it: with its last entry (-1 when empty).
    `slot`: `window_slot(pmz, interval, n_windows)`, for a caller that selects from the same spectra more than once."""
    pmz = np.asarray(pmz, np.float32)
    own = np.full(n_windows, -1, np.int64)
    own[:len(owner)] = owner
    if len(owner):
        own[len(owner):] = owner[-1]
    if slot is None:
        slot = window_slot(pmz, interval, n_windows)
    assert len(slot) == len(pmz)
    rows = np.flatnonzero(own[slot] == rank).astype(np.int64)
    return rows, pmz[rows]


def exclusive_scan_ref(v):
    """out[i] = sum of v[:i] for i = 0 .. n (n + 1 entries, the last is the total), accumulated in int64"""
    return np.concatenate([[0], np.cumsum(v, dtype=np.int64)]).astype(np.int64)


# --------------------------------------------------------------------------- input builders, named by what they hit
def scan_lengths():
    """Lengths on each side of every edge of `device_scan_t` (sortutil.hip): the 64-lane wave, the 1,024-element block, the
    front-sum loop of the fused form (a block index above 1,024: n > 1,049,600 takes a second round), and the 4,096-block
    switch to the three-launch form (n > 4,194,304)."""
    return [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 65537, 1048576, 1049600, 1049601, 1050625, 4194304, 4194305, 5000001]


def select_input(n, seed=0, lo=400.0, hi=600.0):
    """float32 precursor m/z over the ~200 unit windows [lo, hi), and an owner table over the counted slots that gives about
    half of them to rank 0 in no regular pattern"""
    rng = np.random.default_rng(seed)
    pmz = rng.uniform(lo, hi, n).astype(np.float32)
    owner = rng.integers(0, 2, int(hi)).astype(np.int32)
    return pmz, owner


def small_counts(n, seed=0, high=4):
    """int32 counts 0 .. high-1 per element: scan input other than 0 / 1 flags"""
    return np.random.default_rng(seed).integers(0, high, n).astype(np.int32)


def gap_ladder(n, seed, n_runs=4):
    """Ascending float32 precursor m/z in which almost every spectrum is a bucket of its own: 200 * prod(1 + step), step =
    30 ppm (a gap at a 20 ppm tolerance) with probability 0.97, else 2 ppm (none); `n_runs` runs of 200-300 rows 2 ppm
    apart are spliced in, so that blocks longer than a small batch size occur next to the many short ones.  70,001 rows end
    near 1,500 m/z and hold more than 65,536 gaps: `fal_precursor_splits` needs its second readback."""
    rng = np.random.default_rng(seed)
    step = np.where(rng.random(max(n - 1, 0)) < 0.97, 30e-6, 2e-6)
    for r in range(n_runs):
        length = int(rng.integers(200, 301))
        if n - 1 > 2 * length:
            a = int(rng.integers(0, n - 1 - length)) if r else (n - 1) // 3        # (the first run at a fixed place)
            step[a:a + length] = 2e-6
    return (200.0 * np.cumprod(np.concatenate([[1.0], 1.0 + step]))[:n]).astype(np.float32)


def split_flag_positions(mz_f32, tol, mode, mz_interval):
    """rows i >= 1 at which `split_flags_kernel` raises a flag: a precursor gap above `tol` (float32 difference and division,
    float64 product with 1e6: the typing of the oracle's `mass_diff`) or, with mz_interval > 0, a change of the window
    floor(m/z / mz_interval)"""
    mz = np.asarray(mz_f32, np.float32)
    if len(mz) < 2:
        return np.zeros(0, np.int64)
    diff = mz[1:] - mz[:-1]
    md = diff.astype(np.float64) if mode == "Da" else (diff / mz[:-1]).astype(np.float32).astype(np.float64) * 1e6
    flag = md > tol
    if mz_interval and mz_interval > 0:
        w = np.floor(mz.astype(np.float64) / np.float64(mz_interval))
        flag |= w[1:] != w[:-1]
    return np.flatnonzero(flag).astype(np.int64) + 1


def trim_to_flags(mz_f32, n_flags, tol, mode, mz_interval):
    """the shortest prefix of the ladder that holds exactly `n_flags` flagged rows (its last row is the last flagged one)"""
    at = split_flag_positions(mz_f32, tol, mode, mz_interval)
    assert len(at) >= n_flags >= 1, (len(at), n_flags)
    return np.asarray(mz_f32, np.float32)[: int(at[n_flags - 1]) + 1]


def sort_keys(n, seed=0, negatives=False, nans=False):
    """float32 sort keys with heavy ties (about n / 50 distinct values) plus +0.0, -0.0, a denormal, FLT_MAX and +inf; on
    request a block of negative finite values and a few canonical NaN (payload 0x7FC00000)"""
    rng = np.random.default_rng(seed)
    pool = rng.uniform(100.0, 2000.0, max(n // 50, 1)).astype(np.float32)
    keys = pool[rng.integers(0, len(pool), n)]
    special = np.array([0.0, -0.0, 1e-40, np.finfo(np.float32).max, np.inf, -0.0, 0.0, np.inf], np.float32)
    if n >= 2:
        at = rng.choice(n, min(n, 4 * len(special)), replace=False)
        keys[at] = special[np.arange(len(at)) % len(special)]
    if negatives and n >= 1000:
        a = int(rng.integers(0, n - n // 10))
        keys[a:a + n // 10] = -pool[rng.integers(0, len(pool), n // 10)]
    if nans and n >= 1000:
        keys[rng.choice(n, 7, replace=False)] = np.uint32(0x7FC00000).view(np.float32)
    return keys
