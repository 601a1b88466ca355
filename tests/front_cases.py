"""Case builders for the per-spectrum kernels in front of the search (`fal_process_spectra`, `fal_vectorize_rows`,
`fal_to_vector_indices`, `fal_rescore_neighbors`) at the sizes where their launch shape changes.  Pure numpy: shared by
test_front_cases_cpu.py (the builders against the oracle alone) and test_gpu_front_shapes.py / front_poison_worker.py.

Every size is a function of the device's CU count (`num_cus` of the context), restated here from the host code:
  vectorize          chunk = 16, halved while n / chunk < cus * 32 * 4 rows; grid min(ceil(n / chunk), cus * 32) waves
  process_spectra    min(ceil(n / 4), cus * 64) blocks of four waves, one spectrum per wave: cus * 256 spectra per grid turn
  to_vector_indices  cus * 8 blocks of 256 values
  rescore_neighbors  cus * 32 blocks of 256 slots
The oracle is run on a small LIBRARY of spectra only; a large case gathers library rows, and so does its expected output."""
import functools

import numpy as np

from oracle import falcon_oracle as fo
from tests import peakmatch_cases as pc
from tests.prep_cases import OPTION_SETS, raw_spectra

f32, f64 = np.float32, np.float64
MZ_LO, MZ_HI, BIN = 101.0, 1500.0, 0.05            # falcon's default vector geometry


def csr_gather(indptr, pick, *arrays):
    """rows `pick` (any order, repeats allowed) of a CSR -> (new indptr, the arrays' gathered values)"""
    indptr = np.asarray(indptr, np.int64)
    pick = np.asarray(pick, np.int64)
    counts = np.diff(indptr)[pick]
    ip = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pos = np.repeat(indptr[:-1][pick] - ip[:-1], counts) + np.arange(ip[-1])
    return (ip,) + tuple(np.asarray(a)[pos] for a in arrays)


# ---------------------------------------------------------------------------------------------------------------- vectorize
def vectorize_chunk(n, cus):
    """rows a wave takes per turn (csrc/vectorize.hip, vectorize_impl)"""
    chunk = 16
    while chunk > 1 and n // chunk < cus * 32 * 4:
        chunk >>= 1
    return chunk


def vectorize_n(chunk, cus):
    """the case size of a chunk: a partial last chunk, a block count that is no multiple of the grid; chunk 1: the last size
    that still takes it"""
    T = cus * 128
    return 2 * T - 1 if chunk == 1 else chunk * T + 37


#                 chunk, low_dim, width, output mode, normalize
VECTORIZE_CASES = [(2, 400, 400, "f32", True), (2, 400, 400, "f16", True),
                   (2, 50, 64, "f32", True), (2, 50, 64, "f16", True), (2, 50, 64, "split16", True),
                   (2, 50, 64, "f32+f16", True), (2, 50, 64, "f16+image", True), (2, 50, 64, "f32", False),
                   (4, 50, 64, "f32", True), (4, 50, 64, "f32+f16", True),
                   (8, 5, 8, "f32", True), (8, 5, 8, "f16+image", True),
                   (16, 8, 8, "f32", True), (16, 8, 8, "split16", True),
                   (1, 50, 64, "f32", True)]


@functools.lru_cache(maxsize=None)
def vec_library(seed=11):
    """-> dict: the library CSR (mz f32 sorted per row, intensity f32, indptr), the geometry (n_bins, min_mz), `row` = name ->
    library row of the deterministic spectra, `short` / `long` = the rows of at most / more than 64 peaks"""
    rng = np.random.default_rng(seed)
    n_bins, start, _ = fo.get_dim(MZ_LO, MZ_HI, BIN)
    rows, names = [], {}

    def add(name, m):
        if name is not None:
            names[name] = len(rows)
        rows.append(np.sort(np.asarray(m, f64)).astype(f32))

    for p in (0, 1, 2, 63, 64, 65, 127, 128, 129, 200):
        add(p, rng.uniform(MZ_LO + 0.1, MZ_HI - 0.1, p))
    add("outside", [20.0, 50.0, 100.0, 1500.2, 1600.0, 9000.0])     # every peak outside [min_mz, min_mz + n_bins * bin)
    add("one_bin", np.full(40, 500.02))                             # 40 peaks, one m/z bin: 40 ordered adds into one column
    for _ in range(36):
        add(None, rng.uniform(MZ_LO + 0.1, MZ_HI - 0.1, int(rng.integers(0, 13))))
    sizes = np.array([len(r) for r in rows])
    return dict(mz=np.concatenate(rows), intensity=rng.lognormal(0.0, 1.0, int(sizes.sum())).astype(f32),
                indptr=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), n_bins=n_bins, min_mz=start, row=names,
                short=np.flatnonzero(sizes <= 64), long=np.flatnonzero(sizes > 64))


def vec_patterns(lib):
    """16-row patterns (library rows) written at 16-aligned offsets: chunks start at multiples of the chunk size, so an
    aligned pattern meets a chunk boundary of every chunk size 2, 4, 8, 16 in the same place"""
    r = lib["row"]
    E, filler = r[0], [r[1], r[2], r[63], r["one_bin"], r["outside"]]
    fill = [filler[i % len(filler)] for i in range(16)]
    pats = [[E] * 16]                                              # sixteen empty rows
    for c in (2, 4, 8, 16):                                        # an empty row first and a 129-peak row last in a chunk
        p = list(fill)
        for b in range(0, 16, c):
            p[b], p[b + c - 1] = E, r[129]
        pats.append(p)
    pats.append([r[200], E, r[65], r[64]] * 4)                     # long -> empty -> long -> exactly one prefetch
    pats.append([r[64], r[200], E, r[65]] * 4)                     # the same, the hand-overs moved across the chunk-2/4 cuts
    pats.append([r[200], r[1]] * 8)                                # one peak after 200: `acc` has to be back to zero
    pats.append([r[2], r[200], r[1], r[0]] * 4)
    return pats


@functools.lru_cache(maxsize=None)
def vec_row_order(n, seed=5):
    """library row of each of the n output rows: a random fill (about 1 % rows above 64 peaks), the patterns at the first
    16-row blocks, in the middle and at the last whole blocks, and a fixed partial tail"""
    lib = vec_library()
    rng = np.random.default_rng(seed + n)
    order = rng.choice(lib["short"], n)
    is_long = rng.random(n) < 0.01
    order[is_long] = rng.choice(lib["long"], int(is_long.sum()))
    pats = vec_patterns(lib)
    blocks = n // 16
    assert blocks >= 3 * len(pats)
    for base in (0, blocks // 2, blocks - len(pats)):
        for j, p in enumerate(pats):
            order[16 * (base + j): 16 * (base + j + 1)] = p
    r = lib["row"]
    tail = [r[200], r[0], r[65], r[1], r[129]]
    order[n - len(tail):] = tail
    return order.astype(np.int64)


def vec_reference(low_dim, width, normalize):
    """the oracle's rows of the LIBRARY (float32); output row i of a case is row row_order[i] of it"""
    lib = vec_library()
    return fo.vectorize(lib["mz"], lib["intensity"], lib["indptr"], lib["min_mz"], BIN, lib["n_bins"], low_dim, norm=normalize,
                        width=width)


def f16_planes(X):
    """the hi / lo float16 planes of float32 rows (tests/test_gpu_search.py::_f16_planes): x ~= hi + lo / 2048"""
    hi = X.astype(np.float16)
    lo = ((X - hi.astype(f32)) * f32(2048)).astype(np.float16)
    return hi, lo


def vec_expected(ref, mode):
    """the library rows of every output of a mode, in the order `Context.vectorize` returns them"""
    h = ref.astype(np.float16)
    if mode == "f32":
        return (ref,)
    if mode == "f16":
        return (h,)
    if mode == "split16":
        return (np.ascontiguousarray(np.stack(f16_planes(ref), 1)),)
    if mode == "f32+f16":
        return ref, h
    assert mode == "f16+image"
    return h.astype(f32), h


# --------------------------------------------------------------------------------------------------------------- preprocess
DEFAULTS_RANK = OPTION_SETS[3]          # falcon's defaults with scaling="rank"
UNFILTERED = OPTION_SETS[4]             # nothing filtered, rank over every peak
PREP_OPTION_SETS = (DEFAULTS_RANK, UNFILTERED)
assert DEFAULTS_RANK["scaling"] == "rank" and DEFAULTS_RANK["max_peaks_used"] == 50 and UNFILTERED["mz_min"] is None


def prep_turns_n(cus):
    """three turns of the grid-stride loop (cus * 64 blocks of four one-spectrum waves), a last block with one live wave"""
    return 2 * (cus * 64 * 4) + 13


def _cat_spectra(parts):
    """[(mz, it, indptr, pmz, charge)] -> one batch"""
    ip = [np.zeros(1, np.int64)]
    for p in parts:
        ip.append(np.asarray(p[2][1:], np.int64) + ip[-1][-1])
    return (np.concatenate([np.asarray(p[0], f64) for p in parts]), np.concatenate([np.asarray(p[1], f32) for p in parts]),
            np.concatenate(ip), np.concatenate([np.asarray(p[3], f64) for p in parts]),
            np.concatenate([np.asarray(p[4], np.int32) for p in parts]))


def _spectrum(mz, it, pmz=600.0, charge=2):
    mz, it = np.asarray(mz, f64), np.asarray(it, f32)
    assert len(mz) == len(it) and np.all(np.diff(mz) >= 0)
    return mz, it, np.array([0, len(mz)], np.int64), np.array([pmz], f64), np.array([charge], np.int32)


@functools.lru_cache(maxsize=None)
def prep_library(seed=23):
    """about 1,500 raw spectra: random ones of up to 48 peaks, a handful of 70 / 130 / 300 peaks, empty ones, and ones every
    filter set's validity check rejects (one peak: no m/z span ... four peaks far apart: too few for the defaults)"""
    rng = np.random.default_rng(seed)
    parts = [raw_spectra(1280, seed, max_peaks=48)]
    for p in (70, 130, 300, 70, 130, 300):
        m = np.sort(np.round(rng.uniform(50, 1900, p), 4))
        m[0], m[-1] = min(m[0], 101.0), max(m[-1], 1500.0)
        it = np.round(rng.gamma(0.7, 1000.0, p), 0).astype(f32)    # quantised: ties at the top-50 cut
        parts.append(_spectrum(m, it, float(rng.uniform(300, 1200)), int(rng.integers(0, 5))))
    for _ in range(200):
        parts.append(_spectrum([], []))
    for _ in range(12):
        parts.append(_spectrum([300.0], [5.0]))
        parts.append(_spectrum([150.0, 400.0, 800.0, 1400.0], [1.0, 2.0, 3.0, 4.0], 500.0, 1))
    mz, it, ip, pmz, ch = _cat_spectra(parts)
    ch[rng.random(len(ch)) < 0.2] *= -1                            # negative-mode charges: |z| counts
    return mz, it, ip, pmz, ch


@functools.lru_cache(maxsize=None)
def prep_library_expected(which):
    """`fo.process_spectra` of the library under PREP_OPTION_SETS[which]"""
    out = fo.process_spectra(*prep_library(), **PREP_OPTION_SETS[which])
    frac = out[0].mean()
    assert 0.1 <= frac <= 0.9, f"{frac:.3f} of the library is valid: the gathered case would be one-sided"
    return out


def prep_gather(pick):
    """the raw batch whose spectrum i is library spectrum pick[i]"""
    mz, it, ip, pmz, ch = prep_library()
    nip, gmz, git = csr_gather(ip, pick, mz, it)
    return gmz, git, nip, pmz[pick], ch[pick]


def prep_gather_expected(which, pick):
    """the expected (valid, out_indptr, out_mz, out_intensity) of `prep_gather(pick)`, assembled from the library's"""
    valid, ip, omz, oit = prep_library_expected(which)
    nip, gmz, git = csr_gather(ip, pick, omz, oit)
    return valid[pick], nip, gmz, git


def prep_pick(n, seed=3):
    return np.random.default_rng(seed).integers(0, len(prep_library()[2]) - 1, n)


def precursor_targets(pmz, charge):
    """m/z of the precursor ion at every charge state z..1, by the kernel's own float64 formula (csrc/preprocess.hip)"""
    z = abs(int(charge)) if charge != 0 else 1
    neutral = (f64(pmz) - f64(fo.PROTON)) * f64(z)
    return [neutral / f64(c) + f64(fo.PROTON) for c in range(z, 0, -1)]


def _ulps(x):
    x = f64(x)
    return [np.nextafter(x, f64(-np.inf)), x, np.nextafter(x, f64(np.inf))]


def _opts(**kw):
    o = dict(min_peaks=1, min_mz_range=0.0, mz_min=None, mz_max=None, remove_precursor_tolerance=None, min_intensity=None,
             max_peaks_used=None, scaling="rank")
    o.update(kw)
    return o


def _tie_spectrum():
    """200 peaks; the value 50 is shared by positions 60..70 (across the lane-chunk cut at 64) and 125..131 (across 128);
    40 peaks are larger, the rest smaller"""
    it = 1.0 + 0.125 * np.arange(200)                              # < 50, distinct
    ties = np.r_[60:71, 125:132]
    others = np.setdiff1d(np.arange(200), ties)
    above = others[np.linspace(0, len(others) - 1, 40).astype(int)]   # 40 peaks above, in every lane chunk
    it[above] = 100.0 + above
    it[ties] = 50.0
    assert (it > 50).sum() == 40 and (it == 50).sum() == 18
    return _spectrum(100.0 + 5.0 * np.arange(200), it)


def prep_edge_cases():
    """-> [dict(name, batch=(mz, it, indptr, pmz, charge), opts, counts=[(lo, hi) per spectrum])]: `counts` bounds the peaks
    the ORACLE keeps per spectrum (0 = invalid); lo == hi where the construction fixes the outcome, a proper range where it
    depends on a rounding (`both outcomes occur`: lo and hi exclude all-kept and all-removed)"""
    cases = []

    def case(name, parts, counts, **opts):
        cases.append(dict(name=name, batch=_cat_spectra(parts), opts=_opts(**opts), counts=[c if isinstance(c, tuple) else (c, c)
                                                                                             for c in counts]))

    # ---- top-N ties across lane chunks: `need` is carried from chunk to chunk
    tie = _tie_spectrum()
    flat = _spectrum(100.0 + 5.0 * np.arange(200), np.full(200, 7.0))
    for keep in (1, 10, 11, 12, 17):                                # 1; the first run less one / whole / and one; all but one
        case(f"top{40 + keep}_ties", [tie], [40 + keep], max_peaks_used=40 + keep)
    for n_top in (63, 64, 65):
        case(f"top{n_top}_all_tied", [flat, tie], [n_top, n_top], max_peaks_used=n_top)
    # ---- m/z window: >= mz_min, <= mz_max
    lo, hi = _ulps(101.0), _ulps(1500.0)
    case("mz_window", [_spectrum([lo[0], lo[1], lo[2], 500.0, hi[0], hi[1], hi[2]], np.arange(1, 8)),
                       _spectrum([50.0, lo[0], hi[2], 1800.0], [1, 2, 3, 4])], [5, 0], mz_min=101.0, mz_max=1500.0)
    # ---- intensity >= min_intensity * base, the product in float32
    below4 = np.nextafter(f32(4.0), f32(0.0))
    thr = f32(f32(0.3) * f32(7.0))
    case("intensity_half_of_8", [_spectrum([200, 300, 400, 500, 600], [4.0, below4, 8.0, 3.0, 4.0])], [3], min_intensity=0.5)
    case("intensity_0.3_of_7", [_spectrum([200, 300, 400, 500], [thr, np.nextafter(thr, f32(0)), 7.0, np.nextafter(thr, f32(9))])],
         [3], min_intensity=0.3)
    # ---- precursor window |m - target| > tol at every charge state; a peak at target +- tol and one ulp to either side
    tol = 1.5
    parts, counts = [], []
    for pmz, ch in ((500.0, 1), (433.21, 2), (367.4567, 3), (433.21, -2), (611.3, 0)):
        probes = np.array([m for t in precursor_targets(pmz, ch) for edge in (t - f64(tol), t + f64(tol)) for m in _ulps(edge)])
        back = np.array([120.5, 130.5, 140.5, 1700.0, 1800.0])
        assert np.abs(back[:, None] - np.array(precursor_targets(pmz, ch))[None, :]).min() > 10
        m = np.sort(np.concatenate([probes, back]))
        parts.append(_spectrum(m, 1.0 + np.arange(len(m)) % 7, pmz, ch))
        counts.append((len(back) + 1, len(back) + len(probes) - 1))
    case("precursor_edges", parts, counts, remove_precursor_tolerance=tol)
    # ---- survivors exactly min_peaks / one fewer (one raw peak falls to the window first)
    five = [150.0, 300.0, 600.0, 900.0, 1200.0]
    case("min_peaks", [_spectrum(five, np.arange(1, 6)), _spectrum(five[:4], np.arange(1, 5)),
                       _spectrum([50.0] + five, np.arange(1, 7)), _spectrum([50.0] + five[1:], np.arange(1, 6))],
         [5, 0, 5, 0], min_peaks=5, mz_min=101.0)
    # ---- m/z span exactly min_mz_range / one ulp less
    below450 = np.nextafter(f64(450.0), f64(0.0))
    assert below450 - 200.0 < 250.0
    case("mz_span", [_spectrum([200.0, 300.0, 450.0], [1, 2, 3]), _spectrum([200.0, 300.0, below450], [1, 2, 3])], [3, 0],
         min_mz_range=250.0)
    # ---- the norm tree's 256-element passes and the rank loop: kept 255 .. 513 (three raw peaks fall to the window)
    rng = np.random.default_rng(77)
    parts, counts = [], []
    for kept in (255, 256, 257, 512, 513):
        m = np.concatenate([[60.0, 80.0], np.sort(np.round(rng.uniform(110, 1490, kept), 4)), [1700.0]])
        parts.append(_spectrum(m, np.round(rng.gamma(0.7, 50.0, kept + 3), 0)))
        counts.append(kept)
    for raw in (64, 65, 128):
        parts.append(_spectrum(np.sort(np.round(rng.uniform(110, 1490, raw), 4)), np.round(rng.gamma(0.7, 50.0, raw), 0)))
        counts.append(raw)
    case("norm_tree_sizes", parts, counts, mz_min=101.0, mz_max=1500.0)
    # ---- invalid, valid, empty, valid, invalid: out_indptr repeats
    g = lambda p: _spectrum(np.sort(np.round(rng.uniform(110, 1490, p), 4)), np.round(rng.gamma(0.7, 50.0, p), 1) + 1)
    case("indptr_repeats", [g(3), g(10), g(0), g(64), g(4)], [0, 10, 0, 64, 0], min_peaks=5)
    return cases


def check_edge_counts(case, oracle_out):
    """the case does what it was built for, by the oracle's output alone"""
    valid, ip = oracle_out[0], oracle_out[1]
    got = np.diff(ip)
    for i, (lo, hi) in enumerate(case["counts"]):
        assert lo <= got[i] <= hi, (case["name"], i, int(got[i]), (lo, hi))
        assert bool(valid[i]) == (got[i] > 0), (case["name"], i)


# -------------------------------------------------------------------------------------------------------------- flat kernels
def bin_values(cus, seed=9):
    """two turns and a bit of `to_vector_indices`' grid: float32 m/z below min_mz, inside the bins, above them"""
    n = 2 * cus * 8 * 256 + 77
    return np.random.default_rng(seed).uniform(20.0, 2100.0, n).astype(f32)


@functools.lru_cache(maxsize=None)
def rescore_case(cus, seed=41):
    """k = 64 neighbour slots per row, two turns and three rows of the rescore grid; about 4,000 slots are set, the rest empty.
    Rows map at random onto the spectra of `make_pairs(400, seed)` (pairs with a component above 32 peaks dropped, as
    test_gpu_exact_paths._kept drops them); a set slot of a row of spectrum s names a row of s's partner.  A call has one
    fragment tolerance: the slots are grouped by their pair's.
    -> dict(n, k, mz, intensity, indptr, order, turn, slots = {tol: (flat position i64[], neighbour row i32[], pair, side)})"""
    k, turn = 64, cus * 32 * 256
    n = 2 * (turn // k) + 3
    rng = np.random.default_rng(seed)
    cov = pc.Coverage()
    pairs = [p for p in pc.make_pairs(400, seed, "lognormal") if cov.add(pc.components(p[0], p[2], p[4]))]
    # the slot may sit in a row of either side: the transposed pair has to stay within the solver's bound, too
    pairs = [p for p in pairs if not pc.too_large(pc.components(p[2], p[0], p[4]))]
    assert len(pairs) >= 380
    mz, it, indptr = pc.to_csr(pairs)
    order = rng.integers(0, 2 * len(pairs), n).astype(np.int64)
    by_spectrum = [np.flatnonzero(order == s) for s in range(2 * len(pairs))]
    assert min(len(r) for r in by_spectrum) > 0
    flat = np.unique(np.concatenate([rng.integers(0, n * k, 4000), [turn - 1, turn, 2 * turn - 1, 2 * turn, (n - 1) * k + 5,
                                                                     n * k - 1]]))
    s = order[flat // k]
    nb = np.array([rng.choice(by_spectrum[x ^ 1]) for x in s], np.int32)
    tols = np.array([pairs[x // 2][4] for x in s])
    slots = {float(t): (flat[tols == t], nb[tols == t], (s // 2)[tols == t], (s % 2)[tols == t]) for t in pc.TOLS}
    assert all(len(v[0]) > 500 for v in slots.values())
    return dict(n=n, k=k, mz=mz, intensity=it, indptr=indptr, order=order, turn=turn, slots=slots, pairs=pairs)


def rescore_expected(case, tol, min_matches, _cache={}):
    """float32 (1 - sim) of the set slots of `tol`, `fo.cosine_fast` per distinct (pair, side)"""
    _, _, pair, side = case["slots"][tol]
    out = np.empty(len(pair), f32)
    for i, (p, sd) in enumerate(zip(pair.tolist(), side.tolist())):
        key = (id(case["pairs"]), p, sd)
        if key not in _cache:
            a_mz, a_it, b_mz, b_it, t = case["pairs"][p]
            assert t == tol
            _cache[key] = fo.cosine_fast(a_mz, a_it, b_mz, b_it, t) if sd == 0 else fo.cosine_fast(b_mz, b_it, a_mz, a_it, t)
        sim, nm = _cache[key]
        out[i] = f32(1.0 - (0.0 if nm < min_matches else sim))
    return out
