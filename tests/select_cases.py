"""Designed rows for the wavefront top-k select (csrc/select.h), their plain references and a model of the path each row
takes (test_select_cases_cpu.py, test_gpu_select.py).  Plain numpy: no torch, no GPU, no import of the library.

Flat buckets.  Every vector has ONE non-zero column, X[j, 0] = s[j] (low_dim 64), so query i sees the row s[i] * s[j]: a single
float32 product plus zeros -- exact in any summation order and on any form of the scan.  The expected value is
float32(float64(s[i]) * float64(s[j])) (the float64 product of two float32 values is exact: one rounding, as in the kernel),
ordered by (similarity descending, id ascending).  A zero product is +0.0 whatever the signs: the kernels' chains start from
+0.0 accumulators and (+0) + (-0) = +0.  Every product is normal in magnitude or exactly zero.

IVF buckets.  Rows are s[j] * e_c(j) on eight orthogonal axes (one list per axis after k-means), so a similarity is one exact
product or exactly 0: thousands of ties at 0 whose ids (through `perm`) are not monotonic in stream order.  The expected value
is `fo.ivf_search` on the exported index.

Memory order of the flat buckets (search.hip: flat jobs are laid out by decreasing size, stable): the `ascending` buckets stand
last among the buckets of their size in the index and carry values below 0.375 that GROW as the size shrinks, so in the sims
buffer row i + 1 of an ascending bucket is larger than row i everywhere and the row behind a bucket's last one is larger
still: row 0 of the ascending bucket one size down, or row 0 of the `descending` bucket that opens the next size (products of
0.37 and more).  The scan fills the padding of a row (columns nc .. round_up(nc, 32)) with the similarity of the LAST
candidate -- in an ascending row the largest.  An unmasked read past the end of such a row wins.

The two chunk load forms of select_rounds<., 16> (`wide`: one 16-byte load per lane, key i of a lane is chunk position
4 lane + i; otherwise four 4-byte loads, position 64 i + lane).  `wide` needs row + 4 * 1024 bytes on a 16-byte boundary:
 * MODE_DENSE, staged (select_kernel): a row starts at obase + q * round_up(nc, 32) floats, obase a multiple of 1,024 floats
   of a 256-byte aligned buffer: ALWAYS wide.  The narrow form cannot occur; no case is invented for it.
 * MODE_DENSE / MODE_IVF in the fallback kernels (fused.hip): scratch rows at a stride of round_up(max, 64) + 2,048 floats:
   ALWAYS wide.
 * MODE_IVF, staged: a row starts at q_sim_off[slot], the exclusive prefix sum of the candidate totals of the queries in list
   order (32-query tiles, empty slots count 0): wide when that sum is a multiple of 4, narrow otherwise.  Both forms occur
   and both are witnessed (`ivf_rows`)."""
import functools

import numpy as np

f32, f64 = np.float32, np.float64

D = 64                                            # low_dim of every case
K_VALUES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)
K_MAX = 256                                       # FAL_MAX_K_ANN; a top-k for k < K_MAX is a prefix of the top-K_MAX
ASC_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 767, 768, 769,
             1023, 1024, 1025, 1027, 1028, 1279, 1280, 1281, 1537, 2305)
OTHER_SIZES = (129, 1025, 1281, 2305)
EDGE_SIZES = (128, 256, 257, 512, 513)            # + the cuts of the fallback kernels' ladder, for `all_equal`
SCAN_CUTS = (128, 256, 384, 512, 768, 1024)       # select_kernel: R = 2, 4, 6, 8, 12, 16
FALLBACK_CUTS = (128, 256, 512)                   # fused_fallback_kernel / ivf_fallback_kernel: R = 2, 4, 8, 16
FIRST = 1024                                      # keys of the first round of a streamed row
CHUNK = 256                                       # keys per streamed chunk
SEL_BUF = K_MAX + CHUNK                           # kSelBuf
LOW_BITS_BASE = 0x3F000000                        # 0.5: the low 9 bits are free
LOW_BITS_M = (2, 5, 256, 257, 300)
TIE_H = (1, 60, 100, 200)                         # keys of the higher value in a `tie_at_k` row
FALLBACK_PATTERNS = ("all_equal", "tie_at_k")     # sent through the prefilter path: they funnel into the exact fallback


# --------------------------------------------------------------------------- flat patterns
def _ramp(n, lo):
    """n strictly increasing float32 values in [lo, 1.5 lo)"""
    return (lo * (1.0 + (np.arange(n) + 0.5) / (2.0 * n))).astype(f32)


def ascending(n, rank):
    """rank = position of the size in descending order: values in [2^(rank-31), 1.5 * 2^(rank-31))"""
    return _ramp(n, 2.0 ** (rank - 31))


def descending(n):
    return _ramp(n, 0.5)[::-1].copy()


def all_equal(n):
    return np.full(n, 0.75, f32)


def tie_at_k(n, h):
    """h keys of 0.75 spread over the whole row (first round and streamed part), the rest 0.5: for k > h the k-th best lies in
    the run of the lower value, which covers every register of the first round and every chunk"""
    h = min(h, n // 2)
    s = np.full(n, 0.5, f32)
    s[(np.arange(h) * n) // h + (n // h) // 2] = 0.75
    return s


def low_bits(n, m):
    return (np.uint32(LOW_BITS_BASE) + (np.arange(n) % m).astype(np.uint32)).view(f32)


def mixed_sign(n):
    p = min(100, n // 3)                           # p positive, p zero, the rest negative, in shuffled positions
    cat = np.full(n, -1)
    cat[:p] = 1
    cat[p:2 * p] = 0
    cat = np.random.default_rng(n).permutation(cat)
    s = np.zeros(n, f32)
    s[cat > 0] = _ramp(p, 0.5)
    s[cat < 0] = -_ramp(n - 2 * p, 0.5)
    return s


_EXACT_RUNS = (1, 1, 61, 1, 1, 62, 1, 1, 126, 1)   # bins 255, 254, ...: cumulative 1, 2, 63, 64, 65, 127, 128, 129, 255, 256


def exact_bin(n, miss):
    """Keys 0x3F000000 | bin << 15 | rank: the keys differ in bits 0 .. 22, so the first radix level reads bits 15 .. 22 = bin.
    The best keys fill the bins from 255 down in runs whose cumulative sizes are the k values: for every k the bin of the k-th
    best holds exactly the keys still wanted (early exit at the first level).  `miss`: bin 255 holds one key more, so every
    cumulative size is k + 1 and the search descends (the bin holds one key too many).  Eight rows are exactly 0.5, so their
    query rows are the designed keys with the exponent lowered by one; the best keys stand among the first 1,024 positions."""
    runs = list(_EXACT_RUNS)
    runs[0] += 1 if miss else 0
    bins = np.concatenate([np.full(r, 255 - i) for i, r in enumerate(runs)])
    rest = n - len(bins)
    if rest > 0:
        bins = np.concatenate([bins, 200 - (np.arange(rest) % 150)])
    bins = bins[:n]
    key = np.uint32(LOW_BITS_BASE) | (bins.astype(np.uint32) << np.uint32(15)) | np.arange(n, dtype=np.uint32)
    key[n - 8:] = LOW_BITS_BASE
    rng = np.random.default_rng(7 * n + miss)
    head = min(n, FIRST)
    pos = np.concatenate([rng.permutation(head), head + rng.permutation(n - head)])
    s = np.empty(n, np.uint32)
    s[pos] = key
    return s.view(f32)


class FlatCase:
    def __init__(self, pattern, name, s):
        self.pattern, self.name, self.s, self.n = pattern, name, np.ascontiguousarray(s, f32), len(s)
        self.row0 = 0                              # first row of the bucket in the index (set by flat_cases)

    def __repr__(self):
        return f"{self.name}[{self.n}]"


def _spread(variants, make):
    """every variant at 1,281 rows; the other sizes of OTHER_SIZES dealt to the variants in turn"""
    out = [(v, 1281) for v in variants]
    out += [(variants[i % len(variants)], n) for i, n in enumerate(x for x in OTHER_SIZES if x != 1281)]
    return [make(v, n) for v, n in out]


@functools.lru_cache(maxsize=None)
def flat_cases():
    """-> the flat buckets in index order: the other patterns first, then `ascending` by decreasing size"""
    cases = [FlatCase("descending", "descending", descending(n)) for n in OTHER_SIZES]
    cases += [FlatCase("all_equal", "all_equal", all_equal(n)) for n in OTHER_SIZES + EDGE_SIZES]
    cases += _spread(TIE_H, lambda h, n: FlatCase("tie_at_k", f"tie_at_k/{h}", tie_at_k(n, h)))
    cases += _spread(LOW_BITS_M, lambda m, n: FlatCase("low_bits", f"low_bits/{m}", low_bits(n, m)))
    cases += [FlatCase("mixed_sign", "mixed_sign", mixed_sign(n)) for n in OTHER_SIZES]
    cases += _spread((0, 1), lambda miss, n: FlatCase("exact_bin", "exact_bin/miss" if miss else "exact_bin/hit", exact_bin(n, miss)))
    sizes = sorted(ASC_SIZES, reverse=True)
    cases += [FlatCase("ascending", "ascending", ascending(n, r)) for r, n in enumerate(sizes)]
    row0 = 0
    for c in cases:
        c.row0 = row0
        row0 += c.n
    return tuple(cases)


def vectors(cases):
    """-> X float32 [n, D] (column 0 = s), bucket offsets int64"""
    off = np.concatenate([[0], np.cumsum([c.n for c in cases])]).astype(np.int64)
    X = np.zeros((int(off[-1]), D), f32)
    X[:, 0] = np.concatenate([c.s for c in cases])
    return X, off


def products(s):
    """the similarity matrix of a flat bucket: one rounding of the exact product; zero products are +0.0"""
    s64 = np.asarray(s, f32).astype(f64)
    S = (s64[:, None] * s64[None, :]).astype(f32) + f32(0)
    mag = np.abs(S)
    assert ((mag == 0) | (mag >= f32(2.0 ** -126))).all(), "a product is denormal"
    return S


def plain_topk(S, k, base=0):
    """rows of S -> the k best by (similarity descending, column ascending): sim f32 [n, k] (pad -inf), idx i32 (pad -1)"""
    n, m = S.shape
    ids = np.broadcast_to(np.arange(m), S.shape)
    order = np.lexsort((ids, -S), axis=1)[:, :k]
    sim = np.full((n, k), -np.inf, f32)
    idx = np.full((n, k), -1, np.int32)
    sim[:, :order.shape[1]] = np.take_along_axis(S, order, 1)
    idx[:, :order.shape[1]] = order + base
    return sim, idx


def flat_reference(cases, k=K_MAX):
    """-> sim [n, k], idx [n, k] over all rows of the index made of `cases`"""
    parts = [plain_topk(products(c.s), k, c.row0) for c in cases]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# --------------------------------------------------------------------------- survivor counts of the fused filter
SURVIVORS = (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256)
SURVIVOR_QUERIES = 8
SURVIVOR_KEEPS = tuple(sorted({x for c in SURVIVORS for x in (1, c - 1, c, c + 1, 256) if 1 <= x <= K_MAX}))


@functools.lru_cache(maxsize=None)
def survivor_cases(with_rt):
    """One bucket of 256 + 8 rows per survivor count c, for k_ann = 256.  256 rows carry large values (in pairs: ties in
    similarity) and are every row's top 256; 8 rows carry small ones and are never selected.  Rows are sorted by precursor
    m/z in three groups 0.3 Da apart; the middle group holds the 8 small rows (the queries the count is designed for) and c of
    the large ones, so exactly c of a query's 256 candidates pass a tolerance of 0.05 Da (or 20 ppm).  `with_rt`: the middle
    group holds up to 5 more large rows whose retention time is out of tolerance.
    -> cases, mz f32 [n], rt f32 [n] or None, queries: list of (c, rows)"""
    rng = np.random.default_rng(11)
    cases, mz, rt, queries = [], [], [], []
    row0 = 0
    for b, c in enumerate(SURVIVORS):
        extra = min(5, 256 - c) if with_rt else 0
        n_low = (256 - c - extra) // 2
        n_high = 256 - c - extra - n_low
        mid = rng.permutation(np.concatenate([np.zeros(SURVIVOR_QUERIES, int), np.ones(c, int), np.full(extra, 2)]))
        big = 0.3 + 0.7 * (rng.permutation(256) // 2 + 1) / 128.0          # spread out: few approximate values per histogram
        small = 0.2 * (1.0 + np.arange(SURVIVOR_QUERIES) / 16.0)            # bin of the prefilter, so most rows stay on chip
        n = 256 + SURVIVOR_QUERIES
        s = np.empty(n, f64)
        is_q = np.zeros(n, bool)
        is_q[n_low + np.flatnonzero(mid == 0)] = True
        s[is_q] = small
        s[~is_q] = big
        c_ = FlatCase("survivors", f"survivors/{c}", s)
        c_.row0 = row0
        cases.append(c_)
        m0 = 400.0 + 2.0 * b
        mz.append(np.concatenate([np.full(n_low, m0), np.full(len(mid), m0 + 0.3), np.full(n_high, m0 + 0.6)]))
        r = 100.0 + rng.integers(-5, 6, n).astype(f64)
        r[n_low + np.flatnonzero(mid == 2)] = 500.0
        rt.append(r)
        queries.append((c, row0 + np.flatnonzero(is_q)))
        row0 += n
    return (tuple(cases), np.concatenate(mz).astype(f32), np.concatenate(rt).astype(f32) if with_rt else None, queries)


def window_mz(n, step=1e-3):
    """sorted precursor m/z for a whole index: with 0.05 Da about 50 rows on either side pass"""
    return (500.0 + step * np.arange(n)).astype(f32)


# --------------------------------------------------------------------------- IVF buckets
IVF_LISTS = ((127, 128, 129, 256, 257, 384, 385, 512), (513, 768, 769, 1024, 1025, 255, 1, 300),
             (20, 30, 40, 60, 100, 150, 200, 400))      # rows per list; the last bucket: few candidates, for the fallback's R = 2, 4
IVF_ZERO_ROWS = 3                                 # all-zero rows per bucket: they join list 0 (counted in its size above)
IVF_PROBES = (1, 3, 16)                           # below n_list twice, and at or above it
IVF_PREFILTER_PROBES = (1, 3)                     # with the float16 list scan (at most 4,096 candidates per query)
IVF_FALLBACK_K = (64, 128)                        # k_ann of the prefiltered IVF search
IVF_KMEANS_ITERS = 3


@functools.lru_cache(maxsize=None)
def ivf_vectors():
    """-> X [n, D], bucket offsets, n_list (8 per bucket).  Row j of a bucket lies on axis c(j) (column c) with a value from
    {0.5 + t / 256}: duplicates, so ties among the positive similarities too.  The axes are shuffled over the rows; the rows
    k-means starts from (floor(i n / 8)) are put on axis i, so list i = axis i (+ the zero rows in list 0)."""
    Xs, sizes = [], []
    for b, lists in enumerate(IVF_LISTS):
        rng = np.random.default_rng(100 + b)
        pops = list(lists)
        pops[0] -= IVF_ZERO_ROWS
        axis = np.concatenate([np.full(p, a) for a, p in enumerate(pops)] + [np.full(IVF_ZERO_ROWS, -1)])
        axis = rng.permutation(axis)
        n = len(axis)
        for a in range(len(pops)):                # seed rows: one per axis, non-zero
            want = (a * n) // len(pops)
            have = int(np.flatnonzero(axis == a)[-1])
            axis[want], axis[have] = axis[have], axis[want]
        seeds = (np.arange(len(pops)) * n) // len(pops)
        assert np.array_equal(axis[seeds], np.arange(len(pops)))
        val = (0.5 + rng.integers(0, 97, n) / 256.0).astype(f32)
        X = np.zeros((n, D), f32)
        nz = axis >= 0
        X[np.flatnonzero(nz), axis[nz]] = val[nz]
        Xs.append(X)
        sizes.append(n)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(Xs), off, np.full(len(sizes), len(IVF_LISTS[0]), np.int32)


def ivf_streams(Xb, perm, loff, probes):
    """per query of one bucket, in row order: the stream of its candidates as the select sees it (probe order, list order inside)
    -> list of (sims f32, ids i64) with bucket-local ids"""
    out = []
    col = np.abs(Xb).argmax(1)
    val = Xb[np.arange(len(Xb)), col].astype(f64)
    for i in range(len(Xb)):
        cand = np.concatenate([perm[loff[l]:loff[l + 1]] for l in probes[i] if l >= 0]).astype(np.int64)
        s = (np.where(col[cand] == col[i], val[cand] * val[i], 0.0)).astype(f32) + f32(0)
        out.append((s, cand))
    return out


def ivf_rows(nc_in_list_order):
    """candidate totals of the queries of the IVF buckets, bucket after bucket in list order (32-query tiles, the empty slots of
    a bucket's last tile count 0) -> per query: True when its sims row takes the 16-byte chunk load (staged MODE_IVF)"""
    wide, base = [], 0
    for nc in nc_in_list_order:
        start = base + np.concatenate([[0], np.cumsum(nc)[:-1]])
        wide.append(start % 4 == 0)
        base += int(np.sum(nc))
    return wide


# --------------------------------------------------------------------------- the model of select.h (a witness, never a reference)
def sortable(x):
    """f32_sortable, with the kernel's floor of 1 (0 marks an empty slot)"""
    b = np.ascontiguousarray(x, f32).view(np.uint32)
    u = np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.maximum(u, np.uint32(1))


def r_class(nc, cuts):
    for r, cut in zip((2, 4, 6, 8, 12) if len(cuts) == 6 else (2, 4, 8), cuts):
        if nc <= cut:
            return r
    return 16


def radix_search(u, k):
    """select_round's threshold search over the first-round keys u (uint32, all non-zero), m = len(u) > k.
    -> dict: shift, levels (bits per level), exit ('exact' | 'ids'), T, first_miss (keys in the first level's deciding bin
    beyond the wanted ones; None when all keys are equal)"""
    u = u.astype(np.uint64)
    mn, mx = int(u.min()), int(u.max())
    shift = (mn ^ mx).bit_length()
    first_shift = shift
    prefix = 0 if shift >= 32 else (mx >> shift) << shift
    kk, eq, exact, levels, first_miss = k, len(u), False, [], None
    while shift > 0 and not exact:
        wbits = min(8, shift)
        hi = shift
        shift -= wbits
        himask = 0 if hi >= 32 else (0xFFFFFFFF << hi) & 0xFFFFFFFF
        sel = u[(u & np.uint64(himask)) == np.uint64(prefix)]
        hist = np.bincount(((sel >> np.uint64(shift)) & np.uint64((1 << wbits) - 1)).astype(np.int64), minlength=1 << wbits)
        above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])      # keys in higher bins
        b = int(np.flatnonzero(above + hist >= kk)[-1])
        kk -= int(above[b])
        prefix |= b << shift
        eq = int(hist[b])
        exact = eq == kk
        levels.append(wbits)
        if first_miss is None:
            first_miss = eq - kk
    return {"shift": first_shift, "levels": tuple(levels), "exit": "exact" if exact else "ids", "T": prefix,
            "first_miss": first_miss}


def trace(sims, k, dense, cuts=SCAN_CUTS):
    """The path of one row of similarities (stream order) through select_rounds -> dict
      R, fresh, search (radix_search's dict, or None when the first round holds at most k keys),
      chunks, tail (keys of the last chunk), reselects, reselect_at (chunk numbers, from 1), reselect_ids (how many of them
      went to the id search), equal_streamed (streamed keys equal to the threshold in force: dropped when dense, kept when not).
    Between reselects the threshold is the stale one: the k-th best of the last cut."""
    u = sortable(sims)
    nc = len(u)
    R = r_class(nc, cuts)
    fresh = min(nc, 64 * R)
    out = {"R": R, "nc": nc, "fresh": fresh, "search": None, "chunks": 0, "tail": 0, "reselects": 0, "reselect_at": (),
           "reselect_ids": 0, "equal_streamed": 0}
    head = u[:fresh]
    if fresh > k:
        out["search"] = radix_search(head, k)
    kept = np.sort(head)[::-1][:k]                   # the key multiset of the set (ties by id do not change it)
    if R < 16 or nc <= FIRST:
        return out
    T = int(kept.min())                              # carry == k here: k <= 256 < 1,024
    at = []
    n_chunks = -(-(nc - FIRST) // CHUNK)
    for ci in range(n_chunks):
        chunk = u[FIRST + ci * CHUNK: FIRST + (ci + 1) * CHUNK]
        out["equal_streamed"] += int((chunk == T).sum())
        inn = chunk[chunk > T] if dense else chunk[chunk >= T]
        kept = np.concatenate([kept, inn])
        if len(kept) > SEL_BUF - CHUNK or ci == n_chunks - 1:
            if len(kept) > k:
                kept = np.sort(kept)[::-1]
                T = int(kept[k - 1])
                # reselect's bitwise search ends early when a threshold splits off exactly k keys; it goes on to the id search
                # when more keys than wanted equal the k-th best
                out["reselect_ids"] += int((kept >= T).sum() > k)
                kept = kept[:k]
                at.append(ci + 1)
    out.update(chunks=n_chunks, tail=len(chunk), reselects=len(at), reselect_at=tuple(at))
    return out


def witness_rows(case):
    """the rows of a flat bucket the model is run on: first, second, middle, last, and the rows whose value is a power of two
    (their similarity rows are the designed values with another exponent)"""
    n = case.n
    rows = {0, min(1, n - 1), n // 2, n - 1}
    m, _ = np.frexp(case.s)
    rows |= set(np.flatnonzero(m == 0.5)[:2].tolist())
    rows |= set(np.flatnonzero(case.s < 0)[:1].tolist()) | set(np.flatnonzero(case.s == 0)[:1].tolist())
    return sorted(rows)
