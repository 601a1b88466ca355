"""Designed rows for the float16 prefilters (fused.hip, ivf16.hip / list16*.hip, assign16.hip, coarse16.hip, scan16.hip), their
plain references and a model of what the prefilters see (test_prefilter_cases_cpu.py, test_gpu_prefilter.py).  Plain numpy: no
torch, no GPU, no import of the library.

The prefilters rest on |approx - exact| <= 1.3e-3 v + 2e-6 (+ 1.2e-5 once the value is a 16-bit key) and re-evaluate exactly
every decision closer than that.  Random rows put the error at 0.68 of the bound and never at a decision; here it is put at its
maximum, at the decision.

Values.  u = 2^-11 is half a float16 ulp relative to a power of two.  `down(e, k)` is the largest float32 below the float16
rounding midpoint 2^e (1 + (2 k + 1) u): float16 takes away almost u.  `up(e, k)` is the smallest float32 above it: float16
adds almost u.  Candidate rows have ONE non-zero column, query rows two, so a query-candidate similarity is one product:
    exact  = float32(float64(a) * float64(b))      (one rounding, as in the kernels' fmaf chain; the other term adds +0)
    approx = float64(float16(a)) * float64(float16(b))      (exact in float32; the matrix core adds zeros to it)
A `down` query component times a `down` candidate on column 0 is UNDER-estimated by 2 u, an `up` component times an `up`
candidate on column 1 OVER-estimated by 2 u: exact values within 4 u = 1.95e-3 of each other come out in the opposite order.

Keys.  The list scans convert by v_cvt_pknorm_u16_f32, assign16 by __float2uint_rn(x * 65535.f); neither can be observed from
Python, so the modelled key is trusted to +-1 unit and every design keeps 2 units of slack around the boundary it aims at.

The model is a witness (does the design reach what it aims at?), never a reference: the references are `plain_topk` over the
closed-form exact similarities and the oracle's index / search functions."""
import functools

import numpy as np

from tests.select_cases import plain_topk          # (similarity descending, id ascending)

f16, f32, f64 = np.float16, np.float32, np.float64

D = 64
U = 2.0 ** -11
REL, ABS, ABS_KEY = 1.3e-3, 2e-6, 1.2e-5          # the bound the kernels rely on
FUSED_MEM_HALF = 20                               # FAL_FUSED_MEM / 2: members per (query, lane half) of approx_kernel
IVF_MEM = 40                                      # FAL_FUSED_MEM: members per query of select16
COARSE_MEM = 16                                   # members a query of coarse16w_kernel holds before it is handed over
TOL_DA = 0.05                                     # precursor tolerance of every search here (Da)


# --------------------------------------------------------------------------- value primitives
def mid(e, k=0):
    """the float16 rounding midpoint 2^e (1 + (2 k + 1) u): exact in float32"""
    return f32(2.0 ** e * (1.0 + (2 * k + 1) * U))


def down(e, k=0):
    return np.nextafter(mid(e, k), f32(0))


def up(e, k=0):
    return np.nextafter(mid(e, k), f32(np.inf))


def h16(x):
    """float16 rounding (round to nearest even, subnormals kept) as float64"""
    return np.asarray(x, f32).astype(f16).astype(f64)


def largest_rounding_to(t):
    """the largest float32 that float16 rounds to the float16 value t (t > 0, normal)"""
    t = f16(t)
    nxt = np.nextafter(t, f16(np.inf))
    return np.nextafter(f32((f64(t) + f64(nxt)) / 2), f32(0))


def smallest_rounding_to(t):
    t = f16(t)
    prv = np.nextafter(t, f16(0))
    return np.nextafter(f32((f64(t) + f64(prv)) / 2), f32(np.inf))


EXACT16 = (f32(0.75), f32(0.5), f32(0.3125), f32(2.0 ** -9 * 1.5))
SUBNORMAL = (f32(2.0 ** -15), f32(2.0 ** -15 * 1.25), f32(2.0 ** -20 * 1.5), f32(2.0 ** -24), f32(2.0 ** -24 * 1.75),
             np.nextafter(f32(2.0 ** -25), f32(1)))                       # float16 keeps them (as multiples of 2^-24)
FLUSHED = (f32(2.0 ** -25), f32(2.0 ** -26 * 1.5), f32(2.0 ** -30))       # at or below half the smallest subnormal: float16 zero


# --------------------------------------------------------------------------- similarities in closed form
def exact_sims(A, B=None):
    """the kernels' k-ordered fmaf chain (column k, then column d / 2 + k) over the columns that hold a non-zero; a zero
    product leaves the accumulator as it is.  float64 emulation:
    exact while product and accumulator span at most 53 bits -- single products always, two-term sums for components in
    [0.25, 0.71] (test_prefilter_cases_cpu.py checks it against the oracle's compiled chain)"""
    B = A if B is None else B
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    acc = np.zeros((len(A), len(B)), f32)
    dh = A.shape[1] // 2
    for c in sorted(np.flatnonzero(A.any(0) & B.any(0)), key=lambda c: (c % dh, c // dh)):
        acc = (A[:, c, None].astype(f64) * B[None, :, c].astype(f64) + acc.astype(f64)).astype(f32)
    mag = np.abs(acc)
    assert ((mag == 0) | (mag >= f32(2.0 ** -126))).all(), "a similarity is a float32 denormal"
    return acc + f32(0)


def approx_sims(A, B=None):
    """float16 factors, exact products -> float64 [n, m], and `single`: the pairs that share at most one non-zero column
    (there the value is what the f16 matrix cores return, bit for bit; elsewhere it is within a float32 rounding of it)"""
    B = A if B is None else B
    A16, B16 = h16(A), h16(B)
    shared = (np.asarray(A) != 0).astype(np.int32) @ (np.asarray(B) != 0).astype(np.int32).T
    return A16 @ B16.T, shared <= 1


def bound_ratio(approx, exact, keyed=False):
    """|approx - exact| / bound; keyed: approx is key / 65535"""
    approx, exact = np.asarray(approx, f64), np.asarray(exact, f64)
    return np.abs(approx - exact) / (REL * approx + (ABS_KEY if keyed else ABS))


def key_of(v):
    """round(clamp(v, 0, 1) * 65535): the list scans' key (trusted to +-1)"""
    return np.rint(np.clip(np.asarray(v, f64), 0.0, 1.0) * 65535.0).astype(np.int64)


def key_delta(T, rel=REL):
    """ivf16.hip / coarse16.hip: (delta, delta_e) around the key T, in the kernels' float32 arithmetic"""
    Tv = f32(T) * f32(1.0 / 65535.0)
    e = f32(f32(rel) * Tv + f32(ABS_KEY))
    de = int(np.ceil(f32(e * f32(65535.0)))) + 1
    return 2 * de + 2, de


# fused.hip's histogram bins: 128 of 1/512 below 0.25, 32 of 3/128 above
def bin_of(v):
    v = f32(v)
    lo = int(f32(v * f32(512)))
    hi = min(159, 128 + int(f32(max(f32(v - f32(0.25)), f32(0)) * f32(128.0 / 3.0))))
    return lo if v < 0.25 else hi


def bin_lo(b):
    return f32(b) * f32(1.0 / 512) if b < 128 else f32(0.25) + f32(b - 128) * f32(3.0 / 128)


def bin_hi(b):
    return f32(b + 1) * f32(1.0 / 512) if b < 128 else (f32(1.0625) if b == 159 else f32(0.25) + f32(b - 127) * f32(3.0 / 128))


def fused_window(b, rel=REL):
    """the widened threshold bin of approx_kernel: members are the approximate values in [lo - m, hi + m]"""
    e0 = f32(f32(rel) * bin_hi(b) + f32(ABS))
    m = f32(f32(2.5) * e0)
    return f32(bin_lo(b) - m), (f32(np.inf) if b == 159 else f32(bin_hi(b) + m))


def fused_members(approx_row, k, pos, rel=REL):
    """approx_kernel on one query: approximate similarities of its candidates (bucket order; pos = their bucket-local index)
    -> (b*, members in lane half 0, members in half 1, T~, the smallest distance of a value from an edge of the widened bin,
    the bin of every value); the half of a candidate is bit 2 of its index"""
    v = np.maximum(np.asarray(approx_row, f64).astype(f32), f32(0))
    bins = np.array([bin_of(x) for x in v])
    order = np.sort(v)[::-1]
    bstar = bin_of(order[k - 1])
    lo, hi = fused_window(bstar, rel)
    mem = (v >= lo) & (v <= hi)
    half = (np.asarray(pos) >> 2) & 1
    return bstar, int((mem & (half == 0)).sum()), int((mem & (half == 1)).sum()), float(order[k - 1]), \
        float(min(np.abs(v.astype(f64) - f64(lo)).min(), np.abs(v.astype(f64) - f64(hi)).min())), bins


# --------------------------------------------------------------------------- bound: rows for the f16 flat scan
BOUND_EXPONENTS = tuple(range(-1, -8, -1))


@functools.lru_cache(maxsize=None)
def bound_rows(d):
    """One flat bucket at low_dim d, every row with ONE non-zero (column 0 for `down` values, column 1 for `up`, so that
    down . up = 0).  The similarity of two rows is one product: down . down is under-estimated by 2 u, up . up over-estimated.
    + float16-exact values and values in / below float16's subnormal range on both columns.  -> X, names"""
    vals = [(0, down(e), f"down{e}") for e in BOUND_EXPONENTS] + [(1, up(e), f"up{e}") for e in BOUND_EXPONENTS]
    vals += [(c, v, "exact16") for c in (0, 1) for v in EXACT16]
    vals += [(c, v, "sub") for c in (0, 1) for v in SUBNORMAL]
    vals += [(c, v, "flushed") for c in (0, 1) for v in FLUSHED]
    # enough further rows that every row sees more candidates than the k it is searched with
    vals += [(j % 2, f32(0.25 + (j // 2) / 256.0), "fill") for j in range(64)]
    X = np.zeros((len(vals), d), f32)
    for i, (c, v, _) in enumerate(vals):
        X[i, c] = v
    return X, tuple(n for _, _, n in vals)


# --------------------------------------------------------------------------- flat buckets: inversion
FLAT_INV_EXPONENTS = (-1, -2, -3)                 # exponent of the candidates; the queries stay at 2^-1
FLAT_INV_H, FLAT_INV_Q, FLAT_INV_PAIR, FLAT_INV_LOW = 29, 4, 3, 40
FLAT_INV_K = FLAT_INV_H + FLAT_INV_Q + 2          # the k_ann-th place: the second of the three X rows


def flat_inversion(ec):
    """A bucket whose queries Q = (down(-1), up(-1)) see, below H high column-0 rows and each other, three copies of
    X = down(ec, 1) on column 0 and three of Y = up(ec, 0) on column 1:
        exact  X ~ 2^(ec-1) (1 + 4 u)  >  Y ~ 2^(ec-1) (1 + 2 u)        approx  X ~ (1 + 2 u)  <  Y ~ (1 + 4 u)
    With k_ann = H + Q + 2 the exact top-k holds the two X rows of lowest id and no Y; the approximate one two Y and no X.
    The Q, X and Y rows share one precursor m/z (the window of a query holds exactly them), interleaved so that ids do not
    follow similarity.  -> X [n, D], mz [n], designed query rows, x rows, y rows"""
    s = 2.0 ** (ec + 1)
    rows, mz = [], []
    for j in range(FLAT_INV_H):                                               # high rows, float16-exact
        rows.append((0, f32(s * (0.5625 + j / 128.0)), None))
        mz.append(500.0)
    q, xs, ys = [], [], []
    for j in range(FLAT_INV_PAIR):
        ys.append(len(rows)); rows.append((1, up(ec, 0), None)); mz.append(500.3)
        q.append(len(rows)); rows.append((0, down(-1, 0), up(-1, 0))); mz.append(500.3)
        xs.append(len(rows)); rows.append((0, down(ec, 1), None)); mz.append(500.3)
    for j in range(FLAT_INV_Q - FLAT_INV_PAIR):
        q.append(len(rows)); rows.append((0, down(-1, 0), up(-1, 0))); mz.append(500.3)
    for j in range(FLAT_INV_LOW):                                             # low rows on both columns
        rows.append((j % 2, f32(s * (0.25 + (j // 2) / 256.0)), None))
        mz.append(500.6 + 0.2 * j)
    X = np.zeros((len(rows), D), f32)
    for i, (c, v, v1) in enumerate(rows):
        X[i, c] = v
        if v1 is not None:
            X[i, 1] = v1
    return X, np.asarray(mz, f32), np.asarray(q), np.asarray(xs), np.asarray(ys)


# --------------------------------------------------------------------------- flat buckets: collapse and edge (fused.hip)
FLAT_RUNS = ((19, 0), (20, 0), (21, 0), (20, 1), (21, 1))                   # (run length, lane half)
FLAT_COL_HIGH, FLAT_COL_LOW = 24, 60
FLAT_EDGE_MARGIN = 2e-6                           # distance an edge candidate keeps from the window's edge


def _lattice_in(q16, lo, hi):
    """float16 values c (in [0.25, 1)) whose product with q16 lies in [lo, hi] -> sorted float64 array"""
    cand = np.concatenate([np.arange(1024, 2048, dtype=f64) * 2.0 ** -12,     # [0.25, 0.5): ulp 2^-12
                           np.arange(1024, 2048, dtype=f64) * 2.0 ** -11])    # [0.5, 1): ulp 2^-11
    p = cand * q16
    return cand[(p >= lo) & (p <= hi)]


@functools.lru_cache(maxsize=None)
def flat_collapse(run, half, edge):
    """A bucket of column-0 rows only: similarity(i, j) = a_i a_j, one product for EVERY pair, and every row sees the same
    order of candidates.  FLAT_COL_HIGH rows in [0.66, 0.95], `run` rows 0.5 (1 + t u) with distinct 0 < t < 1 -- distinct exact
    values, ONE float16 value -- and low rows in [0.35, 0.4]; k_ann ends inside the run.  The run's rows stand at bucket
    positions of lane half `half` (bit 2 of the position), so run = FUSED_MEM_HALF + 1 overflows approx_kernel's member list of
    that half for every query and run = FUSED_MEM_HALF fills it.
    edge: None, or 'in' / 'out': with run = FUSED_MEM_HALF, one more candidate in the same half whose approximate value, for
    the queries of value 0.5 (the run rows themselves see it too), lies just inside / just outside the upper edge of the widened
    threshold bin -- inside it overflows the list, outside it does not.
    -> X [n, D], mz [n], k_ann, run rows, edge value or None"""
    hi_vals = [f32(0.66 + 0.29 * j / (FLAT_COL_HIGH - 1)) for j in range(FLAT_COL_HIGH)]
    run_vals = [f32(0.5 * (1.0 + (j + 1.0) / (run + 2.0) * U)) for j in range(run)]
    lo_vals = [f32(0.35 + 0.05 * j / (FLAT_COL_LOW - 1)) for j in range(FLAT_COL_LOW)]
    assert len(set(run_vals)) == run and (h16(run_vals) == 0.5).all()
    edge_val = None
    if edge is not None:
        b = bin_of(f32(0.25))
        _, hi = fused_window(b)
        if edge == "in":
            c = _lattice_in(0.5, float(bin_hi(b)), float(hi) - FLAT_EDGE_MARGIN).max()
        else:
            c = _lattice_in(0.5, float(hi) + FLAT_EDGE_MARGIN, float(hi) + 1e-3).min()
        edge_val = f32(c)
    n = FLAT_COL_HIGH + run + FLAT_COL_LOW + (edge is not None)
    slots_half = [p for p in range(n) if ((p >> 2) & 1) == half]
    slots_other = [p for p in range(n) if ((p >> 2) & 1) != half]
    s = np.zeros(n, f32)
    run_rows = slots_half[2:2 + run]                                          # spread over several 8-row groups
    s[run_rows] = run_vals
    rest = hi_vals + lo_vals
    free = sorted(set(range(n)) - set(run_rows))
    if edge is not None:
        at = [p for p in slots_half if p not in run_rows][-1]
        s[at] = edge_val
        free.remove(at)
    rng = np.random.default_rng(run * 7 + half)
    s[free] = np.asarray(rest, f32)[rng.permutation(len(rest))]
    X = np.zeros((n, D), f32)
    X[:, 0] = s
    mz = (500.0 + 0.01 * np.arange(n)).astype(f32)                            # windows of about ten rows
    above = FLAT_COL_HIGH + (edge is not None)                                # (an edge candidate stands above the run)
    return X, mz, above + run // 2, np.asarray(run_rows), edge_val


FLAT_KEEP_HALF = 32                               # FAL_FUSED_KEEP / 2: window candidates band_kernel keeps per (query, lane half)
FLAT_KEEP_HIGH = (11, 12, 13)                     # high rows in the run's half: with a run of 20, at most 31, 32, 33 kept there


@functools.lru_cache(maxsize=None)
def flat_keep(high_in_half):
    """`flat_collapse(20, 0, None)` with ONE precursor m/z for the whole bucket, so every row is a window candidate of every
    query, and with exactly `high_in_half` of the high rows at positions of lane half 0 beside the run.  band_kernel keeps the
    window candidates whose exact similarity reaches L = T~ - eps: the high rows and the run, 20 + high_in_half in half 0
    (one less for a query that is one of them).  -> X, mz, k_ann"""
    run = FUSED_MEM_HALF
    X0, _, k, run_rows, _ = flat_collapse(run, 0, None)
    s0 = X0[:, 0]
    n = len(s0)
    high = np.sort(s0[s0 > 0.6])
    low = np.sort(s0[s0 < 0.45])
    half0 = [p for p in range(n) if ((p >> 2) & 1) == 0 and p not in set(run_rows.tolist())]
    half1 = [p for p in range(n) if ((p >> 2) & 1) == 1]
    s = np.zeros(n, f32)
    s[run_rows] = s0[run_rows]
    rng = np.random.default_rng(high_in_half)
    h0 = rng.permutation(len(half0))[:high_in_half]
    h1 = rng.permutation(len(half1))[:len(high) - high_in_half]
    at_high = [half0[j] for j in h0] + [half1[j] for j in h1]
    s[at_high] = high[rng.permutation(len(high))]
    at_low = sorted(set(range(n)) - set(at_high) - set(run_rows.tolist()))
    s[at_low] = low[rng.permutation(len(low))]
    X = np.zeros((n, D), f32)
    X[:, 0] = s
    return X, np.full(n, 500.0, f32), k


FLAT_SURVIVORS = (15, 16, 17)                     # resolve_kernel ranks up to 16 survivors and sorts more (select.h)
FLAT_SURVIVOR_RUN_IN = FUSED_MEM_HALF - FUSED_MEM_HALF // 2                  # rows of a run of 20 inside the exact top-k: 10


@functools.lru_cache(maxsize=None)
def flat_survivors(c):
    """The rows of `flat_collapse(20, 0, None)` arranged so that ONE precursor window holds the whole run (bucket positions
    2 .. 41: the run at the lane-half-0 positions), c - 10 high rows and low rows on the positions between them.  k_ann ends
    inside the run: the exact top-k holds every high row and the ten run rows of largest exact value -- all twenty share one
    float16 value.  A low row of the window (a designed query; it is in nobody's top-k) therefore has exactly c survivors: 10
    run rows, told from the other ten only by their exact values, and c - 10 high rows.  The run and high rows of the window
    have c or c - 1.  Every other row has a precursor m/z of its own.  20 members and at most 20 kept candidates per lane
    half: nothing overflows, so resolve_kernel itself writes the lists.  -> X, mz, k_ann, designed query rows"""
    X0, _, k, run_rows, _ = flat_collapse(FUSED_MEM_HALF, 0, None)
    s0 = X0[:, 0]
    n = len(s0)
    high = np.sort(s0[s0 > 0.6])
    low = np.sort(s0[s0 < 0.45])
    lo_p, hi_p = int(run_rows[0]), int(run_rows[-1])
    between = [p for p in range(lo_p, hi_p + 1) if p not in set(run_rows.tolist())]
    rng = np.random.default_rng(c)
    between = [between[j] for j in rng.permutation(len(between))]
    n_high = c - FLAT_SURVIVOR_RUN_IN
    s = np.zeros(n, f32)
    s[run_rows] = s0[run_rows][rng.permutation(len(run_rows))]                # ids do not follow the exact values
    at_high, queries = between[:n_high], sorted(between[n_high:])
    s[at_high] = high[rng.permutation(len(high))[:n_high]]
    s[queries] = low[:len(queries)]
    outside = [p for p in range(n) if p < lo_p or p > hi_p]
    rest = np.concatenate([np.setdiff1d(high, s[at_high]), low[len(queries):]])
    s[outside] = rest[rng.permutation(len(rest))]
    assert np.array_equal(np.sort(s), np.sort(s0))
    X = np.zeros((n, D), f32)
    X[:, 0] = s
    mz = np.where(np.arange(n) < lo_p, 499.0 + 0.5 * np.arange(n), np.where(np.arange(n) <= hi_p, 500.0, 500.5 + 0.2 * np.arange(n)))
    return X, mz.astype(f32), k, np.asarray(queries)


def flat_kept_model(X, k, mz, rel=REL):
    """band_kernel on every query of a flat bucket of single products: the window candidates (not the query itself) whose exact
    similarity reaches L = T~ - eps, per lane half of the candidate -> kept [n, 2]"""
    A, single = approx_sims(X)
    assert single.all()
    E = exact_sims(X)
    n = len(X)
    pos = np.arange(n)
    half = (pos >> 2) & 1
    kept = np.zeros((n, 2), np.int64)
    for i in range(n):
        bstar, _, _, T, _, _ = fused_members(A[i], k, pos, rel)
        _, hi = fused_window(bstar, rel)
        eps = f32(f32(rel) * hi + f32(ABS))                                   # (hi = bin_hi + m)
        L = f32(f32(T) - eps)
        ok = (np.abs(mz.astype(f64) - f64(mz[i])) <= TOL_DA) & (pos != i) & (E[i] >= L)
        kept[i] = [(ok & (half == 0)).sum(), (ok & (half == 1)).sum()]
    return kept


def flat_overflow_model(X, k, rel=REL):
    """rows of a flat bucket whose approx_kernel member list overflows (-> exact fallback), and the smallest distance of any
    approximate value from a window edge over the rows of the bucket"""
    A, _ = approx_sims(X)             # (two-term pairs: within a float32 rounding; the designs keep them far from every edge)
    pos = np.arange(len(X))
    over, dist = [], np.inf
    for i in range(len(X)):
        _, m0, m1, _, dmin, _ = fused_members(A[i], k, pos, rel)
        over.append(m0 > FUSED_MEM_HALF or m1 > FUSED_MEM_HALF)
        dist = min(dist, dmin)
    return np.asarray(over), dist


# --------------------------------------------------------------------------- IVF buckets: inversion, collapse, edge
IVF_NLIST = 8
IVF_FILL = (1, 31, 33, 97, 127, 129)              # rows of lists 2 .. 7 (axis c, one list each)
IVF_LIST0, IVF_LIST1 = 126, 29                    # rows on axis 0 / axis 1; with the two edge / three inversion queries that fall
                                                  # to them the lists hold 128 and 32 rows
IVF_LISTS = (128, 32) + IVF_FILL
IVF_H, IVF_RUNS = 20, (35, 36, 37)                # run + 2 X + 2 edge rows inside = 39, 40, 41 members for the edge queries
                                                  # (the inversion queries see Y too: 41, 42, 43)
IVF_NPROBE = 2


def _edge_design():
    """The run's key is T = key(0.25) for every query whose first component rounds to 0.5, and delta(T) = 50.  Axis 0 reaches
    the keys T + 16 j (above 0.5) and T - 8 j (below): T + 48 and T - 48 = delta - 2 on both sides, for every such query.  The
    keys delta + 2 away need another step: they stand on axis 1 and are reached from the edge queries (down(-1), q1) alone.
    Brute force over the float16 value q1, the first that reaches both -> q1, (in_hi, in_lo) axis-0 values, (out_hi, out_lo)
    axis-1 values (all float16 values), T, delta"""
    T = int(key_of(0.25))
    delta, _ = key_delta(T)
    assert delta - 2 == 48
    inside = (0.5 * (1 + 6 * U), 0.5 - 6 * 2.0 ** -12)
    assert tuple(int(key_of(0.5 * c)) for c in inside) == (T + delta - 2, T - delta + 2)
    for q1 in np.arange(1147, 1966, dtype=f64) * 2.0 ** -12:                # float16 values in [0.28, 0.48)
        got = []
        for w in (T + delta + 2, T - delta - 2):
            c = _lattice_in(q1, (w - 0.3) / 65535.0, (w + 0.3) / 65535.0)     # 0.2 units away from a rounding boundary
            if len(c) == 0:
                break
            got.append(float(c[0]))
        if len(got) == 2:
            return float(q1), inside, tuple(got), T, delta
    raise AssertionError("no edge design")


@functools.lru_cache(maxsize=None)
def ivf_bucket(run, d=D, wide_row=False):
    """One bucket of IVF_NLIST lists (k-means with 0 iterations: the centroids are the seed rows floor(i n / 8), one per axis,
    so list c = the rows on axis c; the two-column query rows fall to list 0 or 1).
      axis 0: the seed (0.375), IVF_H high float16-exact rows, X = 2 x down(-1, 1), the run 0.5 (1 + t u), the two edge rows
              delta - 2 from the run's key, low rows
      axis 1: the seed, Y = 2 x up(-1, 0), the two edge rows delta + 2 from the run's key (for the edge queries), low rows
      queries: 3 x Q_inv = (down(-1), up(-1)): X and Y inverted as in `flat_inversion`;
               2 x Q_edge = (down(-1), q1): the edge rows' keys lie delta -+ 2 around the run's key, on both sides
      axes 2 .. 7: IVF_FILL rows each, distinct float16-exact values
    The queries, X, Y, the edge rows and the first six rows of the run share one precursor m/z; every other row has a window
    of its own.  wide_row: one more row with 70 non-zeros (the index then keeps the dense gather), which joins list 0.
    -> dict"""
    q1, e_in, e_out, T, delta = _edge_design()
    q1v = smallest_rounding_to(q1)                                            # float16 adds: the edge rows above T are over-estimated
    a0 = [("seed", f32(0.375))] + [("H", f32(0.5625 + j / 128.0)) for j in range(IVF_H)] + [("X", down(-1, 1))] * 2
    a0 += [("run", f32(0.5 * (1.0 + (j + 1.0) / (run + 2.0) * U))) for j in range(run)]
    # the edge rows' exact values lie as far towards T as float16 rounding allows
    a0 += [("edge", smallest_rounding_to(e_in[0])), ("edge", largest_rounding_to(e_in[1]))]
    a0 += [("low", f32(0.25 + j / 1024.0)) for j in range(IVF_LIST0 - len(a0))]
    a1 = [("seed", f32(0.375))] + [("Y", up(-1, 0))] * 2
    a1 += [("edge", smallest_rounding_to(e_out[0])), ("edge", largest_rounding_to(e_out[1]))]
    a1 += [("low", f32(0.25 + j / 1024.0)) for j in range(IVF_LIST1 - len(a1))]
    rows = [(0, v, None, t) for t, v in a0] + [(1, v, None, t) for t, v in a1]
    for c, m in zip(range(2, IVF_NLIST), IVF_FILL):
        rows += [(c, f32(0.5 + j / 256.0), None, "seed" if j == 0 else "fill") for j in range(m)]
    rows += [(0, down(-1, 0), up(-1, 0), "Qinv")] * 3 + [(0, down(-1, 0), q1v, "Qedge")] * 2
    if wide_row:
        rows.append((-1, f32(0.05), None, "wide"))
    n = len(rows)
    # positions: the seeds first (floor(i n / 8) holds the seed of axis i), then the window block in a gap without a seed
    seeds = [(i * n) // IVF_NLIST for i in range(IVF_NLIST)]
    block = [j for j, r in enumerate(rows) if r[3] in ("Qinv", "Qedge", "X", "Y", "edge")]
    block += [j for j, r in enumerate(rows) if r[3] == "run"][:6]
    rng = np.random.default_rng(run)
    block = [block[j] for j in rng.permutation(len(block))]
    place = np.full(n, -1)
    for i, p in enumerate(seeds):
        place[p] = next(j for j, r in enumerate(rows) if r[3] == "seed" and r[0] == i)
    b0 = seeds[1] + 1
    assert b0 + len(block) < seeds[2]
    place[b0:b0 + len(block)] = block
    used = set(place[place >= 0].tolist())
    rest = [j for j in range(n) if j not in used]
    rest = [rest[j] for j in rng.permutation(len(rest))]
    place[place < 0] = rest
    X = np.zeros((n, d), f32)
    kind = []
    for p, j in enumerate(place):
        c, v, v1, t = rows[j]
        kind.append(t)
        if c < 0:
            X[p, 20:90] = v
        else:
            X[p, c] = v
            if v1 is not None:
                X[p, 1] = v1
    kind = np.asarray(kind)
    mz = 500.0 + 0.2 * np.arange(n)
    mz[b0:b0 + len(block)] = mz[b0]
    return {"X": X, "mz": mz.astype(f32), "kind": kind, "T": T, "delta": delta, "q1": q1, "edges": e_in + e_out, "run": run,
            "block": np.arange(b0, b0 + len(block))}


def ivf_model(X, perm, loff, probes, k, rel=REL):
    """select16 on every query of one bucket: the modelled keys of its candidates (the probed lists) -> per query
    nc, T (the k-th largest key, -1 when nc <= k), delta, members (keys within delta of T), n_above (keys above T)"""
    A, _ = approx_sims(X)
    K = key_of(A)
    out = []
    for i in range(len(X)):
        cand = np.concatenate([perm[loff[l]:loff[l + 1]] for l in probes[i] if l >= 0]).astype(np.int64)
        keys = K[i, cand]
        if len(cand) <= k:
            out.append((len(cand), -1, 0, 0, 0))
            continue
        T = int(np.sort(keys)[::-1][k - 1])
        delta, _ = key_delta(T, rel)
        out.append((len(cand), T, delta, int((np.abs(keys - T) <= delta).sum()), int((keys > T).sum())))
    return np.asarray(out)


def ivf_k_values(b, perm, loff, probes):
    """the k_ann values of an `ivf_bucket`: 'inversion' (the Q_inv queries' k-th place between X and Y), 'collapse' (inside the
    run for Q_inv) and 'edge' (inside the run for Q_edge)"""
    A, _ = approx_sims(b["X"])
    K = key_of(A)
    out = {}
    for name, qk, tk in (("inversion", "Qinv", None), ("collapse", "Qinv", b["T"]), ("edge", "Qedge", b["T"])):
        i = int(np.flatnonzero(b["kind"] == qk)[0])
        cand = np.concatenate([perm[loff[l]:loff[l + 1]] for l in probes[i] if l >= 0]).astype(np.int64)
        keys = K[i, cand]
        if tk is None:
            out[name] = int((keys > K[i, np.flatnonzero(b["kind"] == "Y")[0]]).sum()) + 1     # the first Y is the approximate k-th
        else:
            out[name] = int((keys > tk).sum()) + b["run"] // 2
    return out


# --------------------------------------------------------------------------- k-means assignment and coarse quantiser
ASSIGN_NLIST = (128, 129, 200, 512, 513, 1024, 1025, 2048)
ASSIGN_ROWS_PER_LIST = 3
PROBE_REPEATS = (15, 16, 17)                      # identical centroids on one axis: that many equal keys for its rows


@functools.lru_cache(maxsize=None)
def close_pair(g_lo, g_hi, inverted, scale=1.0):
    """Two (row component, centroid component) products around scale^2 / 4 for a two-axis row:
        side a (axis 0): x0 = down(-1) * scale, centroid down(-1):  approx = 0.25, exact ~ 0.25 (1 + 2 u)
        side b (axis 1): x1 in [0.25, 0.5) * scale and a centroid in [0.5, 1), both the SMALLEST float32 rounding to their
                         float16 value: over-estimated
    with g = (approx b - approx a) / (1.3e-3 approx b + 2e-6) in (g_lo, g_hi); inverted: exact a > exact b, by the widest margin
    found; else exact a < exact b and g nearest the middle of the window.  -> x0, x1, ca, cb (float32), g, exact a, exact b"""
    x0, ca = f32(down(-1) * f32(scale)), down(-1)
    aa = float(h16(x0) * h16(ca))
    ea = f32(f64(x0) * f64(ca))
    B = np.arange(1024, 2048, dtype=f64) * 2.0 ** -11                        # float16 values in [0.5, 1)
    X1 = np.arange(1024, 2048, dtype=f64) * 2.0 ** -12 * scale               # [0.25, 0.5) * scale
    ab = B[:, None] * X1[None, :]
    g = (ab - aa) / (REL * ab + ABS)
    Bv = np.array([smallest_rounding_to(t) for t in B])
    Xv = np.array([smallest_rounding_to(t) for t in X1])
    eb = (Bv[:, None].astype(f64) * Xv[None, :].astype(f64)).astype(f32)
    ok = (g > g_lo) & (g < g_hi)
    margin = (f64(ea) - eb.astype(f64)) / f64(ea)
    ok &= (margin > 0) if inverted else (margin < 0)
    assert ok.any(), (g_lo, g_hi, inverted)
    score = np.where(ok, np.abs(margin) if inverted else 1.0 - np.abs(g - 0.5 * (g_lo + g_hi)), -1.0)
    i, j = np.unravel_index(int(np.argmax(score)), score.shape)
    return x0, Xv[j], ca, Bv[i], float(g[i, j]), ea, eb[i, j]


# row types of an assignment bucket: (name, g window, inverted, where the two centroids stand)
ASSIGN_TYPES = (("inverted", 1.05, 2.1, True, "apart"),       # exact best = a, approximate best = b, beyond 1.0 eps, inside 2.2 eps
                ("inside", 2.12, 2.19, False, "apart"),       # runner-up just inside best - 2.2 eps
                ("outside", 2.21, 2.28, False, "apart"),      # ... just outside: the approximate winner is taken
                ("same_group", 1.05, 2.1, True, "same"),      # both contenders in one 32-centroid group
                ("many", 1.05, 2.1, True, "copies"))          # centroid a five times, in five 32-centroid groups: > 4 contenders


@functools.lru_cache(maxsize=None)
def assign_bucket(n_list):
    """k-means with 0 iterations: centroid i = row floor(i n / n_list), n = ASSIGN_ROWS_PER_LIST * n_list.  Row type t uses
    the axes 2 t (centroid a) and 2 t + 1 (centroid b); the other centroids stand on the axes 10 .. 63, repeated by identical
    seed rows (exact ties: the lowest id wins), three of those axes PROBE_REPEATS times.  Every row that is not a seed is a
    designed row (in turn), a `probe3` row (two clear lists, then an inverted pair as third and fourth) or a copy of a seed.
    -> X, dict of row ids per type, centroid axis per list"""
    n = ASSIGN_ROWS_PER_LIST * n_list
    groups = (n_list + 31) // 32
    cent = {}                                                                 # list id -> (axis, value)
    pairs = {}
    for t, (name, g_lo, g_hi, inv, where) in enumerate(ASSIGN_TYPES):
        x0, x1, ca, cb, g, ea, eb = close_pair(g_lo, g_hi, inv)
        pairs[name] = (x0, x1, g)
        if where == "same":
            ida, idb = 40 + t, 41 + t                                         # one 32-centroid group
        else:
            ida = 3 + t                                                       # group 0; b in another group (another 128 when merged)
            idb = 32 * (1 + t % 3) + 5 + t if n_list <= 128 else n_list - 1 - t
        assert ida not in cent and idb not in cent
        cent[ida] = (2 * t, ca)
        cent[idb] = (2 * t + 1, cb)
        if where == "copies":
            for gi in range(min(groups, 6)):
                assert 32 * gi + 17 not in cent
                cent[32 * gi + 17] = (2 * t, ca)
    free = [c for c in range(n_list) if c not in cent]
    order = [10] * PROBE_REPEATS[0] + [11] * PROBE_REPEATS[1] + [12] * PROBE_REPEATS[2] + [13, 14]      # 13, 14: one centroid each
    while len(order) < len(free):
        order += list(range(15, 64))
    for c, ax in zip(free, order):
        cent[c] = (ax, f32(0.5))
    X = np.zeros((n, D), f32)
    seeds = (np.arange(n_list, dtype=np.int64) * n) // n_list
    for c, p in enumerate(seeds):
        X[p, cent[c][0]] = cent[c][1]
    others = [p for p in range(n) if p not in set(seeds.tolist())]
    ids = {name: [] for name, *_ in ASSIGN_TYPES}
    ids["probe3"], ids["copy"] = [], []
    x0h, x1h, _, _, _, _, _ = close_pair(1.05, 2.1, True, 0.5)
    for j, p in enumerate(others):
        t = j % 12
        if t < len(ASSIGN_TYPES):
            name = ASSIGN_TYPES[t][0]
            X[p, 2 * t], X[p, 2 * t + 1] = pairs[name][0], pairs[name][1]
            ids[name].append(p)
        elif t == len(ASSIGN_TYPES):
            # two clear lists (axes 13, 14), then the inverted pair of type 0 at half the size as third and fourth
            X[p, 13], X[p, 14], X[p, 0], X[p, 1] = f32(0.625), f32(0.5625), x0h, x1h
            ids["probe3"].append(p)
        else:
            ax = (10, 11, 12, 15, 16, 17)[t - len(ASSIGN_TYPES) - 1]
            X[p, ax] = f32(0.5 + (j % 7) / 64.0)
            ids["copy"].append(p)
    return X, {k: np.asarray(v) for k, v in ids.items()}, np.asarray([cent[c][0] for c in range(n_list)])
