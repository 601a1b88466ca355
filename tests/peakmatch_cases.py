"""Spectrum pairs that drive the matched-peak cosine's assignment solver (csrc/peakmatch.h) through every component size,
shared by the host-build test (test_peakmatch_cpu.py) and the device tests (test_gpu_exact_paths.py).

A pair has a dense group of `ga` query peaks and `gb` peaks of the other spectrum (1..32 each) inside a span of 0.8 / 1.5 /
3 / 6 fragment tolerances -- the narrow spans chain all of them into one component, the wide ones into several -- plus
scattered peaks.  `kind` chooses the intensities / positions:
  "lognormal"  lognormal intensities (no ties)
  "equal"      every intensity the same
  "zeros"      30 % of the intensities are zero
  "dupmz"      group positions drawn from a coarse grid: repeated m/z values inside and across the two spectra
  "quant"      intensities from {1, 2, 3}: equal-weight optimal assignments of different cardinality exist; only the score
               is determined, not the matched-peak count
All spectra are L2-normalised in float32 and m/z-sorted."""
import numpy as np

f32, f64 = np.float32, np.float64
TOLS = (0.02, 0.05, 0.5)
SPANS = (0.8, 1.5, 3.0, 6.0)
KINDS = ("lognormal", "equal", "zeros", "dupmz", "quant")
MAX_COMP = 32


def _intensities(rng, n, kind):
    if kind == "equal":
        it = np.ones(n)
    elif kind == "quant":
        it = rng.integers(1, 4, n).astype(np.float64)
    else:
        it = rng.lognormal(0.0, 1.0, n)
        if kind == "zeros":
            it[rng.random(n) < 0.3] = 0.0
    it = it.astype(f32)
    nrm = np.sqrt(np.sum(it.astype(f64) ** 2)).astype(f32)
    return it / nrm if nrm > 0 else it


def _side(rng, g, centre, span, tol, kind, n_scatter):
    if kind == "dupmz":
        grp = centre + rng.integers(0, 9, g) * (span * tol / 8.0)
    else:
        grp = centre + rng.uniform(0.0, span * tol, g)
    mz = np.sort(np.concatenate([grp, rng.uniform(150.0, 1400.0, n_scatter)])).astype(f32)
    return mz, _intensities(rng, len(mz), kind)


def make_pair(rng, kind="lognormal", ga=None, gb=None, span=None, tol=None):
    """-> (mz_a, it_a, mz_b, it_b, tol)"""
    ga = int(rng.integers(1, MAX_COMP + 1)) if ga is None else ga
    gb = int(rng.integers(1, MAX_COMP + 1)) if gb is None else gb
    span = float(rng.choice(SPANS)) if span is None else span
    tol = float(rng.choice(TOLS)) if tol is None else tol
    centre = rng.uniform(300.0, 900.0)
    a = _side(rng, ga, centre, span, tol, kind, int(rng.integers(0, 13)))
    b = _side(rng, gb, centre, span, tol, kind, int(rng.integers(0, 13)))
    return (*a, *b, tol)


def make_pairs(n, seed, kind="lognormal"):
    rng = np.random.default_rng(seed)
    return [make_pair(rng, kind) for _ in range(n)]


def components(mz_a, mz_b, tol):
    """The window walk of the reference's cosine_fast (similarity.py:45-63, numba's types: `peak - tol` in float64, the
    difference in float32) restated: consecutive query peaks whose windows of the other spectrum overlap form a component.
    -> [(query peaks, peaks of the other spectrum)] per component"""
    out = []
    nb = len(mz_b)
    if len(mz_a) == 0 or nb == 0:
        return out
    tol = f64(tol)
    b64 = mz_b.astype(f64)
    o = nr = qs = qe = 0
    for p in range(len(mz_a)):
        pm = mz_a[p]
        lo = f64(pm) - tol
        while o < nb - 1 and lo > b64[o]:
            o += 1
        q = o
        while q < nb and f64(abs(f32(pm - mz_b[q]))) <= tol:
            q += 1
        if q == o:
            continue
        if nr > 0 and o >= qe:
            out.append((nr, qe - qs))
            nr = 0
        if nr == 0:
            qs = o
        nr += 1
        qe = q if nr == 1 else max(qe, q)
    if nr > 0:
        out.append((nr, qe - qs))
    return out


def too_large(comps):
    """a component the library refuses: more than 32 peaks on either side (components of one query peak are solved in place)"""
    return any(nr > 1 and (nr > MAX_COMP or nc > MAX_COMP) for nr, nc in comps)


class Coverage:
    """which component shapes a set of pairs contains (asserted by the tests from the inputs, not asked of the library)"""

    def __init__(self):
        self.rows, self.cols, self.transposed, self.dropped, self.pairs = set(), set(), 0, 0, 0

    def add(self, comps):
        self.pairs += 1
        if too_large(comps):
            self.dropped += 1
            return False
        for nr, nc in comps:
            if nr > 1:                                   # the solver's components
                self.rows.add(nr)
                self.cols.add(nc)
                self.transposed += nr > nc
        return True

    def check(self):
        assert self.dropped <= 0.02 * self.pairs, f"{self.dropped} of {self.pairs} pairs have a component above {MAX_COMP}"
        want = set(range(2, MAX_COMP + 1))
        assert want <= self.rows, f"no component with {sorted(want - self.rows)} query peaks"
        assert want <= self.cols, f"no component with {sorted(want - self.cols)} peaks of the other spectrum"
        assert self.transposed > 0


def to_csr(pairs):
    """pairs -> (mz, it, ptr): spectrum 2k = the query of pair k, 2k + 1 the other"""
    mz, it, sizes = [], [], []
    for a_mz, a_it, b_mz, b_it, _ in pairs:
        mz += [a_mz, b_mz]
        it += [a_it, b_it]
        sizes += [len(a_mz), len(b_mz)]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cat = lambda xs: np.concatenate(xs).astype(f32) if xs else np.zeros(0, f32)
    return cat(mz), cat(it), ptr


def exact_pair(n_side, tol=0.05):
    """a pair whose one component is exactly n_side x n_side: both spectra hold n_side peaks inside 0.8 tolerances (every
    query peak sees every other peak), distinct intensities, + far-away peaks"""
    rng = np.random.default_rng(1000 + n_side)
    out = []
    for _ in range(2):
        grp = 500.0 + np.sort(rng.uniform(0.0, 0.8 * tol, n_side))
        mz = np.concatenate([[200.0, 300.0], grp, [900.0]]).astype(f32)
        out += [mz, _intensities(rng, len(mz), "lognormal")]
    return (*out, tol)
