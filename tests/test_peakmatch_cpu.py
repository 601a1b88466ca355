"""csrc/peakmatch.h under a host build (tests/hostbuild.py) against the oracle's `cosine_fast` (scipy's
linear_sum_assignment on the dense cost matrix; pinned to the reference by tests/golden/cosine_fast.npz): the window walk, the
component decomposition and the Hungarian solver at every component size up to kMaxComp, both orientations, tie-heavy
inputs.  Score: float64 `==`; matched-peak count: `==` wherever the optimum is unique in cardinality."""
import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import hostbuild
from tests import peakmatch_cases as pc

pytestmark = pytest.mark.skipif(not hostbuild.have_compiler(), reason="no host C++ compiler and no hipcc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hostbuild.build(tmp_path_factory.mktemp("hostbuild"))


def _run(lib, pairs):
    """-> (library score clipped, n_match, ok), oracle (score, n_match), kept mask by the test's own component walk, coverage"""
    cov = pc.Coverage()
    keep = np.array([cov.add(pc.components(p[0], p[2], p[4])) for p in pairs])
    got_s, got_n, got_ok = np.zeros(len(pairs)), np.zeros(len(pairs), np.int32), np.zeros(len(pairs), bool)
    for tol in pc.TOLS:                                      # one batched call per tolerance
        ks = [k for k, p in enumerate(pairs) if p[4] == tol]
        s, n, ok = hostbuild.pair_scores(lib, *pc.to_csr([pairs[k] for k in ks]), tol)
        got_s[ks], got_n[ks], got_ok[ks] = np.clip(s, 0.0, 1.0), n, ok
    exp = [fo.cosine_fast(*p) for p in pairs]
    return got_s, got_n, got_ok, np.array([e[0] for e in exp]), np.array([e[1] for e in exp]), keep, cov


def test_max_comp_is_32(lib):
    assert lib.t_max_comp() == pc.MAX_COMP


def test_every_component_size_equals_the_oracle(lib):
    pairs = pc.make_pairs(20000, seed=101)
    got_s, got_n, got_ok, exp_s, exp_n, keep, cov = _run(lib, pairs)
    cov.check()
    assert cov.transposed > 1000 and 32 in cov.rows and 32 in cov.cols
    assert np.array_equal(got_ok, keep)                      # the library refuses exactly the pairs above 32, no others
    assert np.array_equal(got_s[keep], exp_s[keep]), int((got_s[keep] != exp_s[keep]).sum())
    assert np.array_equal(got_n[keep], exp_n[keep]), int((got_n[keep] != exp_n[keep]).sum())


@pytest.mark.parametrize("kind", ["equal", "zeros", "dupmz"])
def test_tie_heavy_inputs_equal_the_oracle(lib, kind):
    pairs = pc.make_pairs(2000, seed=200 + pc.KINDS.index(kind), kind=kind)
    got_s, got_n, got_ok, exp_s, exp_n, keep, cov = _run(lib, pairs)
    assert cov.dropped <= 0.02 * cov.pairs and len(cov.rows) > 20
    assert np.array_equal(got_ok, keep)
    assert np.array_equal(got_s[keep], exp_s[keep]), int((got_s[keep] != exp_s[keep]).sum())
    assert np.array_equal(got_n[keep], exp_n[keep]), int((got_n[keep] != exp_n[keep]).sum())


def test_quantised_intensities_score_equals_the_oracle(lib):
    """Intensities from {1, 2, 3}: optimal assignments of equal weight and different cardinality exist, scipy and the
    library's Hungarian order pick differently -- the score is determined, the matched-peak count is not."""
    pairs = pc.make_pairs(2000, seed=300, kind="quant")
    got_s, got_n, got_ok, exp_s, exp_n, keep, cov = _run(lib, pairs)
    assert cov.dropped <= 0.02 * cov.pairs
    assert np.array_equal(got_ok, keep)
    differ = int((got_n[keep] != exp_n[keep]).sum())
    assert np.array_equal(got_s[keep], exp_s[keep]), \
        f"{int((got_s[keep] != exp_s[keep]).sum())} scores differ (matched-peak count differs in {differ} of {int(keep.sum())})"


@pytest.mark.parametrize("n_side,ok", [(31, True), (32, True), (33, False)])
def test_component_of_exactly_32_is_solved_33_is_refused(lib, n_side, ok):
    for swap in (False, True):
        p = pc.exact_pair(n_side)
        if swap:
            p = (p[2], p[3], p[0], p[1], p[4])
        comps = pc.components(p[0], p[2], p[4])
        assert (n_side, n_side) in comps
        s, n, good = hostbuild.pair_scores(lib, *pc.to_csr([p]), p[4])
        assert bool(good[0]) == ok
        if ok:
            es, en = fo.cosine_fast(*p)
            assert min(max(s[0], 0.0), 1.0) == es and n[0] == en and en >= n_side


def test_rectangular_components_at_the_limit(lib):
    """32 x k and k x 32 (transposed solver) for every k, 33 on either side refused"""
    rng = np.random.default_rng(7)
    for k in range(1, 33):
        for ga, gb in ((32, k), (k, 32)):
            p = pc.make_pair(rng, ga=ga, gb=gb, span=0.8, tol=0.05)
            comps = pc.components(p[0], p[2], p[4])
            s, n, good = hostbuild.pair_scores(lib, *pc.to_csr([p]), p[4])
            assert bool(good[0]) == (not pc.too_large(comps))
            if good[0]:
                es, en = fo.cosine_fast(*p)
                assert min(max(s[0], 0.0), 1.0) == es and n[0] == en, (ga, gb)
    for ga, gb in ((33, 2), (2, 33)):
        p = pc.make_pair(rng, ga=ga, gb=gb, span=0.8, tol=0.5)
        assert pc.too_large(pc.components(p[0], p[2], p[4]))
        assert not hostbuild.pair_scores(lib, *pc.to_csr([p]), p[4])[2][0]


def test_exact_distance_applies_min_matches_and_clipping(lib):
    pairs = [p for p in pc.make_pairs(600, seed=9) if p[4] == 0.05]
    keep = np.array([not pc.too_large(pc.components(p[0], p[2], p[4])) for p in pairs])
    for mm in (0, 3, 12):
        d, ok = hostbuild.exact_distances(lib, *pc.to_csr(pairs), 0.05, mm)
        exp = np.array([1.0 - (0.0 if nm < mm else s) for s, nm in (fo.cosine_fast(*p) for p in pairs)])
        assert np.array_equal(ok, keep) and np.array_equal(d[keep], exp[keep])
    assert lib.t_pair_distance(1.5, 5, 0) == 0.0 and lib.t_pair_distance(-0.5, 5, 0) == 1.0
    assert lib.t_pair_distance(0.25, 2, 3) == 1.0 and lib.t_pair_distance(0.25, 3, 3) == 0.75


def test_empty_and_single_peak_spectra(lib):
    e = np.zeros(0, np.float32)
    one_mz, one_it = np.array([500.0], np.float32), np.array([1.0], np.float32)
    far = np.array([700.0], np.float32)
    cases = [(e, e, e, e), (one_mz, one_it, e, e), (e, e, one_mz, one_it), (one_mz, one_it, one_mz, one_it),
             (one_mz, one_it, far, one_it)]
    for tol in (0.0, 0.05):
        for c in cases:
            s, n, ok = hostbuild.pair_scores(lib, *pc.to_csr([(*c, tol)]), tol)
            es, en = fo.cosine_fast(*c, tol)
            assert ok[0] and s[0] == es and n[0] == en
