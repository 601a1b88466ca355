"""The builders of tests/front_cases.py against the oracle alone (no GPU): the restated launch rules, the gather assembly
of expected output, and that every edge case reaches the outcome it was built for."""
import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import front_cases as fc


@pytest.mark.parametrize("cus", [256, 304])
def test_chunk_rule_at_the_table_sizes(cus):
    T = cus * 128
    assert T == cus * 32 * 4
    for chunk in (2, 4, 8, 16):
        n = fc.vectorize_n(chunk, cus)
        assert n == chunk * T + 37 and fc.vectorize_chunk(n, cus) == chunk
        assert fc.vectorize_chunk(chunk * T, cus) == chunk and fc.vectorize_chunk(chunk * T - 1, cus) == chunk // 2
        assert n % chunk != 0                                      # a partial last chunk
        assert -(-n // chunk) % (cus * 32) != 0                    # the wave count is no multiple of the grid
    assert fc.vectorize_n(1, cus) == 2 * T - 1 and fc.vectorize_chunk(2 * T - 1, cus) == 1
    assert fc.vectorize_chunk(1, cus) == 1 and fc.vectorize_chunk(100 * T, cus) == 16
    assert {c[0] for c in fc.VECTORIZE_CASES} == {1, 2, 4, 8, 16}
    # the other kernels' sizes: more than one turn of their grids
    assert fc.prep_turns_n(cus) > 2 * cus * 64 * 4 and fc.prep_turns_n(cus) % 4 == 1
    assert len(fc.bin_values(cus)) > 2 * cus * 8 * 256
    if cus == 256:                                                 # (the numbers of the 256-CU part)
        assert [fc.vectorize_n(c, cus) for c in (1, 2, 4, 8, 16)] == [65535, 65573, 131109, 262181, 524325]


def test_vectorize_library_and_row_order():
    lib = fc.vec_library()
    sizes = np.diff(lib["indptr"])
    r = lib["row"]
    for p in (0, 1, 2, 63, 64, 65, 127, 128, 129, 200):
        assert sizes[r[p]] == p
    ref = fc.vec_reference(50, 64, True)
    assert not ref[r["outside"]].any() and not ref[r[0]].any()
    assert sizes[r["one_bin"]] == 40 and np.count_nonzero(ref[r["one_bin"]]) == 1
    assert not ref[:, 50:].any()                                   # the columns behind low_dim
    # ref[row_order] is what the oracle gives for a row order it accepts: a true permutation
    perm = np.random.default_rng(0).permutation(len(sizes))
    for low_dim, width, norm in ((50, 64, True), (400, 400, True), (5, 8, False)):
        ref = fc.vec_reference(low_dim, width, norm)
        direct = fo.vectorize(lib["mz"], lib["intensity"], lib["indptr"], lib["min_mz"], fc.BIN, lib["n_bins"], low_dim,
                              norm=norm, row_order=perm, width=width)
        assert np.array_equal(ref[perm].view(np.uint32), direct.view(np.uint32))
    # the layout: patterns at 16-aligned offsets, long rows about 1 %, a few million peaks at the most
    n = fc.vectorize_n(16, 256)
    order = fc.vec_row_order(n)
    assert order.shape == (n,) and order.min() >= 0 and order.max() < len(sizes)
    pats = fc.vec_patterns(lib)
    for base in (0, n // 16 // 2, n // 16 - len(pats)):
        for j, p in enumerate(pats):
            assert order[16 * (base + j): 16 * (base + j + 1)].tolist() == p
    assert sizes[order[:16]].sum() == 0                            # sixteen empty rows
    cnt = sizes[order]
    assert 0.005 < (cnt > 64).mean() < 0.015 and cnt.sum() < 6e6
    assert cnt[-1] == 129 and cnt[-4] == 0
    for c in (2, 4, 8, 16):                                        # an empty row first, 129 peaks last, in a chunk of each size
        starts = np.arange(0, n - c + 1, c)
        assert np.any((cnt[starts] == 0) & (cnt[starts + c - 1] == 129))
    seq = lambda *xs: np.any(np.all([cnt[i: n - len(xs) + 1 + i] == x for i, x in enumerate(xs)], axis=0))
    assert seq(200, 0, 65, 64) and seq(200, 1) and seq(64, 200, 0)


def test_vectorize_expected_modes():
    ref = fc.vec_reference(50, 64, True)
    hi, lo = fc.f16_planes(ref)
    (s,) = fc.vec_expected(ref, "split16")
    assert s.shape == (len(ref), 2, 64) and np.array_equal(s[:, 0], hi) and np.array_equal(s[:, 1], lo)
    err = np.abs(ref.astype(np.float64) - (hi.astype(np.float64) + lo.astype(np.float64) / 2048))
    assert err.max() < 2.0 ** -21                                  # the split holds the float32 value
    img, h = fc.vec_expected(ref, "f16+image")
    assert img.dtype == np.float32 and h.dtype == np.float16 and np.array_equal(img, h.astype(np.float32))


@pytest.mark.parametrize("which", [0, 1])
def test_prep_gather_assembly_equals_the_oracle_on_the_gathered_batch(which):
    valid = fc.prep_library_expected(which)[0]
    assert 0.1 <= valid.mean() <= 0.9
    sizes = np.diff(fc.prep_library()[2])
    assert (sizes == 0).sum() >= 200 and {70, 130, 300} <= set(sizes.tolist()) and (fc.prep_library()[4] < 0).sum() > 50
    pick = fc.prep_pick(3000, seed=8)
    batch = fc.prep_gather(pick)
    assert len(batch[2]) == 3001 and batch[2][-1] == len(batch[0]) == len(batch[1])
    direct = fo.process_spectra(*batch, **fc.PREP_OPTION_SETS[which])
    e = fc.prep_gather_expected(which, pick)
    assert np.array_equal(e[0], direct[0]) and np.array_equal(e[1], direct[1])
    assert np.array_equal(e[2].view(np.uint32), direct[2].view(np.uint32))
    assert np.array_equal(e[3].view(np.uint32), direct[3].view(np.uint32))          # (NaN patterns included)


def test_edge_table_reaches_both_outcomes():
    cases = fc.prep_edge_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        out = fo.process_spectra(*c["batch"], **c["opts"])
        fc.check_edge_counts(c, out)
    by = {c["name"]: c for c in cases}
    # top-N: which of the tied peaks stay (the lower m/z first), run by run
    tie_pos = np.r_[60:71, 125:132]
    for keep in (1, 10, 11, 12, 17):
        c = by[f"top{40 + keep}_ties"]
        _, _, omz, _ = fo.process_spectra(*c["batch"], **c["opts"])
        kept = np.isin(c["batch"][0][tie_pos].astype(np.float32), omz)
        assert kept.tolist() == [True] * keep + [False] * (18 - keep)
    # precursor: at every charge state's target both a kept and a removed probe
    c = by["precursor_edges"]
    mz, _, ip, pmz, ch = c["batch"]
    _, oip, omz, _ = fo.process_spectra(*c["batch"], **c["opts"])
    assert ch.tolist() == [1, 2, 3, -2, 0]
    for i in range(len(pmz)):
        m, o = mz[ip[i]:ip[i + 1]], omz[oip[i]:oip[i + 1]].astype(np.float64)
        targets = fc.precursor_targets(pmz[i], ch[i])
        assert len(targets) == (abs(int(ch[i])) or 1)
        for t in targets:
            near = m[np.abs(m - t) < 2.0]
            left = o[np.abs(o - t) < 2.0]
            assert len(near) == 6 and 0 < len(left) < 6, (i, t, len(left))
    # the sizes of the norm tree's passes
    c = by["norm_tree_sizes"]
    assert np.diff(fo.process_spectra(*c["batch"], **c["opts"])[1]).tolist() == [255, 256, 257, 512, 513, 64, 65, 128]
    c = by["indptr_repeats"]
    assert fo.process_spectra(*c["batch"], **c["opts"])[1].tolist() == [0, 0, 10, 10, 74, 74]


def test_rescore_case_layout():
    cus = 256
    case = fc.rescore_case(cus)
    n, k, turn = case["n"], case["k"], case["turn"]
    assert k == 64 and turn == cus * 32 * 256 and n == 2 * (turn // 64) + 3 and n * k > 2 * turn
    flat = np.concatenate([v[0] for v in case["slots"].values()])
    assert len(np.unique(flat)) == len(flat) and 3900 < len(flat) < 4100
    assert {turn - 1, turn} <= set(flat.tolist()) and (flat // k == n - 1).any()
    for tol, (pos, nb, pair, side) in case["slots"].items():
        a, b = case["order"][pos // k], case["order"][nb]
        assert np.array_equal(a, 2 * pair + side) and np.array_equal(b, a ^ 1)
        assert all(case["pairs"][p][4] == tol for p in pair.tolist())
    tol = 0.05
    d0, d3 = fc.rescore_expected(case, tol, 0), fc.rescore_expected(case, tol, 3)
    assert d0.dtype == np.float32 and (d0 < 1).any() and (d3 >= d0).all() and (d3 > d0).any()     # min_matches cuts some pairs
