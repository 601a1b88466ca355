"""The designed rows of tests/prefilter_cases.py, checked without a GPU: the designs reach what they aim at (a boundary test that
misses its boundary hides the failure), and the plain references equal the oracle on every case."""
import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import prefilter_cases as pc

K_WIDE = 128


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


# --------------------------------------------------------------------------- primitives and the bound
def test_value_primitives_round_the_way_they_are_named():
    for e in pc.BOUND_EXPONENTS:
        for k in (0, 1, 5):
            lo, hi = 2.0 ** e * (1 + 2 * k * pc.U), 2.0 ** e * (1 + (2 * k + 2) * pc.U)
            assert pc.h16(pc.down(e, k)) == lo and pc.h16(pc.up(e, k)) == hi
            assert float(pc.up(e, k)) - float(pc.down(e, k)) <= 2.0 ** (e - 22)           # two float32 steps apart
    for t in (0.5, 0.84619140625, 0.29638671875):
        assert pc.h16(pc.largest_rounding_to(t)) == t == pc.h16(pc.smallest_rounding_to(t))
        two_up = np.nextafter(np.nextafter(pc.largest_rounding_to(t), np.float32(1)), np.float32(1))      # (past a tie to even)
        two_down = np.nextafter(np.nextafter(pc.smallest_rounding_to(t), np.float32(0)), np.float32(0))
        assert pc.h16(two_up) > t > pc.h16(two_down)
    assert (pc.h16(pc.EXACT16) == np.asarray(pc.EXACT16, np.float64)).all()
    sub = pc.h16(pc.SUBNORMAL)
    assert ((sub > 0) & (sub < 2.0 ** -14)).all() and (pc.h16(pc.FLUSHED) == 0).all()


def test_bound_rows_put_the_error_at_three_quarters_of_the_bound():
    X, names = pc.bound_rows(pc.D)
    E = pc.exact_sims(X).astype(np.float64)
    A, single = pc.approx_sims(X)
    assert single.all() and E.max() <= 1.0
    r = pc.bound_ratio(A, E)
    rk = pc.bound_ratio(pc.key_of(A) / 65535.0, E, keyed=True)
    i = names.index("down-1")
    print(f"model: max ratio {r.max():.4f} (down-1 x down-1 {r[i, i]:.4f}), keyed {rk.max():.4f}")
    assert 0.74 <= r.max() < 1.0 and 0.74 <= r[i, i]
    assert 0.70 <= rk.max() < 1.0
    # subnormal factors: kept, the error stays inside the absolute term
    s = [j for j, n in enumerate(names) if n in ("sub", "flushed")]
    assert (np.abs(A - E)[s].max() <= 2.0 ** -25) and r[s].max() < 1.0
    assert (A[s] > 0).any()


def test_two_term_chain_emulation_equals_the_compiled_chain():
    """query-query pairs are two-term sums: the float64 emulation of the fmaf chain is exact for components in [0.25, 0.71]"""
    for ec in pc.FLAT_INV_EXPONENTS:
        X, mz, q, xs, ys = pc.flat_inversion(ec)
        Q = X[q]
        assert ((Q[:, :2] >= 0.25) & (Q[:, :2] <= 0.71)).all() and (np.linalg.norm(Q.astype(np.float64), axis=1) <= 1).all()
        if fo.have_kordered():
            assert np.array_equal(pc.exact_sims(X).view(np.uint32), fo.sims_f32(X, X).view(np.uint32))
    b = pc.ivf_bucket(pc.IVF_RUNS[0])
    if fo.have_kordered():
        assert np.array_equal(pc.exact_sims(b["X"]).view(np.uint32), fo.sims_f32(b["X"], b["X"]).view(np.uint32))


# --------------------------------------------------------------------------- flat buckets
@pytest.mark.parametrize("ec", pc.FLAT_INV_EXPONENTS)
def test_flat_inversion_reverses_the_order_across_the_kth_place(ec):
    X, mz, q, xs, ys = pc.flat_inversion(ec)
    k = pc.FLAT_INV_K
    assert len(X) > k and (np.diff(mz) >= 0).all()
    E = pc.exact_sims(X)
    assert E.max() <= 1.0
    A, single = pc.approx_sims(X)
    es, ei = pc.plain_topk(E, k)
    _, ai = pc.plain_topk(A.astype(np.float32), k)
    far = np.abs(A[q][:, q] / A[q][:, xs[:1]] - 1).min()                       # the two-term pairs lie far above the k-th place
    assert far > 0.5
    for i in q:
        assert set(xs[:2]) <= set(ei[i]) and not set(ys) & set(ei[i]) and xs[2] not in ei[i]
        assert set(ys[:2]) <= set(ai[i]) and not set(xs) & set(ai[i])
        assert ei[i, k - 1] == xs[1] and ai[i, k - 1] == ys[1]
        # both orders strict, the error near its maximum: exact X / Y - 1 ~ +2 u, approx ~ -2 u
        assert E[i, xs[0]] > E[i, ys[0]] and A[i, xs[0]] < A[i, ys[0]]
        assert pc.bound_ratio(A[i, xs[0]], E[i, xs[0]]) > 0.7 and pc.bound_ratio(A[i, ys[0]], E[i, ys[0]]) > 0.7
        # trusting the approximate order changes the neighbour list: the window holds exactly Q, X, Y
        win = np.flatnonzero(np.abs(mz.astype(np.float64) - float(mz[i])) <= pc.TOL_DA)
        assert set(win) == set(q) | set(xs) | set(ys)
    assert _same(pc.plain_topk(E, k), fo.exhaustive_topk(X, k))
    nb_e, _ = fo.filter_neighbors(es, ei, mz, None, pc.TOL_DA, "Da", None, 16)
    nb_a, _ = fo.filter_neighbors(es, ai, mz, None, pc.TOL_DA, "Da", None, 16)
    assert (nb_e[q] != nb_a[q]).any(1).all()
    # the designed queries stay on chip (X and Y are members, settled by resolve_kernel); the rows whose k-th best lies among
    # the zeros -- the column-1 rows, with fewer than k positive similarities -- overflow the member lists
    over, _ = pc.flat_overflow_model(X, k)
    assert not over[q].any() and set(np.flatnonzero(over)) == set(np.flatnonzero((E > 0).sum(1) < k))


def test_flat_collapse_fills_and_overflows_the_member_list_of_each_half():
    for run, half in pc.FLAT_RUNS:
        X, mz, k, rows, _ = pc.flat_collapse(run, half, None)
        assert len(np.unique(X[rows, 0])) == run and (pc.h16(X[rows, 0]) == 0.5).all()
        assert (((rows >> 2) & 1) == half).all()
        A, _ = pc.approx_sims(X)
        for i in (0, int(rows[0]), len(X) - 1):
            bstar, m0, m1, T, _, bins = pc.fused_members(A[i], k, np.arange(len(X)))
            assert (m0, m1)[half] == run and (m0, m1)[1 - half] == 0              # the run alone, in the intended half
            assert T == pc.h16(X[i, 0]) * 0.5                                     # the k-th place lies inside the run
        over, dist = pc.flat_overflow_model(X, k)
        assert over.all() if run > pc.FUSED_MEM_HALF else not over.any()
        assert dist > 2e-7
        E = pc.exact_sims(X)
        assert E.max() <= 1.0 and _same(pc.plain_topk(E, K_WIDE), fo.exhaustive_topk(X, K_WIDE))


def test_flat_edge_candidate_sits_at_the_edge_of_the_widened_bin():
    b = pc.bin_of(np.float32(0.25))
    lo, hi = pc.fused_window(b)
    for edge, inside in (("in", True), ("out", False)):
        X, mz, k, rows, val = pc.flat_collapse(pc.FUSED_MEM_HALF, 0, edge)
        v = float(pc.h16(val) * 0.5)
        gap = float(hi) - v
        assert (pc.FLAT_EDGE_MARGIN <= gap < 2.5e-4) if inside else (pc.FLAT_EDGE_MARGIN <= -gap < 2.5e-4)
        over, dist = pc.flat_overflow_model(X, k)
        assert over[rows].all() == inside and over[rows].any() == inside         # the run rows are the queries it is designed for
        assert dist > 2e-7
        # with 0.9e-3 in place of 1.3e-3 the inside candidate would be outside
        assert not pc.flat_overflow_model(X, k, 0.9e-3)[0][rows].any()
        assert _same(pc.plain_topk(pc.exact_sims(X), K_WIDE), fo.exhaustive_topk(X, K_WIDE))


def test_flat_keep_fills_and_overflows_the_kept_window_candidates_of_a_half():
    for h in pc.FLAT_KEEP_HIGH:
        X, mz, k = pc.flat_keep(h)
        over, dist = pc.flat_overflow_model(X, k)
        assert not over.any() and dist > 2e-7                                   # the member lists hold: 20 in half 0
        kept = pc.flat_kept_model(X, k, mz)
        assert kept[:, 0].max() == pc.FUSED_MEM_HALF + h and kept[:, 1].max() == pc.FLAT_COL_HIGH - h
        assert (kept.max(1) > pc.FLAT_KEEP_HALF).any() == (pc.FUSED_MEM_HALF + h > pc.FLAT_KEEP_HALF)
        # more than 16 survivors in every window: the filter's wider sort forms
        es, ei = pc.plain_topk(pc.exact_sims(X), k)
        nb, _ = fo.filter_neighbors(es, ei, mz, None, pc.TOL_DA, "Da", None, 64)
        assert ((nb >= 0).sum(1) >= k - 1).all() and k - 1 > 32                  # (k when the query is not among its own k best)
        assert _same(pc.plain_topk(pc.exact_sims(X), K_WIDE), fo.exhaustive_topk(X, K_WIDE))
    assert [pc.FUSED_MEM_HALF + h - pc.FLAT_KEEP_HALF for h in pc.FLAT_KEEP_HIGH] == [-1, 0, 1]


@pytest.mark.parametrize("c", pc.FLAT_SURVIVORS)
def test_flat_survivors_stand_at_the_rank_or_sort_cut_on_collapsed_values(c):
    X, mz, k, q = pc.flat_survivors(c)
    assert (np.diff(mz) >= 0).all() and len(q) == 30 - c
    E = pc.exact_sims(X)
    es, ei = pc.plain_topk(E, k)
    nb, _ = fo.filter_neighbors(es, ei, mz, None, pc.TOL_DA, "Da", None, 64)
    cnt = (nb >= 0).sum(1)
    run = np.flatnonzero(pc.h16(X[:, 0]) == 0.5)
    win = np.flatnonzero(mz == np.float32(500.0))
    assert len(run) == pc.FUSED_MEM_HALF and set(run) <= set(win) and len(win) == 40
    assert (cnt[q] == c).all()                                                  # the designed queries
    assert set(cnt[win]) == {c - 1, c} and (cnt[np.setdiff1d(np.arange(len(X)), win)] == 0).all()
    for i in q:                                                                 # ten of the twenty collapsed rows survive, ten do not
        assert len(set(nb[i]) & set(run)) == pc.FLAT_SURVIVOR_RUN_IN
        A, _ = pc.approx_sims(X[i:i + 1], X[run])
        assert len(np.unique(A)) == 1 and len(np.unique(E[i, run])) == len(run)
    # nothing overflows: the lists are written by resolve_kernel, not by the exact fallback
    over, dist = pc.flat_overflow_model(X, k)
    kept = pc.flat_kept_model(X, k, mz)
    assert not over.any() and dist > 2e-7 and kept.max() <= pc.FUSED_MEM_HALF
    assert _same(pc.plain_topk(E, K_WIDE), fo.exhaustive_topk(X, K_WIDE))


# --------------------------------------------------------------------------- IVF buckets
@pytest.fixture(scope="module")
def ivf():
    out = {}
    for run in pc.IVF_RUNS:
        b = pc.ivf_bucket(run)
        C, asg, perm, loff = fo.ivf_build(b["X"], pc.IVF_NLIST, 0)
        probes = fo.coarse_probe(b["X"], C, pc.IVF_NPROBE)
        out[run] = (b, C, asg, perm, loff, probes)
    return out


def test_ivf_bucket_has_the_lists_the_design_assumes(ivf):
    for run, (b, C, asg, perm, loff, probes) in ivf.items():
        X, kind = b["X"], b["kind"]
        one = (X != 0).sum(1) == 1
        assert np.array_equal(asg[one], np.argmax(X[one] != 0, 1))              # list c = axis c
        two = np.flatnonzero(~one)
        assert len(two) == 5 and set(asg[two]) <= {0, 1}
        sizes = np.diff(loff)
        assert tuple(sizes) == pc.IVF_LISTS                                      # 1, 31, 32, 33, 97, 127, 128, 129 rows
        own = fo.coarse_probe(X, C, 1)[:, 0]                                     # n_probe 1: a list is probed by its own rows
        assert np.array_equal(own, asg) and {1, 32, 33, 97} <= set(np.bincount(own))
        for i in two:
            assert set(probes[i]) == {0, 1}
        assert (np.diff(b["mz"]) >= 0).all()
        E = pc.exact_sims(X)
        assert E.max() <= 1.0


def test_ivf_edge_rows_stay_on_their_side_of_delta_and_fill_the_member_room(ivf):
    T = int(pc.key_of(0.25))
    for run, (b, C, asg, perm, loff, probes) in ivf.items():
        X, kind = b["X"], b["kind"]
        ks = pc.ivf_k_values(b, perm, loff, probes)
        A, _ = pc.approx_sims(X)
        K = pc.key_of(A)
        qe = np.flatnonzero(kind == "Qedge")
        edge = np.flatnonzero(kind == "edge")
        delta, _ = pc.key_delta(T)
        assert b["delta"] == delta == 50
        for i in qe:
            df = np.sort(K[i, edge] - T)
            assert list(df) == [-delta - 2, -delta + 2, delta - 2, delta + 2], df
            for off in (-1, 0, 1):                                              # the key model is trusted to one unit
                inside = np.abs(df + off) <= delta
                assert list(inside) == [False, True, True, False]
        m = pc.ivf_model(X, perm, loff, probes, ks["edge"])
        assert (m[qe, 1] == T).all() and (m[qe, 3] == run + 4).all(), m[qe]      # 39, 40, 41 members
        qi = np.flatnonzero(kind == "Qinv")
        m = pc.ivf_model(X, perm, loff, probes, ks["collapse"])
        assert (m[qi, 1] == T).all() and (m[qi, 3] == run + 6).all(), m[qi]
        # a delta from 0.9e-3 would leave the rows at delta - 2 outside: the run and X, no overflow for any run length
        m9 = pc.ivf_model(X, perm, loff, probes, ks["edge"], 0.9e-3)
        assert (m9[qe, 3] == run + 2).all() and run + 2 <= pc.IVF_MEM
        # ceil() in delta: the product is not near an integer, so a fused multiply-add gives the same delta
        e = np.float64(pc.REL) * (T / 65535.0) + pc.ABS_KEY
        assert 0.01 < (e * 65535.0) % 1 < 0.99


def test_ivf_inversion_reverses_the_order_across_the_kth_place(ivf):
    for run, (b, C, asg, perm, loff, probes) in ivf.items():
        X, kind = b["X"], b["kind"]
        k = pc.ivf_k_values(b, perm, loff, probes)["inversion"]
        E = pc.exact_sims(X)
        A, _ = pc.approx_sims(X)
        xs, ys = np.flatnonzero(kind == "X"), np.flatnonzero(kind == "Y")
        for i in np.flatnonzero(kind == "Qinv"):
            cand = np.concatenate([perm[loff[l]:loff[l + 1]] for l in probes[i]])
            _, ei = pc.plain_topk(E[i:i + 1, cand], k)
            _, ai = pc.plain_topk(A[i:i + 1, cand].astype(np.float32), k)
            ei, ai = cand[ei[0]], cand[ai[0]]
            assert ei[k - 1] == xs[0] and ai[k - 1] == ys[0]
            assert not set(ys) & set(ei) and not set(xs) & set(ai)
            assert set(xs) | set(ys) <= set(b["block"])                          # all four inside the query's window
        rs, ri = fo.ivf_search(X, C, asg, perm, loff, pc.IVF_NPROBE, k)
        for i in np.flatnonzero(kind == "Qinv"):
            assert ri[i, k - 1] == xs[0]


# --------------------------------------------------------------------------- assignment and coarse quantiser
def test_close_pairs_lie_where_the_threshold_decides():
    for name, g_lo, g_hi, inv, _ in pc.ASSIGN_TYPES:
        x0, x1, ca, cb, g, ea, eb = pc.close_pair(g_lo, g_hi, inv)
        assert g_lo < g < g_hi and (ea > eb) == inv
        assert float(x0) ** 2 + float(x1) ** 2 <= 1 and float(ea) <= 1 and float(eb) <= 1
        aa, ab = pc.h16(x0) * pc.h16(ca), pc.h16(x1) * pc.h16(cb)
        assert ab > aa                                                          # the approximate winner is b
        if inv:
            # beyond 1.0 eps (a threshold of 1.0 eps would trust the wrong winner), inside 2.2 eps, by 5 % and more
            assert 1.05 < (ab - aa) / (pc.REL * ab + pc.ABS) < 2.1 and (float(ea) - float(eb)) / float(ea) > 1e-4


@pytest.mark.parametrize("n_list", pc.ASSIGN_NLIST)
def test_assignment_rows_have_the_approximate_winner_wrong(n_list):
    X, ids, axis = pc.assign_bucket(n_list)
    n = len(X)
    seeds = (np.arange(n_list, dtype=np.int64) * n) // n_list
    C = X[seeds]
    assert np.array_equal(np.argmax(C != 0, 1), axis) and ((C != 0).sum(1) == 1).all()
    E = pc.exact_sims(X, C)
    assert E.max() <= 1.0 and (np.linalg.norm(X.astype(np.float64), axis=1) <= 1.0).all()       # so no row pair exceeds 1 either
    A, single = pc.approx_sims(X, C)
    assert single.all()
    exact = np.argmax(E, 1)                                                     # ties -> lowest id
    assert np.array_equal(exact, fo.kmeans_assign(X, C))
    approx = np.argmax(A, 1)
    for name in ("inverted", "same_group", "many"):
        r = ids[name]
        assert (approx[r] != exact[r]).all() and (axis[approx[r]] == axis[exact[r]] + 1).all(), name
    r = ids["same_group"]
    assert (approx[r] // 32 == exact[r] // 32).all()
    r = ids["inverted"]
    assert (approx[r] // 32 != exact[r] // 32).all() and (n_list <= 128 or (approx[r] // 128 != exact[r] // 128).all())
    r = ids["many"]
    thr = A[r].max(1) - 2.2 * (pc.REL * A[r].max(1) + pc.ABS)
    assert ((A[r] >= thr[:, None]).sum(1) > 4).all()
    for name, lo, hi in (("inside", 2.12, 2.19), ("outside", 2.21, 2.28)):       # within 4 % of 2.2, on either side
        r = ids[name]
        top = np.sort(A[r], 1)[:, ::-1]
        g = (top[:, 0] - top[:, 1]) / (pc.REL * top[:, 0] + pc.ABS)
        assert ((g > lo) & (g < hi)).all(), (name, g[:3])
        assert (approx[r] == exact[r]).all()
    # coarse quantiser: third and fourth list inverted; 15, 16, 17 equal keys
    r = ids["probe3"]
    e3 = fo.coarse_probe(X[r], C, 3)
    a3 = pc.plain_topk(A[r].astype(np.float32), 3)[1]
    assert np.array_equal(np.sort(e3[:, :2], 1), np.sort(a3[:, :2], 1))
    assert (np.array([len(set(a) ^ set(b)) for a, b in zip(e3, a3)]) == 2).all()
    K = pc.key_of(A)
    members = set()
    for i in ids["copy"]:
        T = np.sort(K[i])[::-1][2]
        delta, _ = pc.key_delta(int(T))
        members.add(int((np.abs(K[i] - T) <= delta).sum()))
    assert set(pc.PROBE_REPEATS) <= members and max(pc.PROBE_REPEATS) > pc.COARSE_MEM >= min(pc.PROBE_REPEATS) + 1
    # the plain reference of the probes: plain_topk over the closed-form similarities
    assert np.array_equal(pc.plain_topk(E, 3)[1], fo.coarse_probe(X, C, 3))
    C2, asg, perm, loff = fo.ivf_build(X, n_list, 0)
    assert np.array_equal(C2, C) and np.array_equal(asg, exact)
