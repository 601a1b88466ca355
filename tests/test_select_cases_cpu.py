"""The designed rows of tests/select_cases.py, checked without a GPU: the plain reference equals `fo.exhaustive_topk` on every
flat case (the two references cannot drift apart), the survivor counts of the filter cases are the designed ones, and the
model of select.h witnesses that the cases reach every branch the GPU tests are there for."""
import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import select_cases as sc

ZERO_KEY = int(sc.sortable(np.zeros(1, np.float32))[0])


@pytest.fixture(scope="module")
def flat_traces():
    """(case, row, k, trace) for the witness rows of every flat case, every k -- the staged ladder"""
    out = []
    for c in sc.flat_cases():
        S = sc.products(c.s)
        for i in sc.witness_rows(c):
            for k in sc.K_VALUES:
                out.append((c, i, k, sc.trace(S[i], k, dense=True)))
    return out


@pytest.fixture(scope="module")
def ivf_model():
    """per bucket and n_probe: candidate totals in list order, and (bucket, n_probe, row, k, trace) for a sample of queries"""
    X, off, nl = sc.ivf_vectors()
    totals, traces, own = {}, [], {}
    for b, (a, e) in enumerate(zip(off[:-1], off[1:])):
        Xb = X[a:e]
        C, asg, perm, loff = fo.ivf_build(Xb, int(nl[b]), sc.IVF_KMEANS_ITERS)
        assert np.array_equal(np.diff(loff), sc.IVF_LISTS[b])            # list i = axis i (+ the zero rows in list 0)
        for P in sc.IVF_PROBES:
            probes = fo.coarse_probe(Xb, C, min(P, int(nl[b])))
            nc = np.diff(loff)[probes].sum(1)
            totals[b, P] = nc[perm]
            own[b, P] = np.where(Xb.any(1), np.diff(loff)[asg] - (asg == 0) * sc.IVF_ZERO_ROWS, 0)[perm]
            streams = sc.ivf_streams(Xb, perm, loff, probes)
            rows = sorted({int(perm[loff[l]]) for l in range(int(nl[b]))} | {int(perm[loff[l + 1] - 1]) for l in range(int(nl[b]))}
                          | set(np.flatnonzero(~Xb.any(1)).tolist()))
            for i in rows:
                for k in sc.K_VALUES:
                    traces.append((b, P, i, k, sc.trace(streams[i][0], k, dense=False)))
    return totals, traces, own


def test_plain_reference_equals_the_oracle_on_every_flat_case():
    for cases in (sc.flat_cases(), sc.survivor_cases(False)[0], sc.survivor_cases(True)[0]):
        for c in cases:
            X = np.zeros((c.n, sc.D), np.float32)
            X[:, 0] = c.s
            rs, ri = fo.exhaustive_topk(X, sc.K_MAX, base=c.row0)
            ps, pi = sc.plain_topk(sc.products(c.s), sc.K_MAX, c.row0)
            assert np.array_equal(pi, ri), c
            assert np.array_equal(ps.view(np.uint32), rs.view(np.uint32)), c


def test_the_case_list_holds_every_size_and_pattern():
    cases = sc.flat_cases()
    assert [c.n for c in cases if c.pattern == "ascending"] == sorted(sc.ASC_SIZES, reverse=True)
    for pattern in ("descending", "all_equal", "tie_at_k", "low_bits", "mixed_sign", "exact_bin"):
        assert set(sc.OTHER_SIZES) <= {c.n for c in cases if c.pattern == pattern}, pattern
    assert {c.name for c in cases if c.pattern == "low_bits"} == {f"low_bits/{m}" for m in sc.LOW_BITS_M}
    # memory order = stable by decreasing size: the first row of the bucket behind an ascending bucket is larger everywhere
    # than anything in that bucket
    order = sorted(range(len(cases)), key=lambda j: -cases[j].n)
    for a, b in zip(order[:-1], order[1:]):
        if cases[a].pattern == "ascending":
            nxt = cases[b].s.astype(np.float64)
            assert (nxt[0] * nxt).min() > float(cases[a].s.max()) ** 2, (cases[a], cases[b])
    for c in cases:
        if c.pattern == "ascending":
            assert (np.diff(c.s) > 0).all() and c.s[0] > 0
    # k > nc, k == nc, k == nc - 1
    sizes = set(sc.ASC_SIZES)
    for rel in (-1, 0, 1):
        assert len([k for k in sc.K_VALUES if k + rel in sizes]) >= 5, rel


def test_flat_cases_reach_every_branch_of_the_first_round(flat_traces):
    def some(pattern, pred, name=None):
        hit = [(c, i, k) for c, i, k, t in flat_traces if c.pattern == pattern and (name is None or c.name == name) and pred(c, i, k, t)]
        assert hit, (pattern, name)
        return hit

    srch = lambda t: t["search"] or {"shift": None, "levels": None, "exit": None, "T": None, "first_miss": None}
    # the R classes of select_kernel's ladder, with a size on either side of every cut
    asc = {c.n: t["R"] for c, i, k, t in flat_traces if c.pattern == "ascending"}
    assert set(asc.values()) == {2, 4, 6, 8, 12, 16}
    for cut in sc.SCAN_CUTS[:-1]:
        assert asc[cut] < asc[cut + 1], cut
    chunks = {c.n: t["chunks"] for c, i, k, t in flat_traces if c.pattern == "ascending"}
    assert chunks[1024] == 0 and chunks[1025] == 1
    # no search when the round holds at most k keys
    some("ascending", lambda c, i, k, t: t["search"] is None and c.n < k)
    some("ascending", lambda c, i, k, t: t["search"] is None and c.n == k)
    some("ascending", lambda c, i, k, t: t["search"] is not None and c.n == k + 1)
    # shift: shared bits skipped / keys of both signs / all keys equal
    some("low_bits", lambda c, i, k, t: srch(t)["shift"] in range(1, 32))
    some("mixed_sign", lambda c, i, k, t: srch(t)["shift"] == 32)
    some("all_equal", lambda c, i, k, t: srch(t)["shift"] == 0 and srch(t)["exit"] == "ids" and srch(t)["levels"] == ())
    some("mixed_sign", lambda c, i, k, t: srch(t)["shift"] == 0 and c.s[i] == 0)          # an all-zero row
    # the levels: one bit; narrower than 8; exactly one full level; two levels, the second one bit wide
    some("low_bits", lambda c, i, k, t: srch(t)["levels"] == (1,), "low_bits/2")
    some("low_bits", lambda c, i, k, t: srch(t)["levels"] == (3,), "low_bits/5")
    some("low_bits", lambda c, i, k, t: srch(t)["levels"] == (8,), "low_bits/256")
    some("low_bits", lambda c, i, k, t: srch(t)["levels"] == (8, 1), "low_bits/257")
    some("low_bits", lambda c, i, k, t: srch(t)["levels"] == (8, 1), "low_bits/300")
    some("ascending", lambda c, i, k, t: srch(t)["levels"] is not None and len(srch(t)["levels"]) >= 3)
    # the k-th best of a mixed row: positive, zero, negative
    some("mixed_sign", lambda c, i, k, t: srch(t)["T"] is not None and srch(t)["T"] > ZERO_KEY)
    some("mixed_sign", lambda c, i, k, t: srch(t)["T"] == ZERO_KEY and srch(t)["exit"] == "ids" and c.s[i] != 0)
    some("mixed_sign", lambda c, i, k, t: srch(t)["T"] is not None and srch(t)["T"] < ZERO_KEY)
    # early exit at the first level for EVERY k; the neighbour misses it by one key
    hit = some("exact_bin", lambda c, i, k, t: c.s[i] == 0.5 and c.n == 1281 and srch(t)["exit"] == "exact" and srch(t)["levels"] == (8,),
               "exact_bin/hit")
    assert {k for _, _, k in hit} == set(sc.K_VALUES)
    miss = some("exact_bin", lambda c, i, k, t: c.s[i] == 0.5 and c.n == 1281 and srch(t)["first_miss"] == 1 and len(srch(t)["levels"]) > 1,
                "exact_bin/miss")
    assert len({k for _, _, k in miss}) >= 4
    # the id tie search of the first round, for several lengths of the tied run
    ties = some("tie_at_k", lambda c, i, k, t: srch(t)["exit"] == "ids" and k > min(int(c.name.split("/")[1]), c.n // 2))
    assert len({(c.name, c.n) for c, _, _ in ties}) >= 6
    some("tie_at_k", lambda c, i, k, t: srch(t)["exit"] == "exact")


def test_flat_cases_reach_every_branch_of_the_streaming(flat_traces):
    st = [(c, i, k, t) for c, i, k, t in flat_traces if t["chunks"] > 0]
    assert all(t["chunks"] == 0 for c, i, k, t in flat_traces if c.n <= 1024)
    # ascending: every chunk overflows the set and reselects; six times at 2,305 candidates
    asc = [(c, i, k, t) for c, i, k, t in st if c.pattern == "ascending"]
    assert asc and all(t["reselects"] == t["chunks"] for c, i, k, t in asc)
    assert max(t["reselects"] for c, i, k, t in asc) >= 5
    # descending: nothing streamed is kept
    desc = [t for c, i, k, t in st if c.pattern == "descending"]
    assert desc and all(t["reselects"] == 0 for t in desc)
    # a streamed row of several chunks that reselects only at the end
    assert any(t["chunks"] >= 2 and t["reselect_at"] == (t["chunks"],) for c, i, k, t in st)
    # tail chunks and streamed lengths
    assert {1, 3, 4, 255, 256} <= {t["tail"] for c, i, k, t in asc}
    assert {1, 3, 4, 255, 257, 513, 1281} <= {c.n - sc.FIRST for c, i, k, t in asc}
    # dense rule: a later key EQUAL to the threshold loses -- all_equal drops every streamed key
    eq = [t for c, i, k, t in st if c.pattern == "all_equal"]
    assert eq and all(t["equal_streamed"] == t["nc"] - sc.FIRST and t["reselects"] == 0 for t in eq)
    # streamed keys one step above the threshold (consecutive bit patterns), and the id tie search inside reselect
    assert any(c.pattern == "low_bits" and t["reselects"] > 0 for c, i, k, t in st)
    assert any(c.pattern == "tie_at_k" and t["reselect_ids"] > 0 for c, i, k, t in st)


def test_fallback_ladder_is_reached_by_the_fallback_cases():
    """the cases test_gpu_select.py sends through fused_fallback_kernel: R = 2, 4, 8, 16 with a size on either side of each cut"""
    sizes = {c.n for c in sc.flat_cases() if c.pattern in sc.FALLBACK_PATTERNS}
    assert {sc.r_class(n, sc.FALLBACK_CUTS) for n in sizes} == {2, 4, 8, 16}
    for cut in sc.FALLBACK_CUTS:
        assert {cut, cut + 1} <= sizes
    assert any(n > sc.FIRST + sc.CHUNK for n in sizes)


def test_survivor_counts_are_the_designed_ones():
    for with_rt, tol, mode, rt_tol in ((False, 0.05, "Da", None), (True, 20.0, "ppm", 10.0)):
        cases, mz, rt, queries = sc.survivor_cases(with_rt)
        assert (np.diff(mz) >= 0).all()
        sim, idx = sc.flat_reference(cases)
        nb, _ = fo.filter_neighbors(sim, idx, mz, rt, tol, mode, rt_tol, sc.K_MAX)
        cnt = (nb >= 0).sum(1)
        assert [c for c, _ in queries] == list(sc.SURVIVORS)
        for c, rows in queries:
            assert len(rows) == sc.SURVIVOR_QUERIES and (cnt[rows] == c).all(), (c, cnt[rows])
        if with_rt:                                            # the retention time removes candidates the m/z window lets through
            nb_mz, _ = fo.filter_neighbors(sim, idx, mz, None, tol, mode, None, sc.K_MAX)
            assert ((nb_mz >= 0).sum(1) > cnt).any()
    for c in sc.SURVIVORS:
        assert {x for x in (1, c - 1, c, c + 1, 256) if 1 <= x <= sc.K_MAX} <= set(sc.SURVIVOR_KEEPS)


def test_ivf_cases_reach_the_cuts_the_tie_rule_and_both_load_forms(ivf_model):
    totals, traces, own = ivf_model
    assert min(sc.IVF_PROBES) < 8 <= max(sc.IVF_PROBES)
    for cuts, probes in ((sc.SCAN_CUTS, sc.IVF_PROBES), (sc.FALLBACK_CUTS, sc.IVF_PREFILTER_PROBES)):
        nc = np.concatenate([v for (b, P), v in totals.items() if P in probes])
        assert {sc.r_class(int(x), cuts) for x in nc} == {sc.r_class(c, cuts) for c in cuts} | {16}
        for cut in cuts:
            assert (nc == cut).any() and (nc == cut + 1).any(), cut
        if cuts is sc.FALLBACK_CUTS:
            assert nc.max() <= 4096                             # the float16 list scan holds at most 4,096 keys per query
    # the prefiltered search: a query with fewer than k_ann positive similarities and more than k_ann candidates has its
    # k-th best inside the zero ties -- those are the rows ivf_fallback_kernel gets, in every R class of its ladder
    tied_nc = np.concatenate([totals[b, P][(own[b, P] < k) & (totals[b, P] > k)] for (b, P) in totals
                              if P in sc.IVF_PREFILTER_PROBES for k in sc.IVF_FALLBACK_K])
    assert {sc.r_class(int(x), sc.FALLBACK_CUTS) for x in tied_nc} == {2, 4, 8, 16}
    # both chunk load forms among the streamed rows of the staged kernel
    for P in sc.IVF_PROBES:
        per_bucket = [totals[b, P] for b in range(len(sc.IVF_LISTS))]
        wide = np.concatenate(sc.ivf_rows(per_bucket))
        streamed = np.concatenate(per_bucket) > sc.FIRST
        assert (wide & streamed).any() and (~wide & streamed).any(), P
    st = [t for b, P, i, k, t in traces if t["chunks"] > 0]
    # u >= T: streamed keys equal to the threshold stay in the race; with the k-th best inside the zero tie group every chunk
    # enters whole, the set overflows and reselect runs under ties, five times and more
    assert any(t["equal_streamed"] > 0 and t["reselects"] >= 5 and t["reselect_ids"] >= 5 for t in st)
    assert any(t["reselects"] == 0 for t in st) or any(t["reselect_at"] == (t["chunks"],) for t in st)
    # the k-th best inside the zero tie group for some rows, above it for others; first-round id search under IVF ids
    T = [(t["search"]["T"], t["search"]["exit"]) for b, P, i, k, t in traces if t["search"]]
    assert any(x == ZERO_KEY and e == "ids" for x, e in T) and any(x > ZERO_KEY for x, e in T)
    assert any(x > ZERO_KEY and e == "ids" for x, e in T)          # ties among the positive similarities too
