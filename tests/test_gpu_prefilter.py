"""The float16 prefilters on rows built to maximise their rounding error at a decision (tests/prefilter_cases.py): index,
similarities, ids and neighbour lists bit for bit against plain references -- `plain_topk` over closed-form exact similarities
for flat buckets, the oracle's index and search for buckets with lists -- and the fallback counter against the model's member
counts.  tests/test_prefilter_cases_cpu.py shows that every design reaches the boundary it aims at."""
import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import prefilter_cases as pc

pytestmark = pytest.mark.gpu

KEEPS = (16, 2)


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.tdev)


def _half(Xd):
    import torch
    return Xd.to(torch.float16).contiguous()


def _same_topk(sim, idx, rs, ri, what):
    sim, idx = sim.cpu().numpy(), idx.cpu().numpy()
    bad = np.flatnonzero((idx != ri).any(1) | (sim.view(np.uint32) != rs.view(np.uint32)).any(1))
    if len(bad):
        r = int(bad[0])
        j = int(np.flatnonzero((idx[r] != ri[r]) | (sim[r].view(np.uint32) != rs[r].view(np.uint32)))[0])
        lo = max(j - 2, 0)
        raise AssertionError(f"{what}: {len(bad)} rows differ, first row {r} at rank {j}: got ids {idx[r, lo:j + 3]} sims "
                             f"{sim[r, lo:j + 3]}, expected ids {ri[r, lo:j + 3]} sims {rs[r, lo:j + 3]}; rows {bad[:12]}")


def _same_neighbours(got, cnt, rs, ri, mz, keep, what):
    """neighbour lists == the CPU filter of the reference top-k; the stored counts too"""
    g_idx, g_dist = (t.cpu().numpy() for t in got)
    e_idx, e_dist = fo.filter_neighbors(rs, ri, mz, None, pc.TOL_DA, "Da", None, keep)
    bad = np.flatnonzero((g_idx != e_idx).any(1) | (g_dist.view(np.uint32) != e_dist.view(np.uint32)).any(1))
    if len(bad):
        r = int(bad[0])
        raise AssertionError(f"{what} keep {keep}: {len(bad)} rows differ, first row {r}: got {g_idx[r, :8]} {g_dist[r, :8]}, "
                             f"expected {e_idx[r, :8]} {e_dist[r, :8]}; rows {bad[:12]}")
    if cnt is not None:
        assert np.array_equal(cnt.cpu().numpy(), (e_idx >= 0).sum(1)), what
    return e_idx


def _every_path(ctx, plain, pre, n_probe, k, mz, rs, ri, what):
    """the prefiltered search, the staged search + filter and the fused filter of the staged select -> fallback queries of the
    prefiltered search (largest keep)"""
    mz_d = _dev(ctx, mz)
    n_fb = None
    for keep in KEEPS:
        got = pre.search_neighbors(n_probe, k, mz_d, None, pc.TOL_DA, "Da", None, keep)
        ctx.sync()
        n_fb = ctx.counter(5) if n_fb is None else n_fb
        _same_neighbours(got, pre.nb_count, rs, ri, mz, keep, what + " prefilter")
    sim, idx = plain.search(n_probe, k)
    _same_topk(sim, idx, rs, ri, what + " staged")
    for keep in KEEPS:
        _same_neighbours(ctx.filter_neighbors(sim, idx, mz_d, None, pc.TOL_DA, "Da", None, keep), None, rs, ri, mz, keep,
                         what + " staged filter")
        got = plain.search_neighbors(n_probe, k, mz_d, None, pc.TOL_DA, "Da", None, keep)
        _same_neighbours(got, plain.nb_count, rs, ri, mz, keep, what + " staged fused filter")
    return n_fb


# --------------------------------------------------------------------------- bound: the f16 flat scan against the model
@pytest.mark.parametrize("d,planes", [(64, 1), (64, 2), (400, 1), (400, 2), (800, 1)])
def test_f16_flat_scan_returns_the_modelled_products_subnormal_factors_kept(ctx, d, planes):
    """Every pair of `bound_rows` is one product.  One plane: the scan returns float16(a) * float16(b) bit for bit -- for factors
    in float16's subnormal range too: the matrix cores keep them (a flushed factor would return 0) -- and the error against the
    exact product reaches 0.7466 of the bound and stays below it.  Two planes (hi + lo / 2048): hi hi + (hi lo + lo hi) / 2048
    within two float32 roundings, with subnormal `lo` values kept as well."""
    import torch
    X, names = pc.bound_rows(d)
    n = len(X)
    if planes == 1:
        X16 = torch.from_numpy(X.astype(np.float16)).to(ctx.tdev)
    else:
        hi = X.astype(np.float16)
        lo = ((X - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
        X16 = torch.from_numpy(np.ascontiguousarray(np.stack([hi, lo], 1))).to(ctx.tdev)
    index = ctx.ivf_build(None, np.array([0, n]), np.ones(1, np.int32), X16=X16)
    sim, idx = index.search(1, 128)                                              # 128 > n: every pair comes back
    sim, idx = sim.cpu().numpy(), idx.cpu().numpy()
    assert ((idx >= 0).sum(1) == n).all()
    S = np.zeros((n, n), np.float32)
    np.put_along_axis(S, idx[:, :n].astype(np.int64), sim[:, :n], 1)
    E = pc.exact_sims(X).astype(np.float64)
    sub = np.array([nm in ("sub", "flushed") for nm in names])
    if planes == 1:
        A, single = pc.approx_sims(X)
        assert single.all()
        bad = np.argwhere(S.view(np.uint32) != A.astype(np.float32).view(np.uint32))
        assert len(bad) == 0, (len(bad), [(names[i], names[j], S[i, j], A[i, j]) for i, j in bad[:6]])
        assert (S[sub][:, sub] > 0).any()                                        # products of two subnormal factors, not zero
        ratio = pc.bound_ratio(S, E)
        i = names.index("down-1")
        print(f"d {d}: measured max ratio {ratio.max():.4f}, down-1 x down-1 {ratio[i, i]:.4f}, subnormal rows {ratio[sub].max():.4f}")
        assert 0.74 <= ratio.max() < 1.0
    else:
        H, L = hi.astype(np.float64), lo.astype(np.float64)
        M = H @ H.T + (H @ L.T + L @ H.T) / 2048.0
        err = np.abs(S.astype(np.float64) - M)
        assert (err <= 2.0 ** -22 * np.abs(M)).all(), float((err / np.maximum(np.abs(M), 1e-300)).max())
        assert (np.abs(L[sub]) > 0).any() and (np.abs(L[sub][L[sub] != 0]) < 2.0 ** -14).any()      # subnormal lo values occur
        ratio = pc.bound_ratio(np.abs(S), E)
        print(f"d {d}, two planes: measured max ratio {ratio.max():.4f}")
        assert ratio.max() < 1.0
    index.close()


# --------------------------------------------------------------------------- flat buckets through fused.hip
@pytest.fixture(scope="module")
def flat_inv(ctx):
    parts = [pc.flat_inversion(ec) for ec in pc.FLAT_INV_EXPONENTS]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
    X = np.concatenate([p[0] for p in parts])
    mz = np.concatenate([p[1] + np.float32(20 * b) for b, p in enumerate(parts)]).astype(np.float32)
    Xd = _dev(ctx, X)
    nl = np.ones(len(parts), np.int32)
    plain = ctx.ivf_build(Xd, off, nl)
    pre = ctx.ivf_build(Xd, off, nl, Xpre=_half(Xd))
    assert ctx.counter(6) == 0
    ref = [pc.plain_topk(pc.exact_sims(p[0]), pc.FLAT_INV_K, int(off[b])) for b, p in enumerate(parts)]
    return plain, pre, mz, np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref]), off, parts


def test_flat_prefilter_with_the_order_reversed_across_the_kth_place(ctx, flat_inv):
    """`flat_inversion`: the approximate k_ann-th best is a Y row, the exact one an X row, both in the query's window"""
    plain, pre, mz, rs, ri, off, parts = flat_inv
    n_fb = _every_path(ctx, plain, pre, 16, pc.FLAT_INV_K, mz, rs, ri, "flat inversion")
    e_idx, _ = fo.filter_neighbors(rs, ri, mz, None, pc.TOL_DA, "Da", None, 16)
    for b, (X, _, q, xs, ys) in enumerate(parts):
        for i in q + off[b]:
            assert set(xs[:2] + off[b]) <= set(e_idx[i]) and not set(ys + off[b]) & set(e_idx[i])
    model = sum(int(pc.flat_overflow_model(p[0], pc.FLAT_INV_K)[0].sum()) for p in parts)
    print(f"flat inversion: fallback queries {n_fb}, model {model} of {len(mz)}")
    assert n_fb == model                                                         # the designed queries were settled on chip
    assert ctx.counter(6) == 0


_FLAT_COLLAPSE = [(run, half, None) for run, half in pc.FLAT_RUNS] + [(pc.FUSED_MEM_HALF, 0, "in"), (pc.FUSED_MEM_HALF, 0, "out")]


@pytest.mark.parametrize("run,half,edge", _FLAT_COLLAPSE, ids=[f"{r}-half{h}-{e or 'run'}" for r, h, e in _FLAT_COLLAPSE])
def test_flat_prefilter_on_collapsed_runs_at_the_member_capacity(ctx, run, half, edge):
    """`flat_collapse`: `run` distinct exact values on one float16 value around the k_ann-th place.  20 fill approx_kernel's
    member list of a lane half, 21 overflow it: the exact fallback runs for exactly the queries the model names (every row / no
    row), and for the run's own rows when one more candidate lies just inside the widened threshold bin."""
    X, mz, k, rows, _ = pc.flat_collapse(run, half, edge)
    off, nl = np.array([0, len(X)], np.int64), np.ones(1, np.int32)
    Xd = _dev(ctx, X)
    plain = ctx.ivf_build(Xd, off, nl)
    pre = ctx.ivf_build(Xd, off, nl, Xpre=_half(Xd))
    assert ctx.counter(6) == 0
    rs, ri = pc.plain_topk(pc.exact_sims(X), k)
    n_fb = _every_path(ctx, plain, pre, 16, k, mz, rs, ri, f"flat collapse {run}/{half}/{edge}")
    over, _ = pc.flat_overflow_model(X, k)
    print(f"run {run} half {half} edge {edge}: fallback queries {n_fb}, model {int(over.sum())} of {len(X)}")
    assert n_fb == int(over.sum())
    plain.close(), pre.close()


@pytest.mark.parametrize("high_in_half", pc.FLAT_KEEP_HIGH)
def test_flat_prefilter_at_the_kept_window_capacity(ctx, high_in_half):
    """`flat_keep`: the whole bucket is one precursor window; band_kernel keeps 31, 32, 33 window candidates in lane half 0
    (it holds 32): the exact fallback takes exactly the queries the model names; 33 or 34 survivors per query for the filter"""
    X, mz, k = pc.flat_keep(high_in_half)
    off, nl = np.array([0, len(X)], np.int64), np.ones(1, np.int32)
    Xd = _dev(ctx, X)
    plain = ctx.ivf_build(Xd, off, nl)
    pre = ctx.ivf_build(Xd, off, nl, Xpre=_half(Xd))
    assert ctx.counter(6) == 0
    rs, ri = pc.plain_topk(pc.exact_sims(X), k)
    mz_d = _dev(ctx, mz)
    for keep in (64, 16):
        got = pre.search_neighbors(16, k, mz_d, None, pc.TOL_DA, "Da", None, keep)
        ctx.sync()
        n_fb = ctx.counter(5)
        _same_neighbours(got, pre.nb_count, rs, ri, mz, keep, f"flat keep {high_in_half}")
        got = plain.search_neighbors(16, k, mz_d, None, pc.TOL_DA, "Da", None, keep)
        _same_neighbours(got, plain.nb_count, rs, ri, mz, keep, f"flat keep {high_in_half} staged")
    over = pc.flat_kept_model(X, k, mz).max(1) > pc.FLAT_KEEP_HALF
    print(f"high rows in half 0 {high_in_half}: fallback queries {n_fb}, model {int(over.sum())} of {len(X)}")
    assert n_fb == int(over.sum()) and over.any() == (high_in_half == max(pc.FLAT_KEEP_HIGH))
    plain.close(), pre.close()


@pytest.mark.parametrize("c", pc.FLAT_SURVIVORS)
def test_flat_prefilter_with_15_16_17_survivors_on_collapsed_values(ctx, c):
    """`flat_survivors`: one precursor window holds a run of twenty values on ONE float16 value with the k_ann-th place in its
    middle; exactly c candidates of a designed query survive the filter -- ten of the run, picked by their exact values, and
    c - 10 high rows.  resolve_kernel ranks up to 16 survivors and sorts 17; nothing overflows, so no query takes the fallback."""
    X, mz, k, q = pc.flat_survivors(c)
    off, nl = np.array([0, len(X)], np.int64), np.ones(1, np.int32)
    Xd = _dev(ctx, X)
    plain = ctx.ivf_build(Xd, off, nl)
    pre = ctx.ivf_build(Xd, off, nl, Xpre=_half(Xd))
    assert ctx.counter(6) == 0
    rs, ri = pc.plain_topk(pc.exact_sims(X), k)
    n_fb = _every_path(ctx, plain, pre, 16, k, mz, rs, ri, f"flat survivors {c}")
    mz_d = _dev(ctx, mz)
    for keep in (64, c, c - 1):
        got = pre.search_neighbors(16, k, mz_d, None, pc.TOL_DA, "Da", None, keep)
        ctx.sync()
        n_fb += ctx.counter(5)
        e_idx = _same_neighbours(got, pre.nb_count, rs, ri, mz, keep, f"flat survivors {c}")
        assert ((e_idx[q] >= 0).sum(1) == min(c, keep)).all()
    print(f"survivors {c}: fallback queries {n_fb} of {len(X)}")
    assert n_fb == 0
    plain.close(), pre.close()


# --------------------------------------------------------------------------- buckets with lists through ivf16.hip
_FORMS = {"list16s": (64, False, None), "dense_800": (800, False, None), "dense_wide_row": (128, True, None),
          "list16r": (64, False, "r")}


@pytest.mark.parametrize("form", list(_FORMS))
@pytest.mark.parametrize("run", pc.IVF_RUNS)
def test_ivf_prefilter_at_inversion_collapse_and_edge(ctx, monkeypatch, run, form):
    """`ivf_bucket` through every form of the float16 list scan (sparse query records, the dense gather at 800 columns and with
    a row of more than 64 non-zeros, FALCON_LIST16=r), lists of 1, 31, 32, 33, 97, 127, 128 and 129 rows:
      inversion  the approximate k_ann-th best is Y, the exact one X;
      collapse   k_ann ends inside `run` candidates with ONE key; with X, Y and the edge rows 41 to 43 keys within delta;
      edge       two keys at delta - 2 and two at delta + 2 around the run's key: 39, 40, 41 members for run = 35, 36, 37 --
                 select16 holds 40, so the exact fallback takes the edge queries at 37 and not below.
    Index == the oracle's, searches == the oracle's on it, fallback queries == the model's count."""
    d, wide, env = _FORMS[form]
    if env:
        monkeypatch.setenv("FALCON_LIST16", env)
    b = pc.ivf_bucket(run, d, wide)
    X, mz = b["X"], b["mz"]
    off, nl = np.array([0, len(X)], np.int64), np.array([pc.IVF_NLIST], np.int32)
    Xd = _dev(ctx, X)
    x16 = _half(Xd)
    # (the exact float32 assignment kernels end at 512 columns: at 800 the staged index is built with the float16 assignment too)
    plain = ctx.ivf_build(Xd, off, nl, kmeans_iters=0, Xkm=x16 if d > 512 else None)
    pre = ctx.ivf_build(Xd, off, nl, kmeans_iters=0, Xkm=x16, Xpre=x16, prefilter_which=2)
    assert ctx.counter(6) == 0
    C, asg, perm, loff = fo.ivf_build(X, pc.IVF_NLIST, 0)
    for index in (plain, pre):
        for got, want in zip(index.export(), (C, asg, perm, loff)):
            assert np.array_equal(got.cpu().numpy(), want)
    probes = fo.coarse_probe(X, C, pc.IVF_NPROBE)
    fb = {}
    for name, k in pc.ivf_k_values(b, perm, loff, probes).items():
        rs, ri = fo.ivf_search(X, C, asg, perm, loff, pc.IVF_NPROBE, k)
        fb[name] = _every_path(ctx, plain, pre, pc.IVF_NPROBE, k, mz, rs, ri, f"ivf {form} run {run} {name}")
        m = pc.ivf_model(X, perm, loff, probes, k)
        over = (m[:, 1] >= 0) & (m[:, 3] > pc.IVF_MEM)
        qe, qi = b["kind"] == "Qedge", b["kind"] == "Qinv"
        print(f"{form} run {run} {name} k {k}: fallback queries {fb[name]}, model {int(over.sum())} of {len(X)}; "
              f"edge queries over {int(over[qe].sum())}, inversion queries over {int(over[qi].sum())}")
        if name == "edge":
            assert over[qe].all() == (run + 4 > pc.IVF_MEM) == over[qe].any()
        assert fb[name] == int(over.sum()), (name, fb[name], int(over.sum()))
    # n_probe 1: every list is probed by its own rows alone (1, 31, 32, 33, 97, 127, 128, 129 queries per list); the run
    # collapses for the queries of list 0
    own = fo.coarse_probe(X, C, 1)
    rs, ri = fo.ivf_search(X, C, asg, perm, loff, 1, 24)
    n_fb = _every_path(ctx, plain, pre, 1, 24, mz, rs, ri, f"ivf {form} run {run} n_probe 1")
    m = pc.ivf_model(X, perm, loff, own, 24)
    assert n_fb == int(((m[:, 1] >= 0) & (m[:, 3] > pc.IVF_MEM)).sum())
    assert ctx.counter(6) == 0
    plain.close(), pre.close()


# --------------------------------------------------------------------------- k-means assignment and coarse quantiser
@pytest.mark.parametrize("n_list", pc.ASSIGN_NLIST)
def test_float16_assignment_and_keyed_quantiser_on_close_centroids(ctx, n_list):
    """`assign_bucket`: rows whose best and runner-up centroid come out in the opposite order in float16 (in two 32-centroid
    groups, in one, with more than four contenders), rows with the runner-up 4 % inside / outside best - 2.2 eps; up to 128
    lists, merged partials, list counts that are no multiple of 128.  The keyed build == the exact build == the oracle's index.
    The search through the keys (n_probe 1, 3 and, with 128 lists, every list) == the oracle's on that index: queries whose
    third and fourth list are inverted, queries with 15, 16 and 17 equal keys."""
    X, ids, axis = pc.assign_bucket(n_list)
    off, nl = np.array([0, len(X)], np.int64), np.array([n_list], np.int32)
    Xd = _dev(ctx, X)
    plain = ctx.ivf_build(Xd, off, nl, kmeans_iters=0)
    keyed = ctx.ivf_build(Xd, off, nl, kmeans_iters=0, Xkm=_half(Xd))
    assert ctx.counter(6) == 0
    C, asg, perm, loff = fo.ivf_build(X, n_list, 0)
    for what, index in (("exact build", plain), ("keyed build", keyed)):
        cent, a, p, lo = (t.cpu().numpy() for t in index.export())
        wrong = np.flatnonzero(a != asg)
        names = sorted({nm for nm, r in ids.items() if len(np.intersect1d(r, wrong))})
        assert len(wrong) == 0, (what, len(wrong), wrong[:8], a[wrong[:8]], asg[wrong[:8]], names)
        assert np.array_equal(cent, C) and np.array_equal(p, perm) and np.array_equal(lo, loff), what
    for n_probe in (1, 3) + ((128,) if n_list == 128 else ()):
        rs, ri = fo.ivf_search(X, C, asg, perm, loff, n_probe, 32)
        for what, index in (("exact build", plain), ("keyed build", keyed)):
            sim, idx = index.search(n_probe, 32)
            _same_topk(sim, idx, rs, ri, f"{what}, {n_list} lists, n_probe {n_probe}")
    plain.close(), keyed.close()
