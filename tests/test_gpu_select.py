"""The wavefront top-k select (csrc/select.h) on designed rows (tests/select_cases.py), bit for bit against plain references:
the staged top-k of flat and IVF buckets for every k, the fused filter of the staged select and the prefilter path's
resolve / fallback kernels against the CPU filter applied to the reference top-k.  No tolerances anywhere: every similarity
is one exact float32 product or zero.  tests/test_select_cases_cpu.py shows which branch of select.h each case reaches."""
import numpy as np
import pytest

from oracle import falcon_oracle as fo
from tests import select_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


class _Flat:
    """an index over flat cases + the plain reference of its rows (built once)"""

    def __init__(self, ctx, cases, half=False):
        import torch
        self.cases = cases
        X, self.off = sc.vectors(cases)
        self.n = len(X)
        self.Xd = torch.from_numpy(X).to(ctx.tdev)
        nl = np.ones(len(cases), np.int32)
        self.index = ctx.ivf_build(self.Xd, self.off, nl)
        self.pre = ctx.ivf_build(self.Xd, self.off, nl, Xpre=self.Xd.to(torch.float16).contiguous()) if half else None
        self.sim, self.idx = sc.flat_reference(cases)

    def case_of(self, row):
        return self.cases[int(np.searchsorted(self.off, row, side="right")) - 1]


def _rebased(cases):
    out, row0 = [], 0
    for c in cases:
        c2 = sc.FlatCase(c.pattern, c.name, c.s)
        c2.row0 = row0
        row0 += c.n
        out.append(c2)
    return tuple(out)


@pytest.fixture(scope="module")
def flat(ctx):
    return _Flat(ctx, sc.flat_cases())


@pytest.fixture(scope="module")
def survivors(ctx):
    return {with_rt: (_Flat(ctx, sc.survivor_cases(with_rt)[0], half=True),) + sc.survivor_cases(with_rt)[1:] for with_rt in (False, True)}


@pytest.fixture(scope="module")
def tie_rows(ctx):
    return _Flat(ctx, _rebased([c for c in sc.flat_cases() if c.pattern in sc.FALLBACK_PATTERNS]), half=True)


class _Ivf:
    def __init__(self, ctx):
        import torch
        self.X, self.off, self.nl = sc.ivf_vectors()
        self.n = len(self.X)
        self.Xd = torch.from_numpy(self.X).to(ctx.tdev)
        self.index = ctx.ivf_build(self.Xd, self.off, self.nl, kmeans_iters=sc.IVF_KMEANS_ITERS)
        self.pre = ctx.ivf_build(self.Xd, self.off, self.nl, kmeans_iters=sc.IVF_KMEANS_ITERS,
                                 Xpre=self.Xd.to(torch.float16).contiguous(), prefilter_which=2)
        self.exported = [t.cpu().numpy() for t in self.index.export()]
        self._ref = {}

    def reference(self, n_probe):
        """`fo.ivf_search` on the exported index, K_MAX wide (a smaller k is a prefix)"""
        if n_probe not in self._ref:
            cent, asg, perm, loff = self.exported
            lb = np.concatenate([[0], np.cumsum(self.nl)])
            parts = []
            for b, (a, e) in enumerate(zip(self.off[:-1], self.off[1:])):
                lo = loff[lb[b]:lb[b + 1] + 1] - a
                parts.append(fo.ivf_search(self.X[a:e], cent[lb[b]:lb[b + 1]], asg[a:e], perm[a:e] - a, lo, n_probe, sc.K_MAX, base=a))
            self._ref[n_probe] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        return self._ref[n_probe]


@pytest.fixture(scope="module")
def ivf(ctx):
    return _Ivf(ctx)


def _same_topk(sim, idx, rs, ri, k, name=lambda row: ""):
    sim, idx = sim.cpu().numpy(), idx.cpu().numpy()
    rs, ri = rs[:, :k], ri[:, :k]
    bad = np.flatnonzero((idx != ri).any(1) | (sim.view(np.uint32) != rs.view(np.uint32)).any(1))
    if len(bad):
        r = int(bad[0])
        j = int(np.flatnonzero((idx[r] != ri[r]) | (sim[r].view(np.uint32) != rs[r].view(np.uint32)))[0])
        lo = max(j - 2, 0)
        raise AssertionError(f"k {k}: {len(bad)} rows differ, first row {r} {name(r)} at rank {j}: got ids {idx[r, lo:j + 3]} "
                             f"sims {sim[r, lo:j + 3]}, expected ids {ri[r, lo:j + 3]} sims {rs[r, lo:j + 3]}; "
                             f"rows of {sorted({str(name(int(b))) for b in bad})[:12]}")


def _same_neighbours(got, index, ref_sim, ref_idx, k_ann, mz, rt, tol, mode, rt_tol, keep, name=lambda row: "", what=""):
    """`search_neighbors` output == the CPU filter (`fo.filter_neighbors`) of the reference top-k_ann; nb_count too"""
    g_idx, g_dist = (t.cpu().numpy() for t in got)
    cnt = index.nb_count.cpu().numpy()
    e_idx, e_dist = fo.filter_neighbors(ref_sim[:, :k_ann], ref_idx[:, :k_ann], mz, rt, tol, mode, rt_tol, keep)
    bad = np.flatnonzero((g_idx != e_idx).any(1) | (g_dist.view(np.uint32) != e_dist.view(np.uint32)).any(1))
    if len(bad):
        r = int(bad[0])
        raise AssertionError(f"{what} k_ann {k_ann} keep {keep}: {len(bad)} rows differ, first row {r} {name(r)}: got {g_idx[r, :8]} "
                             f"{g_dist[r, :8]}, expected {e_idx[r, :8]} {e_dist[r, :8]}; rows of {sorted({str(name(int(b))) for b in bad})[:12]}")
    assert np.array_equal(cnt, (e_idx >= 0).sum(1)), (what, keep)
    return e_idx


def _dev(ctx, a):
    import torch
    return None if a is None else torch.from_numpy(a).to(ctx.tdev)


# --------------------------------------------------------------------------- staged top-k
@pytest.mark.parametrize("k", sc.K_VALUES)
def test_staged_topk_of_designed_flat_rows(flat, k):
    """select_kernel<MODE_DENSE, false> on every pattern and size: similarities, ids, tie order and padding"""
    sim, idx = flat.index.search(16, k)
    _same_topk(sim, idx, flat.sim, flat.idx, k, flat.case_of)


def test_ivf_index_is_the_one_the_model_assumes(ivf):
    """list i of a bucket = axis i (+ the zero rows in list 0), as tests/test_select_cases_cpu.py models the candidate counts"""
    cent, asg, perm, loff = ivf.exported
    lb = np.concatenate([[0], np.cumsum(ivf.nl)])
    for b, (a, e) in enumerate(zip(ivf.off[:-1], ivf.off[1:])):
        C, ra, rperm, roff = fo.ivf_build(ivf.X[a:e], int(ivf.nl[b]), sc.IVF_KMEANS_ITERS)
        assert np.array_equal(asg[a:e], ra) and np.array_equal(perm[a:e] - a, rperm)
        assert np.array_equal(loff[lb[b]:lb[b + 1] + 1] - a, roff) and np.array_equal(np.diff(roff), sc.IVF_LISTS[b])


@pytest.mark.parametrize("k", sc.K_VALUES)
@pytest.mark.parametrize("n_probe", sc.IVF_PROBES)
def test_staged_topk_of_designed_ivf_rows(ivf, n_probe, k):
    """select_kernel<MODE_IVF, false>: ties at zero by the thousand, ids through perm, both chunk load forms"""
    rs, ri = ivf.reference(n_probe)
    sim, idx = ivf.index.search(n_probe, k)
    _same_topk(sim, idx, rs, ri, k, lambda r: f"bucket {int(np.searchsorted(ivf.off, r, side='right')) - 1}")


# --------------------------------------------------------------------------- the fused filter and the prefilter path
_FILTERS = {False: (0.05, "Da", None), True: (20.0, "ppm", 10.0)}


@pytest.mark.parametrize("with_rt", [False, True], ids=["Da", "ppm+rt"])
@pytest.mark.parametrize("path", ["staged", "prefilter"])
def test_filter_with_designed_survivor_counts(ctx, survivors, path, with_rt):
    """exactly c of a query's 256 candidates pass, c = 0 .. 256 across the network cuts; n_neighbors = 1, c - 1, c, c + 1, 256.
    staged: select_kernel<MODE_DENSE, true> (filter_sort_store).  prefilter: the same index with float16 rows --
    resolve_kernel's rank / sort-32 / sort-64 forms up to 64 survivors, the exact fallback beyond."""
    fl, mz, rt, queries = survivors[with_rt]
    tol, mode, rt_tol = _FILTERS[with_rt]
    index = fl.index if path == "staged" else fl.pre
    mz_d, rt_d = _dev(ctx, mz), _dev(ctx, rt)
    fb = set()
    for keep in sc.SURVIVOR_KEEPS:
        got = index.search_neighbors(16, sc.K_MAX, mz_d, rt_d, tol, mode, rt_tol, keep)
        if path == "prefilter":
            ctx.sync()
            fb.add(ctx.counter(5))
        e_idx = _same_neighbours(got, index, fl.sim, fl.idx, sc.K_MAX, mz, rt, tol, mode, rt_tol, keep, fl.case_of, path)
        for c, rows in queries:
            assert ((e_idx[rows] >= 0).sum(1) == min(c, keep)).all()
    if path == "prefilter":
        # a row with more than 64 survivors overflows the hand-off (FAL_FUSED_KEEP) and takes the exact fallback
        e_idx, _ = fo.filter_neighbors(fl.sim, fl.idx, mz, rt, tol, mode, rt_tol, sc.K_MAX)
        over = int(((e_idx >= 0).sum(1) > 64).sum())
        print(f"{mode}: fallback queries {sorted(fb)} of {fl.n} rows, {over} with more than 64 survivors")
        assert min(fb) >= over, (sorted(fb), over)


@pytest.mark.parametrize("with_rt", [False, True], ids=["Da", "ppm+rt"])
def test_resolve_kernel_runs_its_rank_and_both_sort_forms(ctx, with_rt):
    """Each survivor bucket as an index of its own, so the fallback counter speaks of that bucket alone.  A row with more than
    64 survivors must take the fallback; if fewer FURTHER rows took it than the bucket holds rows with 0..16 (17..32, 33..64)
    survivors, one of those was written by resolve_kernel's rank (sort-32, sort-64) form.  Every form is shown by a bucket."""
    import torch
    cases, mz, rt, _ = sc.survivor_cases(with_rt)
    tol, mode, rt_tol = _FILTERS[with_rt]
    shown, seen = [False] * 3, []
    for c in cases:
        sl = slice(c.row0, c.row0 + c.n)
        X, off = sc.vectors([c])
        Xd = torch.from_numpy(X).to(ctx.tdev)
        index = ctx.ivf_build(Xd, off, np.ones(1, np.int32), Xpre=Xd.to(torch.float16).contiguous())
        rs, ri = sc.plain_topk(sc.products(c.s), sc.K_MAX)
        mz_c, rt_c = mz[sl], None if rt is None else rt[sl]
        got = index.search_neighbors(16, sc.K_MAX, _dev(ctx, mz_c), _dev(ctx, rt_c), tol, mode, rt_tol, 64)
        ctx.sync()
        n_fb = ctx.counter(5)
        _same_neighbours(got, index, rs, ri, sc.K_MAX, mz_c, rt_c, tol, mode, rt_tol, 64, what=c.name)
        cnt = (fo.filter_neighbors(rs, ri, mz_c, rt_c, tol, mode, rt_tol, sc.K_MAX)[0] >= 0).sum(1)
        over = int((cnt > 64).sum())
        classes = [int(((cnt >= lo) & (cnt <= hi)).sum()) for lo, hi in ((0, 16), (17, 32), (33, 64))]
        seen.append((c.name, n_fb, over, classes))
        assert n_fb >= over, seen[-1]
        for j in range(3):
            shown[j] = shown[j] or n_fb - over < classes[j]
        index.close()
    print(seen)
    assert all(shown), (shown, seen)


@pytest.mark.parametrize("k_ann,keep", [(64, 16), (128, 256), (256, 64)])
def test_fused_filter_of_the_staged_select_on_every_pattern(ctx, flat, ivf, k_ann, keep):
    """select_kernel<., true> on the designed rows themselves (flat and IVF), a window of about a hundred rows passing"""
    for what, obj, n_probe, ref in (("flat", flat, 16, (flat.sim, flat.idx)), ("ivf", ivf, 3, ivf.reference(3))):
        mz = sc.window_mz(obj.n)
        got = obj.index.search_neighbors(n_probe, k_ann, _dev(ctx, mz), None, 0.05, "Da", None, keep)
        e_idx = _same_neighbours(got, obj.index, ref[0], ref[1], k_ann, mz, None, 0.05, "Da", None, keep, what=what)
        assert (e_idx >= 0).sum() > 0


@pytest.mark.parametrize("k_ann", [128, 256])
def test_tie_rows_funnel_through_the_flat_fallback(ctx, tie_rows, k_ann):
    """all_equal and tie_at_k with float16 rows: more keys at the threshold than the chip keeps, so the rows go through
    fused_fallback_kernel -- select_rounds<MODE_DENSE, 2 / 4 / 8 / 16> at that kernel's own cuts (128 / 256 / 512)"""
    fl = tie_rows
    mz = np.repeat(500.0 + np.arange(len(fl.cases)), [c.n for c in fl.cases]).astype(np.float32)      # a bucket = one window
    got = fl.pre.search_neighbors(16, k_ann, _dev(ctx, mz), None, 0.05, "Da", None, 64)
    ctx.sync()
    n_fb = ctx.counter(5)
    _same_neighbours(got, fl.pre, fl.sim, fl.idx, k_ann, mz, None, 0.05, "Da", None, 64, fl.case_of, "prefilter")
    # every row of an all_equal bucket with more than k_ann rows sees only keys equal to its k-th best
    tied = sum(c.n for c in fl.cases if c.pattern == "all_equal" and c.n > k_ann)
    print(f"fallback queries {n_fb}, rows of all_equal buckets above k_ann {tied}, rows {fl.n}")
    assert n_fb >= tied, (n_fb, tied)


@pytest.mark.parametrize("k_ann", sc.IVF_FALLBACK_K)
@pytest.mark.parametrize("n_probe", sc.IVF_PREFILTER_PROBES)
def test_zero_ties_funnel_through_the_ivf_fallback(ctx, ivf, n_probe, k_ann):
    """the IVF buckets with float16 rows: a query whose k-th best lies inside the tie group at zero cannot be settled from the
    keys and goes through ivf_fallback_kernel -- select_rounds<MODE_IVF, .> at the fallback's cuts, always the 16-byte load"""
    keep = 64
    mz = sc.window_mz(ivf.n)
    rs, ri = ivf.reference(n_probe)
    got = ivf.pre.search_neighbors(n_probe, k_ann, _dev(ctx, mz), None, 0.05, "Da", None, keep)
    ctx.sync()
    n_fb = ctx.counter(5)
    _same_neighbours(got, ivf.pre, rs, ri, k_ann, mz, None, 0.05, "Da", None, keep, what="ivf prefilter")
    # rows whose k_ann-th best is a zero with more zeros behind it
    tied = int(((rs[:, k_ann - 1] == 0) & (rs[:, k_ann] == 0)).sum())
    print(f"fallback queries {n_fb}, rows with the k-th best inside the zero ties {tied}, rows {ivf.n}")
    assert n_fb >= tied > 0, (n_fb, tied)
