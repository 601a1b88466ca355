"""The host plan of a search (`csrc/searchplan.h`, plain C++) compiled on its own (tests/hostbuild.py) and compared with the
rules as tests/search_cases.py states them in Python: bucket order and kernel choice, the XCD dealing, the flat, tile and bucket
batch cuts at a cap given as an argument, the dense4 item table and the roofline counters."""
import ctypes as C

import numpy as np
import pytest

from tests import hostbuild
from tests import search_cases as sc

pytestmark = pytest.mark.skipif(not hostbuild.have_compiler(), reason="no host C++ compiler and no hipcc")

# jobs cross the boundary as rows of 7 int64: q_row0, c_row0, obase, tile0, nq, nc, xtile0
SHIM = r"""
#include <stddef.h>
#include "searchplan.h"
using namespace fal;
static void put(const std::vector<DenseJob>& v, int64_t* out) {
    for (size_t i = 0; i < v.size(); ++i) {
        const int64_t w[7] = {v[i].q_row0, v[i].c_row0, v[i].obase, v[i].tile0, v[i].nq, v[i].nc, v[i].xtile0};
        for (int k = 0; k < 7; ++k) out[7 * i + k] = w[k];
    }
}
static std::vector<DenseJob> get(const int64_t* in, int64_t n) {
    std::vector<DenseJob> v;
    for (int64_t i = 0; i < n; ++i)
        v.push_back({in[7 * i], in[7 * i + 1], in[7 * i + 2], in[7 * i + 3], (int32_t)in[7 * i + 4], (int32_t)in[7 * i + 5], in[7 * i + 6]});
    return v;
}
extern "C" {
void p_layout(int64_t* out) {
    const int64_t w[8] = {sizeof(DenseJob), offsetof(DenseJob, q_row0), offsetof(DenseJob, c_row0), offsetof(DenseJob, obase),
                          offsetof(DenseJob, tile0), offsetof(DenseJob, nq), offsetof(DenseJob, nc), offsetof(DenseJob, xtile0)};
    for (int k = 0; k < 8; ++k) out[k] = w[k];
}
int64_t p_block(int64_t nq, int64_t nc) { return sims_block_floats(nq, nc); }
int64_t p_cap(int64_t mb) { return (int64_t)sims_cap_floats((size_t)mb); }
int64_t p_small_max(int have4, int d, int env) { return FlatRule::make(false, have4 != 0, true, d, env).small_max; }
int p_kernel(int have16, int have4, int has_f32, int d, int64_t small_max, int64_t nb) {
    return flat_kernel_of(FlatRule{have16 != 0, have4 != 0, has_f32 != 0, d, small_max}, nb);
}
int64_t p_deal(const int64_t* tiles, int64_t n, int64_t* at) {
    XcdDeal x;
    for (int64_t j = 0; j < n; ++j) at[j] = x.take((size_t)j, tiles[j]);
    return x.longest();
}
int64_t p_order(const int64_t* off, const int32_t* nl, int64_t nb, int64_t* out) {
    const std::vector<int64_t> o = flat_order(off, nl, nb);
    for (size_t i = 0; i < o.size(); ++i) out[i] = o[i];
    return (int64_t)o.size();
}
// -> batches; jobs [flat buckets][7], batches [..][10], out = need, counters 0 / 4 / 7 / 8
int64_t p_flat(const int64_t* off, const int32_t* nl, int64_t nb, int have16, int have4, int has_f32, int d, int64_t small_max,
               int64_t cap, int64_t* jobs, int64_t* batches, int64_t* out) {
    const FlatRule rule{have16 != 0, have4 != 0, has_f32 != 0, d, small_max};
    const FlatPlan p = plan_flat(flat_order(off, nl, nb), off, rule, (size_t)cap);
    put(p.jobs, jobs);
    for (size_t i = 0; i < p.batches.size(); ++i) {
        const FlatBatch& b = p.batches[i];
        const int64_t w[10] = {(int64_t)b.j0, (int64_t)b.jm, (int64_t)b.js, (int64_t)b.jk, (int64_t)b.j1, b.tiles, b.list_tiles16,
                               b.list_tiles32, b.list_tiles1, b.floats};
        for (int k = 0; k < 10; ++k) batches[10 * i + k] = w[k];
    }
    const FlatCounters c = flat_counters(p, have4 != 0);
    out[0] = (int64_t)p.need; out[1] = c.pairs; out[2] = c.mfma; out[3] = c.tiny_pairs; out[4] = c.tiny_mfma;
    return (int64_t)p.batches.size();
}
// -> jobs of the 32-row table; out = jobs of the 128-row table, the two longest lists, pairs
int64_t p_fused(const int64_t* off, const int32_t* nl, int64_t nb, int k_ann, int64_t* j32, int64_t* j128, int64_t* out) {
    const FusedFlatPlan p = plan_fused_flat(flat_order(off, nl, nb), off, k_ann);
    put(p.j32, j32);
    put(p.j128, j128);
    out[0] = (int64_t)p.j128.size(); out[1] = p.list_tiles32; out[2] = p.list_tiles128; out[3] = p.pairs;
    return (int64_t)p.j32.size();
}
int64_t p_coarse(const int64_t* off, const int32_t* nl, const int64_t* base, int64_t nb, int64_t* jobs, int64_t* out) {
    const CoarsePlan p = plan_coarse(off, nl, base, nb);
    put(p.jobs, jobs);
    out[0] = p.tiles; out[1] = p.floats; out[2] = p.max_n_list;
    return (int64_t)p.jobs.size();
}
// -> cuts; obase[i] = obase_of_tile at cuts[i] (the last cut, n_tiles, is no tile)
int64_t p_tile_cuts(const int64_t* jobs, int64_t n, int64_t n_tiles, int64_t cap, int64_t* cuts, int64_t* obase, int64_t* need) {
    const std::vector<DenseJob> v = get(jobs, n);
    const TileCuts c = cut_tile_batches(v, n_tiles, (size_t)cap);
    for (size_t i = 0; i < c.cuts.size(); ++i) {
        cuts[i] = c.cuts[i];
        obase[i] = (!v.empty() && c.cuts[i] < n_tiles) ? obase_of_tile(v, c.cuts[i]) : -1;
    }
    *need = (int64_t)c.need;
    return (int64_t)c.cuts.size();
}
int64_t p_bucket_cuts(const int64_t* jobs, int64_t n, const int64_t* qoff, int64_t n_qoff, int64_t cap, int64_t* out, int64_t* need) {
    const BucketCuts c = cut_bucket_batches(get(jobs, n), std::vector<int64_t>(qoff, qoff + n_qoff), cap);
    for (size_t i = 0; i < c.batches.size(); ++i) {
        out[2 * i] = (int64_t)c.batches[i].j0;
        out[2 * i + 1] = (int64_t)c.batches[i].j1;
    }
    *need = (int64_t)c.need;
    return (int64_t)c.batches.size();
}
int64_t p_sorted32(const int64_t* jobs, int64_t n, int64_t* out) {
    const SortedTiles32 p = plan_sorted_tiles32(get(jobs, n));
    put(p.j32, out);
    return p.list_tiles32;
}
int64_t p_items(const int32_t* nq, int64_t n, int32_t* out) {
    std::vector<DenseJob> v((size_t)n, DenseJob{0, 0, 0, 0, 0, 0, 0});
    for (int64_t j = 0; j < n; ++j) v[(size_t)j].nq = nq[j];
    const std::vector<int32_t> t = dense4_items(v.data(), (int)n);
    for (size_t i = 0; i < t.size(); ++i) out[i] = t[i];
    return (int64_t)t.size();
}
}
"""

I64 = C.c_int64


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = hostbuild.compile_shim(tmp_path_factory.mktemp("searchplan"), "searchplan_shim", SHIM)
    for name in ("p_block", "p_cap", "p_small_max", "p_deal", "p_order", "p_flat", "p_fused", "p_coarse", "p_tile_cuts",
                 "p_bucket_cuts", "p_sorted32", "p_items"):
        getattr(lib, name).restype = I64
    return lib


def table(sizes, n_list):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return off, np.asarray(n_list, np.int32), np.concatenate([[0], np.cumsum(n_list)]).astype(np.int64)


def rows(a, n, w=7):
    return [tuple(int(x) for x in r) for r in a[:n * w].reshape(n, w)]


def flat(lib, sizes, n_list, rule, cap):
    """-> (jobs, batches, need, counters 0 / 4 / 7 / 8) of the shim"""
    off, nl, _ = table(sizes, n_list)
    jobs, batches, out = np.zeros(7 * len(sizes) + 7, np.int64), np.zeros(10 * len(sizes) + 10, np.int64), np.zeros(5, np.int64)
    nb = lib.p_flat(_p(off), _p(nl), I64(len(sizes)), *rule[:4], I64(rule[4]), I64(cap), _p(jobs), _p(batches), _p(out))
    n_jobs = sum(1 for s, l in zip(sizes, n_list) if l == 1 and s > 0)
    return rows(jobs, n_jobs), rows(batches, nb, 10), int(out[0]), tuple(int(x) for x in out[1:])


def check_flat(lib, sizes, n_list, rule, cap):
    """the shim's plan == the Python rule's; the properties every plan has.  -> (jobs, batches)"""
    jobs, batches, need, counters = flat(lib, sizes, n_list, rule, cap)
    rj, rb, rneed = sc.plan_flat(sizes, n_list, rule, cap)
    assert jobs == rj and batches == rb and need == rneed
    assert counters == sc.flat_counters(rj, rb, rule[1])
    assert [b[0] for b in batches] == [0] + [b[4] for b in batches[:-1]] and (not batches or batches[-1][4] == len(jobs))
    for j0, jm, js, jk, j1, tiles, lt16, lt32, lt1, floats in batches:
        assert j0 <= jm <= js <= jk <= j1 and j1 > j0
        assert floats <= cap or j1 == j0 + 1                                       # over the cap: one bucket alone
        assert jobs[j0][2] == 0 and jobs[j0][3] == 0                               # obase and tile0 restart
        for lo, hi, per, longest in ((j0, jm, 128, lt16), (js, jk, 32, lt1), (jk, j1, 32, lt32)):
            t = [sc.ceil_div(j[4], per) for j in jobs[lo:hi]]
            for i in range(hi - lo):                                               # xtile0: the earlier jobs of the same list
                assert jobs[lo + i][6] == sum(t[i % 8:i:8])
            assert longest == max([sum(t[x::8]) for x in range(8)], default=0)
        assert all(j[6] == 0 for j in jobs[jm:js])
        cls = [sc.kernel_of(rule, j[4]) for j in jobs[j0:j1]]
        assert cls == sorted(cls)                                                  # the classes are runs, in launch order
        assert [c for c in cls if c == sc.F16] == cls[:jm - j0] and cls[jm - j0:js - j0] == [sc.DENSE4] * (js - jm)
        assert cls[js - j0:jk - j0] == [sc.ONE_WAVE] * (jk - js)
    return jobs, batches


def test_job_layout_and_block_rule(lib):
    out = np.zeros(8, np.int64)
    lib.p_layout(_p(out))
    assert out.tolist() == [48, 0, 8, 16, 24, 32, 36, 40]                          # what the kernels read (simtile.h)
    for nq, nc in [(1, 1), (32, 32), (33, 33), (1000, 1000), (3000, 16), (65535, 65535), (64, 4097)]:
        assert lib.p_block(I64(nq), I64(nc)) == sc.block_floats(nq, nc)
    assert lib.p_block(I64(1000), I64(1000)) == 1048576
    assert [lib.p_cap(I64(mb)) for mb in (0, 8, 16, 17, 2048)] == [4194304, 4194304, 4194304, 17 * 262144, 2048 * 262144]
    for have4, d, env in [(1, 400, 0), (1, 400, 100), (1, 400, 7), (1, 512, 100), (1, 800, 100), (0, 400, 100)]:
        assert lib.p_small_max(have4, d, env) == sc.small_max_of(have4, d, env)


def test_order_is_stable_by_decreasing_size(lib):
    sizes, n_list = sc.MIXED
    off, nl, _ = table(sizes, n_list)
    out = np.zeros(len(sizes), np.int64)
    n = lib.p_order(_p(off), _p(nl), I64(len(sizes)), _p(out))
    got = out[:n].tolist()
    assert got == sc.flat_order(sizes, n_list)
    assert all(n_list[b] == 1 and sizes[b] > 0 for b in got) and n == sum(1 for s, l in zip(sizes, n_list) if l == 1 and s > 0)
    assert all(sizes[a] > sizes[b] or (sizes[a] == sizes[b] and a < b) for a, b in zip(got, got[1:]))   # ties keep bucket order
    for case in ([], [0, 0], [5]):
        off, nl, _ = table(case, [1] * len(case))
        assert lib.p_order(_p(off), _p(nl), I64(len(case)), _p(out)) == sum(1 for s in case if s > 0)


@pytest.mark.parametrize("rule", sc.RULES)
def test_kernel_choice(lib, rule):
    for nb in sc.EDGE_SIZES[1:] + [100, 101]:
        assert lib.p_kernel(*rule[:4], I64(rule[4]), I64(nb)) == sc.kernel_of(rule, nb), nb
    check_flat(lib, sc.EDGE_SIZES, [1] * len(sc.EDGE_SIZES), rule, sc.BIG_CAP)
    check_flat(lib, *sc.MIXED, rule, sc.BIG_CAP)
    check_flat(lib, *sc.MIXED, rule, 3 * 1048576)


@pytest.mark.parametrize("n", sc.DEAL_COUNTS)
def test_xcd_dealing(lib, n):
    tiles = np.array([1 + (7 * i) % 11 for i in range(n)], np.int64)
    at = np.zeros(n, np.int64)
    longest = lib.p_deal(_p(tiles), I64(n), _p(at))
    assert at.tolist() == [int(tiles[j % 8:j:8].sum()) for j in range(n)] == sc.deal(tiles.tolist())[0]
    assert longest == max(int(tiles[x::8].sum()) for x in range(8))
    sizes = sc.per_class(n)
    for rule in ((0, 1, 1, 400, 100), (1, 1, 1, 400, 100)):
        for cap in (sc.BIG_CAP, 200000):                                          # (the small cap: several batches, each dealt anew)
            jobs, batches = check_flat(lib, sizes, [1] * len(sizes), rule, cap)
    assert len(batches) > 1 or n == 1
    jobs, batches = check_flat(lib, sizes, [1] * len(sizes), (0, 1, 1, 400, 100), sc.BIG_CAP)
    assert [batches[0][i + 1] - batches[0][i] for i in range(4)] == [0, n, n, n]   # n jobs in each fp32 class


@pytest.mark.parametrize("name,sizes,rule,cap,expect", sc.FLAT_CUTS, ids=[c[0] for c in sc.FLAT_CUTS])
def test_flat_batch_cuts(lib, name, sizes, rule, cap, expect):
    jobs, batches = check_flat(lib, sizes, [1] * len(sizes), rule, cap)
    if expect is not None:
        assert [b[4] - b[0] for b in batches] == expect
    if name.startswith("one bucket over the cap"):
        assert batches[0][9] == sc.block_floats(3000, 3000) > cap                 # need = its own size
        assert flat(lib, sizes, [1] * len(sizes), rule, cap)[2] == batches[0][9]
    if name.startswith("cut between"):
        j0, jm, js, jk, j1 = batches[1][:5]
        assert (jm - j0, js - j0, jk - j0, j1 - j0) == (0, 3, 3, 5)                # no f16 job, three dense4, two one-block
        assert batches[0][:5] == (0, 4, 4, 4, 4)
    if name.startswith("cut inside"):
        assert len(batches) == 2 and batches[1][1] == batches[1][2] == batches[1][0] and batches[1][3] == batches[1][4]
        assert jobs[batches[1][0]][6] == 0                                         # the dealing starts again


def test_the_gpu_test_flat_case(lib):
    """tests/search_batches_worker.py expects this many batches from the library under FALCON_SIMS_MB=16"""
    assert lib.p_cap(I64(16)) == sc.CAP_1000
    _, batches = check_flat(lib, sc.GPU_FLAT_SIZES, [1] * len(sc.GPU_FLAT_SIZES), sc.GPU_FLAT_RULE, sc.CAP_1000)
    assert len(batches) == sc.GPU_FLAT_BATCHES == 3
    assert len(check_flat(lib, [1000] * 9, [1] * 9, sc.GPU_FLAT_RULE, sc.CAP_1000)[1]) == 3


@pytest.mark.parametrize("k_ann", [16, 128, 700])
def test_fused_flat_tables(lib, k_ann):
    sizes, n_list = sc.MIXED
    off, nl, _ = table(sizes, n_list)
    j32, j128, out = np.zeros(7 * len(sizes), np.int64), np.zeros(7 * len(sizes), np.int64), np.zeros(4, np.int64)
    n32 = lib.p_fused(_p(off), _p(nl), I64(len(sizes)), k_ann, _p(j32), _p(j128), _p(out))
    r32, r128, l32, l128, pairs = sc.plan_fused(sizes, n_list, k_ann)
    assert rows(j32, n32) == r32 and rows(j128, int(out[0])) == r128
    assert out[1:].tolist() == [l32, l128, pairs]


def coarse(lib, sizes, n_list):
    off, nl, base = table(sizes, n_list)
    jobs, out = np.zeros(7 * len(sizes), np.int64), np.zeros(3, np.int64)
    n = lib.p_coarse(_p(off), _p(nl), _p(base), I64(len(sizes)), _p(jobs), _p(out))
    assert (rows(jobs, n), *out.tolist()) == sc.plan_coarse(sizes, n_list)
    return jobs[:7 * n], n, int(out[0])


def test_coarse_jobs_and_tile_cuts(lib):
    jobs, n, n_tiles = coarse(lib, *sc.COARSE)
    ref = sc.plan_coarse(*sc.COARSE)[0]
    widest = max(sc.block_floats(32, j[5]) for j in ref)
    for cap in (3 * widest, widest, widest - 1, 1024, sc.BIG_CAP):
        cuts, obase, need = np.zeros(n_tiles + 2, np.int64), np.zeros(n_tiles + 2, np.int64), I64()
        nc = lib.p_tile_cuts(_p(jobs), I64(n), I64(n_tiles), I64(cap), _p(cuts), _p(obase), C.byref(need))
        cuts, obase = cuts[:nc].tolist(), obase[:nc].tolist()
        rcuts, rneed = sc.tile_cuts(ref, cap)
        assert cuts == rcuts and need.value == rneed
        assert cuts[0] == 0 and cuts[-1] == n_tiles and all(a < b for a, b in zip(cuts, cuts[1:]))      # [0, n_tiles], no gap
        per_tile = [sc.block_floats(32, j[5]) for j in ref for _ in range(sc.ceil_div(j[4], 32))]
        run = np.concatenate([[0], np.cumsum(per_tile)])
        for a, b in zip(cuts, cuts[1:]):
            assert run[b] - run[a] <= cap or b == a + 1                            # over the cap: one tile alone
        assert obase[:-1] == [int(run[t]) for t in cuts[:-1]]                      # obase_of_tile = the running sum
        assert need.value == max(int(run[b] - run[a]) for a, b in zip(cuts, cuts[1:]))
    cuts, obase, need = np.zeros(2, np.int64), np.zeros(2, np.int64), I64()
    assert lib.p_tile_cuts(_p(jobs), I64(0), I64(0), I64(1024), _p(cuts), _p(obase), C.byref(need)) == 1 and need.value == 0


def bucket_cuts(lib, ref, qoff, cap):
    jobs = np.array(ref, np.int64).reshape(-1)
    q = np.asarray(qoff, np.int64)
    out, need = np.zeros(2 * len(ref) + 2, np.int64), I64()
    n = lib.p_bucket_cuts(_p(jobs), I64(len(ref)), _p(q), I64(len(q)), I64(cap), _p(out), C.byref(need))
    got = rows(out, n, 2)
    assert (got, need.value) == sc.bucket_cuts(ref, qoff, cap)
    assert got[0][0] == 0 and got[-1][1] == len(ref) and all(a[1] == b[0] for a, b in zip(got, got[1:]))
    return got, need.value


def test_bucket_batch_cuts(lib):
    ref = sc.plan_coarse([64, 64, 32, 96, 64], [2, 2, 2, 2, 2])[0]                 # 2, 2, 1, 3, 2 tiles
    spans = [500, 500, 1000, 300, 700]                                             # candidates of every bucket
    per_tile = [s / sc.ceil_div(j[4], 32) for s, j in zip(spans, ref) for _ in range(sc.ceil_div(j[4], 32))]
    qoff = np.concatenate([[0], np.cumsum(per_tile)]).astype(np.int64).tolist()
    assert bucket_cuts(lib, ref, qoff, 1000) == ([(0, 2), (2, 3), (3, 5)], 1000)   # a span equal to the cap does not cut ...
    assert bucket_cuts(lib, ref, qoff, 999) == ([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], 1000)   # ... one over it does
    assert bucket_cuts(lib, ref, qoff, 400) == ([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], 1000)   # a first bucket over the cap
    assert bucket_cuts(lib, ref, qoff, 1300) == ([(0, 2), (2, 4), (4, 5)], 1300)
    assert bucket_cuts(lib, ref, qoff, sc.BIG_CAP) == ([(0, 5)], 3000)
    # the two 3,000-row buckets of tests/search_batches_worker.py, every list probed: 9 M candidates each
    ref = sc.plan_coarse([3000, 3000], [16, 16])[0]
    qoff = [3000 * min(32 * t, 3000) if t <= 94 else 9000000 + 3000 * min(32 * (t - 94), 3000) for t in range(189)]
    assert bucket_cuts(lib, ref, qoff, sc.CAP_1000) == ([(0, 1), (1, 2)], 9000000)        # the staged path's batches
    assert bucket_cuts(lib, ref, qoff, 2 * sc.CAP_1000) == ([(0, 1), (1, 2)], 9000000)    # the key path's: twice the candidates


def test_sorted_tiles32(lib):
    ref = sc.plan_coarse(*sc.COARSE)[0] + sc.plan_coarse([700] * 9, [4] * 9)[0]
    jobs, out = np.array(ref, np.int64).reshape(-1), np.zeros(7 * len(ref), np.int64)
    longest = lib.p_sorted32(_p(jobs), I64(len(ref)), _p(out))
    assert (rows(out, len(ref)), longest) == sc.sorted_tiles32(ref)


@pytest.mark.parametrize("nq", sc.ITEM_CASES, ids=lambda v: f"{len(v)} jobs")
def test_dense4_items(lib, nq):
    a = np.asarray(nq, np.int32)
    out = np.zeros(16 + 2 * (int(sum(sc.ceil_div(x, 128) for x in nq)) + 1), np.int32)
    n = lib.p_items(_p(a), I64(len(nq)), _p(out))
    t = out[:n].tolist()
    assert t == sc.dense4_items(nq)
    head, items = t[:9], list(zip(t[16::2], t[17::2]))
    assert head[0] == 0 and all(a <= b for a, b in zip(head, head[1:])) and head[8] == len(items)   # monotone offsets
    for x in range(8):                                                             # list x: its jobs in order, groups ascending
        assert items[head[x]:head[x + 1]] == [(j, g) for j in range(x, len(nq), 8) for g in range(sc.ceil_div(nq[j], 128))]
    assert [sc.ceil_div(v, 128) for v in (1, 128, 129)] == [1, 1, 2]
