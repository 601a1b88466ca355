"""The host plan of an index build (`csrc/buildplan.h`, plain C++) compiled on its own (tests/hostbuild.py) and compared with the
rules as tests/build_cases.py states them in Python: the list table and its validation, the assignment class of every bucket and
the job tables in upload order, the segment lengths at their clamps, and the small rules (sort bits, sparsify segments, coarse
keys against a budget given in bytes, the host-made counts and list offsets)."""
import ctypes as C

import numpy as np
import pytest

from tests import build_cases as bc
from tests import hostbuild

pytestmark = pytest.mark.skipif(not hostbuild.have_compiler(), reason="no host C++ compiler and no hipcc")

# buckets cross the boundary as rows of 5 int64 (row0, list0, n, n_list, wave0), assignment jobs as rows of 6 (row0, cent0,
# nrows, ncent, id_base, part0), dense jobs as rows of 7 (test_searchplan_cpu.py)
SHIM = r"""
#include <stddef.h>
#include "buildplan.h"
using namespace fal;
static std::vector<BucketDev> get(const int64_t* in, int64_t n) {
    std::vector<BucketDev> v;
    for (int64_t i = 0; i < n; ++i) v.push_back({in[5 * i], in[5 * i + 1], (int32_t)in[5 * i + 2], (int32_t)in[5 * i + 3], in[5 * i + 4]});
    return v;
}
static void put(const std::vector<AssignJob>& v, int64_t* out) {
    for (size_t i = 0; i < v.size(); ++i) {
        const int64_t w[6] = {v[i].row0, v[i].cent0, v[i].nrows, v[i].ncent, v[i].id_base, v[i].part0};
        for (int k = 0; k < 6; ++k) out[6 * i + k] = w[k];
    }
}
extern "C" {
void b_layout(int64_t* out) {
    const int64_t w[13] = {sizeof(BucketDev), offsetof(BucketDev, row0), offsetof(BucketDev, list0), offsetof(BucketDev, n),
                           offsetof(BucketDev, n_list), offsetof(BucketDev, wave0),
                           sizeof(AssignJob), offsetof(AssignJob, row0), offsetof(AssignJob, cent0), offsetof(AssignJob, nrows),
                           offsetof(AssignJob, ncent), offsetof(AssignJob, id_base), offsetof(AssignJob, part0)};
    for (int k = 0; k < 13; ++k) out[k] = w[k];
}
void b_consts(int64_t* out) {
    out[0] = kAssignSeg; out[1] = kAssignGroup; out[2] = kAssignMaxLists; out[3] = kAssignMergeLists; out[4] = kBucketSortMaxLists;
}
int b_all_flat(const int32_t* nl, int64_t nb) { return all_flat(nl, nb) ? 1 : 0; }
// -> first bad bucket or -1; list_base [nb + 1], bk [indexed buckets][5], out = indexed buckets, total lists, waves
int64_t b_lists(const int64_t* off, const int32_t* nl, int64_t nb, int max_n_list, int64_t* list_base, int64_t* bk, int64_t* out) {
    ListTable t;
    const int64_t bad = plan_lists(off, nl, nb, max_n_list, t);
    if (bad >= 0) return bad;
    for (size_t i = 0; i < t.list_base.size(); ++i) list_base[i] = t.list_base[i];
    for (size_t i = 0; i < t.bk.size(); ++i) {
        const int64_t w[5] = {t.bk[i].row0, t.bk[i].list0, t.bk[i].n, t.bk[i].n_list, t.bk[i].wave0};
        for (int k = 0; k < 5; ++k) bk[5 * i + k] = w[k];
    }
    out[0] = (int64_t)t.bk.size(); out[1] = t.total_lists; out[2] = t.ivf_waves;
    return -1;
}
// the tables are written when they hold at most `cap` jobs each; out = 14 scalars
void b_assign(const int64_t* bk, int64_t n_bk, int num_cus, int use16, int64_t cap, int64_t* wide, int64_t* half, int64_t* dense,
              int64_t* out) {
    const std::vector<BucketDev> v = get(bk, n_bk);
    const AssignPlan p = plan_assign(v.data(), v.size(), num_cus, use16 != 0);
    const int64_t w[14] = {(int64_t)p.wide.size(), p.n_wide, p.n_wave, (int64_t)p.half.size(), p.n_single, p.n_merge, p.n_group,
                           (int64_t)p.dense.size(), p.dtiles, p.merge_rows, p.merge_max_lists, p.max_n_list, p.seg, p.wseg};
    for (int k = 0; k < 14; ++k) out[k] = w[k];
    if ((int64_t)p.wide.size() > cap || (int64_t)p.half.size() > cap || (int64_t)p.dense.size() > cap) return;
    put(p.wide, wide);
    put(p.half, half);
    for (size_t i = 0; i < p.dense.size(); ++i) {
        const DenseJob& j = p.dense[i];
        const int64_t d[7] = {j.q_row0, j.c_row0, j.obase, j.tile0, j.nq, j.nc, j.xtile0};
        for (int k = 0; k < 7; ++k) dense[7 * i + k] = d[k];
    }
}
int b_end_bit(int64_t total) { return list_sort_end_bit(total); }
int b_sort_serves(int max_n_list) { return bucket_sort_serves(max_n_list) ? 1 : 0; }
void b_segments(const int64_t* bk, int64_t n_bk, int64_t* out) {
    const std::vector<BucketDev> v = get(bk, n_bk);
    const std::vector<int64_t> s = sparsify_segments(v.data(), v.size());
    for (size_t i = 0; i < s.size(); ++i) out[i] = s[i];
}
int b_stride(int max_n_list) { return ckeys_stride_of(max_n_list); }
int64_t b_key_bytes(int64_t n, int stride) { return (int64_t)ckeys_bytes(n, stride); }
int64_t b_budget(int64_t mb) { return (int64_t)ckeys_budget_bytes((size_t)mb); }
int b_fit(int64_t n, int stride, int64_t budget) { return ckeys_fit(n, stride, (size_t)budget) ? 1 : 0; }
int64_t b_counts(const int64_t* off, const int32_t* nl, const int64_t* base, int64_t nb, int64_t* out) {
    const std::vector<int64_t> c = initial_counts(off, nl, base, nb);
    for (size_t i = 0; i < c.size(); ++i) out[i] = c[i];
    return (int64_t)c.size();
}
int64_t b_flat_off(const int64_t* off, const int64_t* base, int64_t nb, int64_t* out) {
    const std::vector<int64_t> o = flat_list_off(off, base, nb);
    for (size_t i = 0; i < o.size(); ++i) out[i] = o[i];
    return (int64_t)o.size();
}
}
"""

I64 = C.c_int64
SCALARS = ("n_table", "n_wide", "n_wave", "n_half", "n_single", "n_merge", "n_group", "n_dense", "dtiles", "merge_rows",
           "merge_max_lists", "max_n_list", "seg", "wseg")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def load(tmp_dir):
    lib = hostbuild.compile_shim(tmp_dir, "buildplan_shim", SHIM)
    for name in ("b_lists", "b_key_bytes", "b_budget", "b_counts", "b_flat_off"):
        getattr(lib, name).restype = I64
    return lib


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return load(tmp_path_factory.mktemp("buildplan"))


def rows(a, n, w):
    return [tuple(int(x) for x in r) for r in a[:n * w].reshape(n, w)]


def lists(lib, off, n_list, max_n_list=bc.MAX_N_LIST):
    """-> the first bad bucket, or (list_base, bk, total, waves) of the shim"""
    off, nl = np.asarray(off, np.int64), np.asarray(n_list, np.int32)
    base, bk, out = np.zeros(len(nl) + 1, np.int64), np.zeros(5 * len(nl) + 5, np.int64), np.zeros(3, np.int64)
    bad = lib.b_lists(_p(off), _p(nl), I64(len(nl)), max_n_list, _p(base), _p(bk), _p(out))
    return bad if bad >= 0 else (base.tolist(), rows(bk, int(out[0]), 5), int(out[1]), int(out[2]))


def assign(lib, bk, num_cus, use16):
    """-> the shim's plan in the form of build_cases.plan_assign"""
    ref = bc.plan_assign(bk, num_cus, use16)
    cap = max(len(ref["wide"]), len(ref["half"]), len(ref["dense"]))
    a = np.array(bk, np.int64).reshape(-1)
    wide, half, dense, out = np.zeros(6 * cap + 6, np.int64), np.zeros(6 * cap + 6, np.int64), np.zeros(7 * cap + 7, np.int64), np.zeros(14, np.int64)
    lib.b_assign(_p(a), I64(len(bk)), num_cus, int(use16), I64(cap), _p(wide), _p(half), _p(dense), _p(out))
    s = dict(zip(SCALARS, (int(x) for x in out)))
    assert max(s["n_table"], s["n_half"], s["n_dense"]) <= cap, (s, cap)             # (else nothing was written)
    got = {k: s[k] for k in SCALARS[1:3] + SCALARS[4:7] + SCALARS[8:]}
    got.update(wide=rows(wide, s["n_table"], 6), half=rows(half, s["n_half"], 6), dense=rows(dense, s["n_dense"], 7))
    return got, ref


def check_assign(lib, bk, num_cus, use16):
    """the shim's plan == the Python rule's; the properties every plan has.  -> the plan"""
    got, ref = assign(lib, bk, num_cus, use16)
    assert got == ref
    p = got
    assert len(p["wide"]) == p["n_wide"] + p["n_wave"] and len(p["half"]) == p["n_single"] + p["n_merge"] + p["n_group"]
    single, merge = p["half"][:p["n_single"]], p["half"][p["n_single"]:p["n_single"] + p["n_merge"]]
    group = p["half"][p["n_single"] + p["n_merge"]:]
    covered = {}                                                                    # bucket (by its list 0) -> rows its jobs cover
    by_list0 = {b[1]: b for b in bk}

    def cover(jobs, width, seg):
        """jobs of one class: per segment the groups of `width` centroids side by side, ids from 0 up to the bucket's n_list"""
        i = 0
        while i < len(jobs):
            r, nr = jobs[i][0], jobs[i][2]
            b = by_list0[jobs[i][1] - jobs[i][4]]
            assert b[0] <= r and r + nr <= b[0] + b[2] and 0 < nr <= seg
            t = 0
            while t < b[3]:
                j = jobs[i]
                assert (j[0], j[2], j[1], j[4]) == (r, nr, b[1] + t, t) and j[3] == min(width, b[3] - t)
                t += j[3]
                i += 1
            assert covered.setdefault(b[1], b[0]) == r                              # the segments of a bucket in row order, no gap
            covered[b[1]] = r + nr
    cover(p["wide"][:p["n_wide"]], bc.GROUP, p["seg"])
    cover(p["wide"][p["n_wide"]:], 32, p["wseg"])
    cover(group, bc.GROUP, bc.SEG)
    for j in single:
        b = by_list0[j[1]]
        assert j[3] == b[3] <= bc.GROUP and j[4:] == (0, 0) and 0 < j[2] <= bc.SEG
        assert covered.setdefault(b[1], b[0]) == j[0]
        covered[b[1]] = j[0] + j[2]
    # merge jobs: part0 = the rows of the merge segments in front, across buckets; their groups carry the same part0
    assert [m[5] for m in merge] == [sum(x[2] for x in merge[:i]) for i in range(len(merge))]
    assert p["merge_rows"] == sum(m[2] for m in merge) and all(m[3] == by_list0[m[1]][3] and m[4] == 0 for m in merge)
    part_of = {m[0]: m[5] for m in merge}
    assert all(g[5] == part_of[g[0]] for g in group)
    assert p["merge_max_lists"] == max([m[3] for m in merge], default=0)
    for q_row0, c_row0, obase, tile0, nq, nc, xtile0 in p["dense"]:
        assert (q_row0, c_row0, nq, nc) == by_list0[c_row0][:4] and obase == 0 and xtile0 == 0
        covered[c_row0] = q_row0 + nq
    assert [d[3] for d in p["dense"]] == bc.offsets([bc.ceil_div(d[4], 32) for d in p["dense"]])[:-1]
    assert p["dtiles"] == sum(bc.ceil_div(d[4], 32) for d in p["dense"])
    for b in bk:                                                                    # every row of every indexed bucket, once
        assert covered.get(b[1], b[0]) == b[0] + b[2], b
    assert all(x % 32 == 0 and 256 <= x <= bc.SEG for x in (p["seg"], p["wseg"]))
    return p


def test_struct_layout_and_constants(lib):
    out = np.zeros(13, np.int64)
    lib.b_layout(_p(out))
    assert out.tolist() == [32, 0, 8, 16, 20, 24, 32, 0, 8, 16, 20, 24, 28]         # what the kernels read (ivf.hip, assign*.hip)
    lib.b_consts(_p(out))
    assert out[:5].tolist() == [bc.SEG, bc.GROUP, bc.MAX_LISTS, bc.MERGE_LISTS, bc.SORT_MAX_LISTS] == [2048, 128, 512, 2048, 2048]


@pytest.mark.parametrize("name", list(bc.TABLES))
def test_list_table(lib, name):
    sizes, n_list = bc.TABLES[name]
    off = bc.offsets(sizes)
    assert bc.first_bad_bucket(off, n_list) == -1
    got = lists(lib, off, n_list)
    assert got == bc.list_table(off, n_list)
    base, bk, total, waves = got
    assert total == sum(n_list) and waves == sum(nl for nl in n_list if nl > 1) and len(bk) == sum(1 for nl in n_list if nl > 1)
    assert [b[4] for b in bk] == bc.offsets([b[3] for b in bk])[:-1]                # wave0: the lists of the indexed buckets in front
    nl = np.asarray(n_list, np.int32)
    assert lib.b_all_flat(_p(nl), I64(len(nl))) == int(not bk)


@pytest.mark.parametrize("name,table,n_list,bad", bc.INVALID, ids=[c[0] for c in bc.INVALID])
def test_invalid_tables_report_the_first_bad_bucket(lib, name, table, n_list, bad):
    off = table["off"] if "off" in table else bc.offsets(table["sizes"])
    assert bc.first_bad_bucket(off, n_list) == bad
    got = lists(lib, off, n_list)
    assert (got if bad >= 0 else -1) == bad
    if name == "n_list at the limit is valid":                                      # the limit is an argument
        assert lists(lib, off, n_list, bc.MAX_N_LIST - 1) == 0


@pytest.mark.parametrize("use16", [False, True], ids=["exact", "use16"])
@pytest.mark.parametrize("n_list", bc.EDGE_LISTS)
def test_class_of_every_edge_list_count(lib, n_list, use16):
    bk = bc.list_table([0, bc.rows_for(n_list)], [n_list])[1]
    if n_list == 1:
        assert bk == []
    p = check_assign(lib, bk, 256, use16)
    filled = {bc.SINGLE: p["n_single"], bc.MERGE: p["n_merge"], bc.WAVE: p["n_wave"], bc.WIDE: p["n_wide"], bc.DENSE: len(p["dense"])}
    assert [c for c, n in filled.items() if n > 0] == ([bc.class_of(n_list, use16)] if n_list > 1 else [])
    if n_list > 1:
        assert p["n_group"] == p["n_merge"] * bc.ceil_div(n_list, bc.GROUP) and p["max_n_list"] == n_list


@pytest.mark.parametrize("use16", [False, True], ids=["exact", "use16"])
@pytest.mark.parametrize("num_cus", bc.NUM_CUS)
@pytest.mark.parametrize("name", ["edges", "sizes", "two merge buckets", "long", "all flat"])
def test_job_tables(lib, name, num_cus, use16):
    sizes, n_list = bc.TABLES[name]
    bk = lists(lib, bc.offsets(sizes), n_list)[1]
    check_assign(lib, bk, num_cus, use16)


def test_segment_lengths_reach_both_clamps(lib):
    seen = {"seg": set(), "wseg": set()}
    for name in ("edges", "sizes", "long"):
        bk = bc.list_table(bc.offsets(bc.TABLES[name][0]), bc.TABLES[name][1])[1]
        for num_cus in bc.NUM_CUS:
            p = check_assign(lib, bk, num_cus, False)
            seen["seg"].add(p["seg"])
            seen["wseg"].add(p["wseg"])
    for v in seen.values():
        assert {256, bc.SEG} <= v and any(256 < x < bc.SEG for x in v), seen
    # the cut sizes: 2,048 rows one segment, 2,049 two (the second of one row), 4,097 three
    bk = bc.list_table(bc.offsets(bc.CUT_SIZES), [100] * 3)[1]
    p = check_assign(lib, bk, 1, True)
    assert p["n_single"] == 1 + 2 + 3 and [j[2] for j in p["half"]] == [2048, 2048, 1, 2048, 2048, 1]


def test_two_merge_buckets_in_a_row(lib):
    sizes, n_list = bc.TWO_MERGE
    bk = bc.list_table(bc.offsets(sizes), n_list)[1]
    p = check_assign(lib, bk, 256, True)
    assert (p["n_single"], p["n_merge"], p["n_group"]) == (2, 3 + 2, 3 * 2 + 2 * 3)   # 16 lists: single; 129 and 300 lists: merge
    merge = p["half"][2:7]
    assert [m[5] for m in merge] == [0, 2048, 4096, 4200, 6248] and p["merge_rows"] == 6300   # part0 runs on into the next bucket
    group = p["half"][7:]
    assert [(g[0], g[4]) for g in group[:6]] == [(0, 0), (0, 128), (2048, 0), (2048, 128), (4096, 0), (4096, 128)]   # a segment's groups side by side
    assert [g[3] for g in group[6:9]] == [128, 128, 44] and p["merge_max_lists"] == 300
    q = check_assign(lib, bk, 256, False)                                           # without float16 rows: no merge, no part0
    assert (q["n_single"], q["n_merge"], q["n_group"], q["merge_rows"]) == (0, 0, 0, 0) and all(j[5] == 0 for j in q["wide"])


def test_the_gpu_test_table_fills_every_class(lib):
    """tests/test_gpu_search.py builds this table plain and with float16 rows: the classes each build must exercise.  With
    float16 rows every bucket of up to 2,048 lists takes a float16 class, so the one-wave and 4-wave exact classes only fill
    without them"""
    bk = lists(lib, bc.offsets(bc.GPU_SIZES), bc.GPU_LISTS)[1]
    for use16 in (True, False):
        check_assign(lib, bk, 256, use16)
        by_class = {}
        for b in bk:
            by_class.setdefault(bc.class_of(b[3], use16), []).append(b[3])
        assert by_class == bc.GPU_CLASSES[use16]
    p = check_assign(lib, bk, 256, True)
    assert p["n_merge"] == 3 + 1 + 2 and [j[5] for j in p["half"][p["n_single"]:p["n_single"] + 4]] == [0, 2048, 4096, 4200]


@pytest.mark.parametrize("total", [0, 1, 2, 3, 4, 5, 1 << 16, (1 << 16) + 1, 1 << 31, (1 << 31) + 1, 1 << 32, (1 << 32) + 1, 1 << 40])
def test_list_sort_end_bit(lib, total):
    e = lib.b_end_bit(I64(total))
    assert e == bc.end_bit(total) and 1 <= e <= 32
    assert e == 32 or (1 << e) >= total                                             # every list id fits the sorted bits ...
    assert e == 1 or (1 << (e - 1)) < total                                         # ... and no bit more


def test_small_rules(lib):
    assert [lib.b_sort_serves(v) for v in (2, 2047, 2048, 2049, 131072)] == [1, 1, 1, 0, 0]     # kBucketSortMaxLists
    for v in (2, 127, 128, 129, 512, 513, 2048):
        assert lib.b_stride(v) == bc.ckeys_stride(v)
    assert [lib.b_stride(v) for v in (2, 128, 129, 2048)] == [128, 128, 256, 2048]
    n, stride = 1000003, 384
    need = 2 * n * stride
    assert lib.b_key_bytes(I64(n), stride) == need
    assert lib.b_fit(I64(n), stride, I64(need)) == 1 and lib.b_fit(I64(n), stride, I64(need - 1)) == 0   # at the budget, a byte over
    assert lib.b_fit(I64(n), stride, I64(0)) == 0 and lib.b_fit(I64(0), stride, I64(0)) == 1
    assert [lib.b_budget(I64(mb)) for mb in (0, 1, 32768)] == [0, 1 << 20, 32768 << 20]
    assert lib.b_fit(I64(10 ** 7), 2048, I64(lib.b_budget(I64(32768)))) == 0        # one 2,048-list bucket at 10 M rows: 41 GB
    for name in ("edges", "sizes"):
        bk = bc.list_table(bc.offsets(bc.TABLES[name][0]), bc.TABLES[name][1])[1]
        a, out = np.array(bk, np.int64).reshape(-1), np.zeros(len(bk) + 1, np.int64)
        lib.b_segments(_p(a), I64(len(bk)), _p(out))
        assert out.tolist() == bc.sparsify_segments(bk)
    bk = [(0, 0, n, 2, 0) for n in (0, 1, 256, 257)]
    a, out = np.array(bk, np.int64).reshape(-1), np.zeros(5, np.int64)
    lib.b_segments(_p(a), I64(4), _p(out))
    assert out.tolist() == [0, 0, 1, 2, 4]


@pytest.mark.parametrize("name", list(bc.TABLES))
def test_initial_counts(lib, name):
    sizes, n_list = bc.TABLES[name]
    off, nl = np.asarray(bc.offsets(sizes), np.int64), np.asarray(n_list, np.int32)
    base = np.asarray(bc.offsets(n_list), np.int64)
    out = np.full(int(base[-1]) + 2, -7, np.int64)
    assert lib.b_counts(_p(off), _p(nl), _p(base), I64(len(nl)), _p(out)) == base[-1] + 1
    assert out[:-1].tolist() == bc.initial_counts(off.tolist(), n_list) and out[-1] == -7
    assert sum(out[:-1].tolist()) == sum(s for s, l in zip(sizes, n_list) if l == 1)


@pytest.mark.parametrize("sizes", [[5, 0, 0, 9, 0], [0, 0], [7], [], [0, 3, 0, 0, 4]], ids=str)
def test_all_flat_list_offsets(lib, sizes):
    off, base = np.asarray(bc.offsets(sizes), np.int64), np.arange(len(sizes) + 1, dtype=np.int64)
    out = np.full(len(sizes) + 2, -7, np.int64)
    assert lib.b_flat_off(_p(off), _p(base), I64(len(sizes)), _p(out)) == len(sizes) + 1
    assert out[:-1].tolist() == bc.flat_list_off(off.tolist()) == off.tolist() and out[-1] == -7
