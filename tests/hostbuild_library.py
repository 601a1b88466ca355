"""Host build of `csrc/libsearch.h` + `csrc/netmatch.h` for the CPU tests: the headers the kernels of libsearch.hip include,
compiled with the host C++ compiler behind `extern "C"` entry points that run the whole rule -- scope, orientation, walks, greedy
matching, sum, hit rule, top-n -- with the headers' functions.  The greedy matching and the scoring of an oriented pair are
tests/hostbuild_network.py's; compiler discovery and flags as in tests/hostbuild.py (`-ffp-contract=off`)."""
import ctypes as C

import numpy as np

from tests import hostbuild_network as hbn
from tests.hostbuild import compile_shim, have_compiler  # noqa: F401

SHIM = hbn.SHIM.split('extern "C" {')[0] + r"""
#include "libsearch.h"

namespace {
struct Hit { int32_t q, l; float sim; int32_t matched; };
}

extern "C" {

int t_in_scope(float pq, float pl, int analog, double precursor_tol, int tol_is_da, double max_shift) {
    return fal::lib_in_scope(pq, pl, analog, precursor_tol, tol_is_da, max_shift);
}
int t_query_is_a(float pq, float pl) { return fal::lib_query_is_a(pq, pl); }
float t_shift(int analog, float pa, float pb) { return fal::lib_shift(analog, pa, pb); }
int t_window(float q_min, float q_max, int analog, double precursor_tol, int tol_is_da, double max_shift, double* lo, double* hi) {
    return fal::lib_window(q_min, q_max, analog, precursor_tol, tol_is_da, max_shift, lo, hi);
}

// fal_library_search on the host.  stats: [0] pairs in scope, [1] pairs rejected by cardinality, [2] pairs of the greedy kernels,
// [3] pairs in scope outside lib_window's range of their own query (0: the range is a superset).
// -> the number of hits (written up to max_hits), or -5 when a pair in scope has a side above the peak limit
int64_t t_library(const float* qmz, const float* qit, const int64_t* qptr, const int32_t* qrows, const float* qp, int64_t nq,
                  const float* lmz, const float* lit, const int64_t* lptr, const int32_t* lrows, const float* lp, int64_t nl,
                  double tol, double precursor_tol, int tol_is_da, int analog, double max_shift, double min_cosine, int min_matched,
                  int top_n, int32_t* hq, int32_t* hl, float* hs, int32_t* hm, int64_t max_hits, int64_t* stats) {
    std::vector<Hit> hits;
    const int need = fal::net_need(min_matched);
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    for (int64_t x = 0; x < nq; ++x)
        for (int64_t y = 0; y < nl; ++y) {
            if (!fal::lib_in_scope(qp[x], lp[y], analog, precursor_tol, tol_is_da, max_shift)) continue;
            stats[0] += 1;
            double lo = 0.0, hi = 0.0;
            if (fal::lib_window(qp[x], qp[x], analog, precursor_tol, tol_is_da, max_shift, &lo, &hi) &&
                !((double)lp[y] >= lo && (double)lp[y] <= hi))
                stats[3] += 1;
            const int64_t gq = qptr[qrows[x]], gl = lptr[lrows[y]];
            const int lq = (int)(qptr[qrows[x] + 1] - gq), ll = (int)(lptr[lrows[y] + 1] - gl);
            if (lq > fal::kNetMaxPeaks || ll > fal::kNetMaxPeaks) return -5;
            const fal::NetPair r = scored(fal::lib_orient(analog, fal::NetRow{qmz + gq, qit + gq, lq, qp[x]},
                                                          fal::NetRow{lmz + gl, lit + gl, ll, lp[y]}), tol, need, stats);
            if (r.kind != fal::NET_REJECT && fal::net_is_edge(r.sim, r.matched, min_cosine, min_matched))
                hits.push_back(Hit{(int32_t)x, (int32_t)y, r.sim, r.matched});
        }
    // as libsearch.hip: the hits in (query, library) order, then a stable sort by the rank key
    std::sort(hits.begin(), hits.end(), [](const Hit& p, const Hit& q) { return p.q != q.q ? p.q < q.q : p.l < q.l; });
    std::stable_sort(hits.begin(), hits.end(),
                     [](const Hit& p, const Hit& q) { return fal::net_rank_key(p.q, p.sim) < fal::net_rank_key(q.q, q.sim); });
    int64_t out = 0;
    size_t start = 0;
    for (size_t k = 0; k < hits.size(); ++k) {
        if (hits[k].q != hits[start].q) start = k;
        if (top_n > 0 && k - start >= (size_t)top_n) continue;
        if (out < max_hits) hq[out] = hits[k].q, hl[out] = hits[k].l, hs[out] = hits[k].sim, hm[out] = hits[k].matched;
        out += 1;
    }
    return out;
}

}  // extern "C"
"""


def build(tmp_dir, extra_flags=()):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "library_shim", SHIM, extra_flags)
    p, d, i, f = C.c_void_p, C.c_double, C.c_int, C.c_float
    lib.t_in_scope.argtypes = [f, f, i, d, i, d]
    lib.t_in_scope.restype = i
    lib.t_query_is_a.argtypes = [f, f]
    lib.t_query_is_a.restype = i
    lib.t_shift.argtypes = [i, f, f]
    lib.t_shift.restype = f
    lib.t_window.argtypes = [f, f, i, d, i, d, p, p]
    lib.t_window.restype = i
    lib.t_library.argtypes = [p, p, p, p, p, C.c_int64, p, p, p, p, p, C.c_int64, d, d, i, i, d, d, i, i, p, p, p, p, C.c_int64, p]
    lib.t_library.restype = C.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _side(s):
    mz, it = (np.ascontiguousarray(s[k], np.float32) for k in ("mz", "intensity"))
    if len(mz) == 0:
        mz, it = np.zeros(1, np.float32), np.zeros(1, np.float32)
    return [mz, it, np.ascontiguousarray(s["indptr"], np.int64), np.ascontiguousarray(s["rows"], np.int32),
            np.ascontiguousarray(s["precursor_mz"], np.float32)]


def window(lib, q_min, q_max, r):
    """-> (lo, hi) of lib_window, or None when the range is the whole library"""
    lo, hi = C.c_double(), C.c_double()
    ok = lib.t_window(float(q_min), float(q_max), int(r["analog"]), r["precursor_tol"], int(r["tol_is_da"]), r["max_shift"],
                      C.byref(lo), C.byref(hi))
    return (lo.value, hi.value) if ok else None


def search(lib, q, l, fragment_tol, r, min_cosine, min_matched, top_n):
    """-> ((query, library, sim, matched), stats dict), or (None, stats) when a pair in scope is above the peak limit"""
    qa, la = _side(q), _side(l)
    nq, nl = len(qa[3]), len(la[3])
    cap = max(nq * nl, 1)
    hq, hl, hm = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    hs, stats = np.zeros(cap, np.float32), np.zeros(4, np.int64)
    m = lib.t_library(*(_p(a) for a in qa), nq, *(_p(a) for a in la), nl, float(fragment_tol), r["precursor_tol"], int(r["tol_is_da"]),
                      int(r["analog"]), r["max_shift"], float(min_cosine), int(min_matched), int(top_n), _p(hq), _p(hl), _p(hs), _p(hm),
                      cap, _p(stats))
    stats = dict(in_scope=int(stats[0]), rejected_cardinality=int(stats[1]), greedy_pairs=int(stats[2]), outside_window=int(stats[3]))
    if m < 0:
        return None, stats
    return (hq[:m], hl[:m], hs[:m], hm[:m]), stats
