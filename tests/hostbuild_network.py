"""Host build of `csrc/netmatch.h` for the CPU tests: the header the kernels of network.hip include, compiled with the host C++
compiler behind `extern "C"` entry points that run the whole rule -- order, scope, walks, greedy matching, sum, edge rule, mutual
top-k -- with the header's functions.  Compiler discovery and flags as in tests/hostbuild.py (`-ffp-contract=off`)."""
import ctypes as C

import numpy as np

from tests.hostbuild import compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "netmatch.h"

namespace {

struct Edge { int32_t u, v; float sim; int32_t matched; };

// the greedy matching of one pair with the header's order: every round the first free candidate in (w, i, j) order
void greedy(const float* amz, const float* ait, int la, const float* bmz, const float* bit, int lb, float shift, double tol,
            double* score_out, int* matched_out) {
    std::vector<int> z0(la), z1(la), s0(la), s1(la);
    for (int i = 0; i < la; ++i) {
        fal::net_window(amz[i], bmz, lb, tol, &z0[i], &z1[i]);
        fal::net_window(amz[i] - shift, bmz, lb, tol, &s0[i], &s1[i]);
    }
    std::vector<char> used_a(la, 0), used_b(lb, 0);
    std::vector<float> got(la, 0.f);
    int matched = 0;
    for (;;) {
        bool any = false;
        float bw = 0.f;
        int bi = 0, bj = 0;
        for (int i = 0; i < la; ++i) {
            if (used_a[i]) continue;
            for (int pass = 0; pass < 2; ++pass) {
                const int q0 = pass ? std::max(s0[i], z1[i]) : z0[i], q1 = pass ? s1[i] : z1[i];
                for (int q = q0; q < q1; ++q) {
                    if (used_b[q] || !fal::net_candidate_mz(amz[i], bmz[q], shift, tol)) continue;
                    const float w = fal::net_weight(ait[i], bit[q]);
                    if (w > 0.f && (!any || fal::net_before(w, i, q, bw, bi, bj))) any = true, bw = w, bi = i, bj = q;
                }
            }
        }
        if (!any) break;
        used_a[bi] = used_b[bj] = 1;
        got[bi] = bw;
        matched += 1;
    }
    double score = 0.0;
    for (int i = 0; i < la; ++i)
        if (used_a[i]) fal::net_sum_add(score, got[i]);
    *score_out = score;
    *matched_out = matched;
}

// one oriented pair through the header's decision and, where it says so, the greedy matching above; stats[1]: pairs rejected by
// cardinality, stats[2]: pairs of the greedy kernels
fal::NetPair scored(const fal::NetOriented& o, double tol, int need, int64_t* stats) {
    fal::NetPair r = fal::net_pair(o, tol, need);
    if (r.kind != fal::NET_INLINE) stats[r.kind == fal::NET_REJECT ? 1 : 2] += 1;
    if (r.kind == fal::NET_GREEDY) {
        double score = 0.0;
        greedy(o.a.mz, o.a.it, o.a.len, o.b.mz, o.b.it, o.b.len, o.shift, tol, &score, &r.matched);
        r.sim = fal::net_similarity(score);
    }
    return r;
}

}  // namespace

extern "C" {

int t_max_peaks() { return fal::kNetMaxPeaks; }

// fal_network_edges on the host.  stats: [0] pairs in scope, [1] pairs rejected by cardinality, [2] pairs of the greedy kernel.
// -> the number of edges (written up to max_edges), or -5 when a pair in scope has a side above the peak limit
int64_t t_network(const float* mz, const float* it, const int64_t* ptr, const int32_t* rows, const float* pmz, int64_t n, double tol,
                  double max_shift, double min_cosine, int min_matched, int top_k, int32_t* eu, int32_t* ev, float* es, int32_t* em,
                  int64_t max_edges, int64_t* stats) {
    std::vector<int32_t> order(n);
    for (int64_t v = 0; v < n; ++v) order[v] = (int32_t)v;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return pmz[x] < pmz[y]; });
    std::vector<Edge> edges;
    const int need = fal::net_need(min_matched);
    stats[0] = stats[1] = stats[2] = 0;
    for (int64_t x = 0; x < n; ++x)
        for (int64_t y = x + 1; y < n; ++y) {
            const int32_t a = order[x], b = order[y];
            if (!fal::net_in_scope(pmz[a], pmz[b], max_shift)) continue;
            stats[0] += 1;
            const int64_t ga = ptr[rows[a]], gb = ptr[rows[b]];
            const int la = (int)(ptr[rows[a] + 1] - ga), lb = (int)(ptr[rows[b] + 1] - gb);
            if (la > fal::kNetMaxPeaks || lb > fal::kNetMaxPeaks) return -5;
            const fal::NetPair r = scored(fal::net_orient(fal::NetRow{mz + ga, it + ga, la, pmz[a]}, fal::NetRow{mz + gb, it + gb, lb, pmz[b]}),
                                          tol, need, stats);
            if (r.kind != fal::NET_REJECT && fal::net_is_edge(r.sim, r.matched, min_cosine, min_matched))
                edges.push_back(Edge{std::min(a, b), std::max(a, b), r.sim, r.matched});
        }
    std::sort(edges.begin(), edges.end(), [](const Edge& p, const Edge& q) { return p.u != q.u ? p.u < q.u : p.v < q.v; });
    std::vector<char> drop(edges.size(), 0);
    if (top_k > 0) {
        // as network.hip: every edge at its higher node, then every edge at its lower node; a stable sort by the rank key
        const size_t m = edges.size();
        std::vector<std::pair<uint64_t, uint32_t>> ent(2 * m);
        for (size_t e = 0; e < m; ++e) {
            ent[e] = {fal::net_rank_key(edges[e].v, edges[e].sim), (uint32_t)e};
            ent[m + e] = {fal::net_rank_key(edges[e].u, edges[e].sim), (uint32_t)e};
        }
        std::stable_sort(ent.begin(), ent.end(), [](const auto& p, const auto& q) { return p.first < q.first; });
        size_t start = 0;
        for (size_t k = 0; k < 2 * m; ++k) {
            if ((ent[k].first >> 32) != (ent[start].first >> 32)) start = k;
            if (k - start >= (size_t)top_k) drop[ent[k].second] = 1;
        }
    }
    int64_t out = 0;
    for (size_t e = 0; e < edges.size(); ++e) {
        if (drop[e]) continue;
        if (out < max_edges) eu[out] = edges[e].u, ev[out] = edges[e].v, es[out] = edges[e].sim, em[out] = edges[e].matched;
        out += 1;
    }
    return out;
}

}  // extern "C"
"""


def build(tmp_dir, extra_flags=()):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "network_shim", SHIM, extra_flags)
    p = C.c_void_p
    lib.t_max_peaks.restype = C.c_int
    lib.t_network.argtypes = [p, p, p, p, p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, p, p, p, p, C.c_int64, p]
    lib.t_network.restype = C.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def network(lib, nodes, fragment_tol, max_shift, min_cosine, min_matched, top_k):
    """-> ((u, v, sim, matched), stats dict), or (None, stats) when a pair in scope is above the peak limit"""
    mz, it = (np.ascontiguousarray(nodes[k], np.float32) for k in ("mz", "intensity"))
    if len(mz) == 0:
        mz, it = np.zeros(1, np.float32), np.zeros(1, np.float32)
    ptr, rows = np.ascontiguousarray(nodes["indptr"], np.int64), np.ascontiguousarray(nodes["rows"], np.int32)
    pmz = np.ascontiguousarray(nodes["precursor_mz"], np.float32)
    n = len(rows)
    cap = max(n * (n - 1) // 2, 1)
    eu, ev, em = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    es, stats = np.zeros(cap, np.float32), np.zeros(3, np.int64)
    m = lib.t_network(_p(mz), _p(it), _p(ptr), _p(rows), _p(pmz), n, float(fragment_tol), float(max_shift), float(min_cosine),
                      int(min_matched), int(top_k), _p(eu), _p(ev), _p(es), _p(em), cap, _p(stats))
    stats = dict(in_scope=int(stats[0]), rejected_cardinality=int(stats[1]), greedy_pairs=int(stats[2]))
    if m < 0:
        return None, stats
    return (eu[:m], ev[:m], es[:m], em[:m]), stats
