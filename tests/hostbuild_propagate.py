"""Host build of `csrc/netpropagate.h` for the CPU tests: the header the kernels of propagate.hip include, compiled with the host
C++ compiler behind one `extern "C"` entry point that runs the whole rule sequentially -- the checks, level 0, and per level the
offers of every link (the greatest key of a node) and then the commits -- with the header's functions.  Compiler discovery and
flags as in tests/hostbuild.py."""
import ctypes as C

import numpy as np

from tests.hostbuild import compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include <vector>
#include "netpropagate.h"

extern "C" {

// fal_network_propagate on the host -> 0, or -1 (FAL_EINVAL) with nothing written.  counts: [0] nodes reached, [1] levels
int t_propagate(const int32_t* eu, const int32_t* ev, const float* es, int64_t m, int64_t n, const int32_t* seed, int max_hops,
                double min_score, int32_t* source, int32_t* hops, int32_t* parent, float* score, int64_t* counts) {
    if (!fal::prop_valid_hops(max_hops) || !fal::prop_valid_min_score(min_score)) return -1;
    for (int64_t e = 0; e < m; ++e)
        if (!fal::prop_valid_edge(eu[e], ev[e], es[e], n)) return -1;
    for (int64_t i = 0; i < n; ++i)
        if (!fal::prop_valid_seed(seed[i])) return -1;
    for (int64_t i = 0; i < n; ++i) {
        const bool annotated = seed[i] >= 0;
        hops[i] = annotated ? 0 : -1, source[i] = annotated ? (int32_t)i : -1, parent[i] = -1, score[i] = annotated ? 1.0f : 0.0f;
    }
    std::vector<unsigned long long> key(n, 0ull);
    int64_t reached = 0, levels = 0;
    for (int d = 1; d <= max_hops; ++d) {
        bool pending = false;
        for (int64_t e = 0; e < m; ++e) {
            int32_t a, b;
            if (hops[eu[e]] == d - 1 && hops[ev[e]] == -1) a = eu[e], b = ev[e];
            else if (hops[ev[e]] == d - 1 && hops[eu[e]] == -1) a = ev[e], b = eu[e];
            else continue;
            const float c = fal::prop_candidate(score[a], es[e]);
            if (!fal::prop_counts(c, min_score)) continue;
            const unsigned long long k = fal::prop_key(c, a);
            if (k > key[b]) key[b] = k;
            pending = true;
        }
        if (!pending) break;
        for (int64_t i = 0; i < n; ++i) {
            if (hops[i] != -1 || key[i] == 0ull) continue;
            const int32_t a = fal::prop_key_parent(key[i]);
            hops[i] = d, parent[i] = a, source[i] = source[a], score[i] = fal::prop_key_score(key[i]);
            reached += 1;
        }
        levels = d;
    }
    counts[0] = reached, counts[1] = levels;
    return 0;
}

}  // extern "C"
"""


def build(tmp_dir, extra_flags=()):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "propagate_shim", SHIM, extra_flags)
    p = C.c_void_p
    lib.t_propagate.argtypes = [p, p, p, C.c_int64, C.c_int64, p, C.c_int, C.c_double, p, p, p, p, p]
    lib.t_propagate.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


MARK = -7


def propagate(lib, g, seed, max_hops, min_score):
    """-> dict like tests/propagate_cases.propagate (source, hops, parent, score, n_reached, n_levels), or None when the call
    refused its input -- every output is then still the marker it was filled with"""
    u, v = np.ascontiguousarray(g["u"], np.int32), np.ascontiguousarray(g["v"], np.int32)
    sim, seed = np.ascontiguousarray(g["sim"], np.float32), np.ascontiguousarray(seed, np.int32)
    n, m = int(g["n"]), len(u)
    source, hops, parent = (np.full(max(n, 1), MARK, np.int32) for _ in range(3))
    score = np.full(max(n, 1), MARK, np.float32)
    counts = np.full(2, MARK, np.int64)
    rc = lib.t_propagate(_p(u), _p(v), _p(sim), m, n, _p(seed), int(max_hops), float(min_score), _p(source), _p(hops), _p(parent),
                         _p(score), _p(counts))
    if rc != 0:
        assert rc == -1 and all((a == MARK).all() for a in (source, hops, parent, score, counts))
        return None
    return dict(source=source[:n], hops=hops[:n], parent=parent[:n], score=score[:n], n_reached=int(counts[0]), n_levels=int(counts[1]))
