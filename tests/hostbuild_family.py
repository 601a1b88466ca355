"""Host build of `csrc/netfamily.h` for the CPU tests: the header the kernels of families.hip include, compiled with the host C++
compiler behind one `extern "C"` entry point that runs the whole rule sequentially -- the edge check, a union-find per pass, the
weakest edge of every oversized component, the cuts, the numbering -- with the header's functions.  Compiler discovery and flags
as in tests/hostbuild.py."""
import ctypes as C

import numpy as np

from tests.hostbuild import compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include <vector>
#include "netfamily.h"

namespace {
int32_t find(std::vector<int32_t>& parent, int32_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
}
}  // namespace

extern "C" {

// fal_network_families on the host -> 0, or -1 (FAL_EINVAL) with nothing written.  counts: [0] families, [1] rounds, [2] edges cut
int t_families(const int32_t* eu, const int32_t* ev, const float* es, int64_t m, int64_t n, int max_size, double delta,
               int32_t* family, int32_t* size_out, int32_t* round_out, int64_t* counts) {
    if (max_size < 0 || !(delta >= 0.0)) return -1;
    for (int64_t e = 0; e < m; ++e)
        if (!fal::fam_valid_edge(eu[e], ev[e], es[e], n)) return -1;
    std::vector<int32_t> round(m, 0), parent(n), size(n);
    std::vector<uint32_t> lo(n);
    int rounds = 0;
    for (;;) {
        for (int64_t i = 0; i < n; ++i) parent[i] = (int32_t)i, size[i] = 0, lo[i] = fal::kFamNoKey;
        for (int64_t e = 0; e < m; ++e) {
            if (round[e] != 0) continue;
            int32_t a = find(parent, eu[e]), b = find(parent, ev[e]);
            if (a == b) continue;
            if (a < b) { const int32_t t = a; a = b; b = t; }
            parent[a] = b;                                        // the larger root under the smaller
        }
        for (int64_t i = 0; i < n; ++i) size[find(parent, (int32_t)i)] += 1;
        bool over = false;
        for (int64_t e = 0; e < m; ++e) {
            if (round[e] != 0) continue;
            const int32_t r = find(parent, eu[e]);
            if (!fal::fam_oversized(size[r], max_size)) continue;
            const uint32_t key = fal::fam_key(es[e]);
            if (key < lo[r]) lo[r] = key;
            over = true;
        }
        if (!over) break;
        rounds += 1;
        for (int64_t e = 0; e < m; ++e) {
            if (round[e] != 0) continue;
            const int32_t r = find(parent, eu[e]);
            if (fal::fam_oversized(size[r], max_size) && fal::fam_is_cut(es[e], lo[r], delta)) round[e] = rounds;
        }
    }
    std::vector<int32_t> rank(n);
    int32_t families = 0;
    for (int64_t i = 0; i < n; ++i) {
        rank[i] = families;
        if (parent[i] == (int32_t)i && fal::fam_is_family(size[i])) families += 1;
    }
    for (int64_t i = 0; i < n; ++i) {
        const int32_t r = find(parent, (int32_t)i);
        family[i] = fal::fam_is_family(size[r]) ? rank[r] : -1;
        size_out[i] = size[r];
    }
    int64_t cut = 0;
    for (int64_t e = 0; e < m; ++e) round_out[e] = round[e], cut += round[e] > 0;
    counts[0] = families, counts[1] = rounds, counts[2] = cut;
    return 0;
}

}  // extern "C"
"""


def build(tmp_dir, extra_flags=()):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "family_shim", SHIM, extra_flags)
    p = C.c_void_p
    lib.t_families.argtypes = [p, p, p, C.c_int64, C.c_int64, C.c_int, C.c_double, p, p, p, p]
    lib.t_families.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


MARK = -7


def families(lib, g, max_size, delta):
    """-> dict like tests/family_cases.families (family, size, round, n_families, n_rounds, n_cut), or None when the call
    refused its input -- every output is then still the marker it was filled with"""
    u, v = np.ascontiguousarray(g["u"], np.int32), np.ascontiguousarray(g["v"], np.int32)
    sim = np.ascontiguousarray(g["sim"], np.float32)
    n, m = int(g["n"]), len(u)
    family, size, rnd = np.full(max(n, 1), MARK, np.int32), np.full(max(n, 1), MARK, np.int32), np.full(max(m, 1), MARK, np.int32)
    counts = np.full(3, MARK, np.int64)
    rc = lib.t_families(_p(u), _p(v), _p(sim), m, n, int(max_size), float(delta), _p(family), _p(size), _p(rnd), _p(counts))
    if rc != 0:
        assert rc == -1 and all((a == MARK).all() for a in (family, size, rnd, counts))
        return None
    return dict(family=family[:n], size=size[:n], round=rnd[:m], n_families=int(counts[0]), n_rounds=int(counts[1]),
                n_cut=int(counts[2]))
