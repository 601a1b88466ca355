"""Host build of `csrc/assignrep.h` for the CPU tests: the header the kernels of assignrep.hip include, compiled with the host
C++ compiler behind `extern "C"` entry points.  Compiler discovery and flags as in tests/hostbuild.py (`-ffp-contract=off`:
the float32 difference and division must not fuse)."""
import ctypes as C

import numpy as np

from tests.hostbuild import compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "assignrep.h"
#include "peakmatch.h"

extern "C" {

void t_candidates(const float* q_pmz, const float* l_pmz, const float* q_rt, const float* l_rt, int64_t n, double tol, int is_da,
                  int has_rt, double rt_tol, int32_t* out) {
    for (int64_t k = 0; k < n; ++k) out[k] = fal::as_candidate(q_pmz[k], l_pmz[k], tol, is_da, has_rt != 0, q_rt[k], l_rt[k], rt_tol);
}

int t_window(float q_min, float q_max, double tol, int is_da, double* lo, double* hi) {
    return fal::as_window(q_min, q_max, tol, is_da, lo, hi) ? 1 : 0;
}

void t_pack(const float* d, const uint32_t* pos, int64_t n, uint64_t* keys) {
    for (int64_t k = 0; k < n; ++k) keys[k] = fal::as_pack(d[k], pos[k]);
}

void t_unpack(const uint64_t* keys, int64_t n, float* d, uint32_t* pos) {
    for (int64_t k = 0; k < n; ++k) d[k] = fal::as_key_dist(keys[k]), pos[k] = fal::as_key_pos(keys[k]);
}

uint64_t t_empty_key() { return fal::kAsEmptyKey; }

// fal_assign_nearest's walk on the host, through the header's functions: both sides in stable precursor order, tiles of `tile`
// sorted queries, the library range of as_window found by binary search, the per-pair test, pair_score, the minimum of the keys.
// -> 0, or 1 when a scored pair has a component beyond the solver
int t_assign(const float* q_mz, const float* q_it, const int64_t* q_ptr, const float* q_pmz, const float* q_rt, int64_t nq,
             const float* l_mz, const float* l_it, const int64_t* l_ptr, const float* l_pmz, const float* l_rt, int64_t nl, double tol,
             int is_da, double rt_tol, double fragment_tol, int min_matches, int tile, int32_t* best_row, float* best_dist,
             int32_t* n_cand, int64_t* walked) {
    auto order_of = [](const float* pmz, int64_t n) {
        std::vector<int64_t> o(n);
        std::iota(o.begin(), o.end(), 0);
        std::stable_sort(o.begin(), o.end(), [&](int64_t a, int64_t b) { return pmz[a] < pmz[b]; });
        return o;
    };
    const std::vector<int64_t> qo = order_of(q_pmz, nq), lo_ = order_of(l_pmz, nl);
    std::vector<float> ls(nl);
    for (int64_t i = 0; i < nl; ++i) ls[i] = l_pmz[lo_[i]];
    int err = 0;
    *walked = 0;
    for (int64_t t0 = 0; t0 < nq; t0 += tile) {
        const int64_t t1 = std::min<int64_t>(nq, t0 + tile);
        double lo = 0.0, hi = 0.0;
        int64_t a = 0, b = nl;
        if (fal::as_window(q_pmz[qo[t0]], q_pmz[qo[t1 - 1]], tol, is_da, &lo, &hi)) {
            a = std::lower_bound(ls.begin(), ls.end(), lo, [](float v, double x) { return (double)v < x; }) - ls.begin();
            b = std::upper_bound(ls.begin(), ls.end(), hi, [](double x, float v) { return x < (double)v; }) - ls.begin();
            b = std::max(a, b);
        }
        *walked += (t1 - t0) * (b - a);
        for (int64_t s = t0; s < t1; ++s) {
            const int64_t q = qo[s];
            uint64_t best = fal::kAsEmptyKey;
            int32_t cnt = 0;
            for (int64_t pos = a; pos < b; ++pos) {
                const int64_t l = lo_[pos];
                if (!fal::as_candidate(q_pmz[q], l_pmz[l], tol, is_da, q_rt && l_rt, q_rt ? q_rt[q] : 0.f, l_rt ? l_rt[l] : 0.f, rt_tol))
                    continue;
                ++cnt;
                const fal::PeakLists pl{q_mz + q_ptr[q], q_it + q_ptr[q], l_mz + l_ptr[l], l_it + l_ptr[l]};
                double score = 0.0;
                int nm = 0;
                if (!fal::pair_score(pl, (int)(q_ptr[q + 1] - q_ptr[q]), (int)(l_ptr[l + 1] - l_ptr[l]), fragment_tol, &score, &nm)) err = 1;
                best = std::min(best, fal::as_pack((float)fal::pair_distance(score, nm, min_matches), (uint32_t)pos));
            }
            n_cand[q] = cnt;
            best_row[q] = best == fal::kAsEmptyKey ? -1 : (int32_t)lo_[fal::as_key_pos(best)];
            best_dist[q] = best == fal::kAsEmptyKey ? 1.0f : fal::as_key_dist(best);
        }
    }
    return err;
}

}  // extern "C"
"""


def build(tmp_dir, extra_flags=()):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "assign_shim", SHIM, extra_flags)
    p = C.c_void_p
    lib.t_candidates.argtypes = [p, p, p, p, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_double, p]
    lib.t_candidates.restype = None
    lib.t_window.argtypes = [C.c_float, C.c_float, C.c_double, C.c_int, p, p]
    lib.t_window.restype = C.c_int
    lib.t_pack.argtypes = [p, p, C.c_int64, p]
    lib.t_pack.restype = None
    lib.t_unpack.argtypes = [p, C.c_int64, p, p]
    lib.t_unpack.restype = None
    lib.t_empty_key.restype = C.c_uint64
    lib.t_assign.argtypes = [p] * 5 + [C.c_int64] + [p] * 5 + [C.c_int64, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                                              p, p, p, p]
    lib.t_assign.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def candidates(lib, q_pmz, l_pmz, tol, mode, rt_tol=None, q_rt=None, l_rt=None):
    """the header's per-pair test of pairs (q_pmz[k], l_pmz[k]) -> bool[n]"""
    q_pmz, l_pmz = np.ascontiguousarray(q_pmz, np.float32), np.ascontiguousarray(l_pmz, np.float32)
    n = len(q_pmz)
    q_rt = np.zeros(n, np.float32) if q_rt is None else np.ascontiguousarray(q_rt, np.float32)
    l_rt = np.zeros(n, np.float32) if l_rt is None else np.ascontiguousarray(l_rt, np.float32)
    out = np.zeros(n, np.int32)
    lib.t_candidates(_p(q_pmz), _p(l_pmz), _p(q_rt), _p(l_rt), n, float(tol), int(mode == "Da"), int(rt_tol is not None),
                     -1.0 if rt_tol is None else float(rt_tol), _p(out))
    return out.astype(bool)


def window(lib, q_min, q_max, tol, mode):
    """-> (lo, hi) of the library precursors that may hold candidates, or None (the whole library)"""
    lo, hi = C.c_double(), C.c_double()
    ok = lib.t_window(float(q_min), float(q_max), float(tol), int(mode == "Da"), C.byref(lo), C.byref(hi))
    return (lo.value, hi.value) if ok else None


def pack(lib, d, pos):
    d, pos = np.ascontiguousarray(d, np.float32), np.ascontiguousarray(pos, np.uint32)
    keys = np.zeros(len(d), np.uint64)
    lib.t_pack(_p(d), _p(pos), len(d), _p(keys))
    return keys


def unpack(lib, keys):
    keys = np.ascontiguousarray(keys, np.uint64)
    d, pos = np.zeros(len(keys), np.float32), np.zeros(len(keys), np.uint32)
    lib.t_unpack(_p(keys), len(keys), _p(d), _p(pos))
    return d, pos


def assign(lib, q, l, tol, mode, rt_tol, fragment_tol, min_matches, tile=64):
    """the host build of the kernels' walk over two sides (tests/assign_cases.py) -> (best_row, best_dist, n_cand, unsupported,
    pairs inside the pre-filter ranges)"""
    def arrays(d):
        mz, it = np.ascontiguousarray(d["mz"], np.float32), np.ascontiguousarray(d["intensity"], np.float32)
        if len(mz) == 0:
            mz, it = np.zeros(1, np.float32), np.zeros(1, np.float32)
        return (mz, it, np.ascontiguousarray(d["indptr"], np.int64), np.ascontiguousarray(d["precursor_mz"], np.float32),
                np.ascontiguousarray(d["retention_time"], np.float32))
    qa, la = arrays(q), arrays(l)
    nq, nl = len(qa[3]), len(la[3])
    row, dist, cand = np.zeros(nq, np.int32), np.zeros(nq, np.float32), np.zeros(nq, np.int32)
    walked = np.zeros(1, np.int64)
    ptrs = lambda a: [_p(x) if len(x) else None for x in a[:4]] + [_p(a[4]) if rt_tol is not None and len(a[4]) else None]
    err = lib.t_assign(*ptrs(qa), nq, *ptrs(la), nl, float(tol), int(mode == "Da"), -1.0 if rt_tol is None else float(rt_tol),
                       float(fragment_tol), int(min_matches), int(tile), _p(row), _p(dist), _p(cand), _p(walked))
    return row, dist, cand, bool(err), int(walked[0])
