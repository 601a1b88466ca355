"""Host build of `csrc/memberscore.h` for the CPU tests: the header the kernels of memberscore.hip include, compiled with the host
C++ compiler behind `extern "C"` entry points that walk members and clusters with the header's functions, in the header's order.
Compiler discovery and flags as in tests/hostbuild.py (`-ffp-contract=off`: the float64 sums must not fuse)."""
import ctypes as C

import numpy as np

from tests.hostbuild import compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include <vector>
#include "memberscore.h"

extern "C" {

int t_chains() { return fal::kMsChains; }

// fal_member_scores on the host: pair_score per member, the header's clip.  -> 0, or 1 when a pair is beyond the solver
int t_member_scores(const float* mz, const float* it, const int64_t* ptr, int64_t n, const int32_t* labels, int64_t nc,
                    const float* r_mz, const float* r_it, const int64_t* r_ptr, int64_t n_rep, const int32_t* rep_row, double tol,
                    float* similarity, int32_t* matched) {
    int err = 0;
    for (int64_t i = 0; i < n; ++i) {
        similarity[i] = 0.f;
        matched[i] = 0;
        if (labels[i] < 0 || labels[i] >= nc) continue;
        const int64_t r = rep_row[labels[i]];
        const bool has = r >= 0 && r < n_rep;
        const int64_t b0 = has ? r_ptr[r] : 0, nb = has ? r_ptr[r + 1] - b0 : 0;
        const fal::PeakLists s{mz + ptr[i], it + ptr[i], r_mz + b0, r_it + b0};
        double score = 0.0;
        int nm = 0;
        if (!fal::pair_score(s, (int)(ptr[i + 1] - ptr[i]), (int)nb, tol, &score, &nm)) err = 1;
        similarity[i] = fal::ms_similarity(score);
        matched[i] = nm;
    }
    return err;
}

// fal_cluster_summary on the host: every cluster's members in row order, member p on chain p mod kMsChains (one MsFold per chain,
// merged like the lanes of the wave), the chains added in order
void t_summary(const int32_t* labels, int64_t n, int64_t nc, const float* sim, const float* pmz, const float* rt, int32_t* size,
               float* sim_min, int32_t* worst_row, double* sim_mean, float* pmz_min, float* pmz_max, float* rt_min, float* rt_max) {
    std::vector<std::vector<int32_t>> members(nc);
    for (int64_t r = 0; r < n; ++r)
        if (labels[r] >= 0 && labels[r] < nc) members[labels[r]].push_back((int32_t)r);
    for (int64_t c = 0; c < nc; ++c) {
        fal::MsFold fold[fal::kMsChains];
        double chain[fal::kMsChains];
        for (int l = 0; l < fal::kMsChains; ++l) chain[l] = 0.0;
        for (size_t p = 0; p < members[c].size(); ++p) {
            const int32_t r = members[c][p];
            fal::ms_chain_add(chain[p % fal::kMsChains], sim[r]);
            fal::ms_fold_add(fold[p % fal::kMsChains], sim[r], r, pmz[r], rt ? rt[r] : 0.f);
        }
        double total = 0.0;
        fal::MsFold f;
        for (int l = 0; l < fal::kMsChains; ++l) {
            fal::ms_total_add(total, chain[l]);
            fal::ms_fold_merge(f, fold[l]);
        }
        const fal::MsRow o = fal::ms_row(f, total, (int64_t)members[c].size());
        size[c] = o.size, sim_min[c] = o.sim_min, worst_row[c] = o.worst_row, sim_mean[c] = o.sim_mean;
        pmz_min[c] = o.pmz_min, pmz_max[c] = o.pmz_max, rt_min[c] = o.rt_min, rt_max[c] = o.rt_max;
    }
}

}  // extern "C"
"""

COLUMNS = (("size", np.int32), ("sim_min", np.float32), ("worst_row", np.int32), ("sim_mean", np.float64), ("pmz_min", np.float32),
           ("pmz_max", np.float32), ("rt_min", np.float32), ("rt_max", np.float32))


def build(tmp_dir, extra_flags=()):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "memberscore_shim", SHIM, extra_flags)
    p = C.c_void_p
    lib.t_chains.restype = C.c_int
    lib.t_member_scores.argtypes = [p, p, p, C.c_int64, p, C.c_int64, p, p, p, C.c_int64, p, C.c_double, p, p]
    lib.t_member_scores.restype = C.c_int
    lib.t_summary.argtypes = [p, C.c_int64, C.c_int64] + [p] * 11
    lib.t_summary.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _csr(d):
    mz, it = np.ascontiguousarray(d["mz"], np.float32), np.ascontiguousarray(d["intensity"], np.float32)
    if len(mz) == 0:
        mz, it = np.zeros(1, np.float32), np.zeros(1, np.float32)
    return mz, it, np.ascontiguousarray(d["indptr"], np.int64)


def member_scores(lib, case, rep, rep_row, fragment_tol):
    """-> (similarity f32[n], matched i32[n], unsupported)"""
    mz, it, ptr = _csr(case)
    r_mz, r_it, r_ptr = _csr(rep)
    labels, rep_row = np.ascontiguousarray(case["labels"], np.int32), np.ascontiguousarray(rep_row, np.int32)
    n = len(labels)
    sim, matched = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32)
    err = lib.t_member_scores(_p(mz), _p(it), _p(ptr), n, _p(labels), len(rep_row), _p(r_mz), _p(r_it), _p(r_ptr), len(r_ptr) - 1,
                              _p(rep_row), float(fragment_tol), _p(sim), _p(matched))
    return sim[:n], matched[:n], bool(err)


def summary(lib, labels, n_clusters, sim, pmz, rt=None):
    """-> dict of the per-cluster columns"""
    labels, sim, pmz = (np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(sim, np.float32),
                        np.ascontiguousarray(pmz, np.float32))
    rt = None if rt is None else np.ascontiguousarray(rt, np.float32)
    out = {k: np.zeros(max(n_clusters, 1), t) for k, t in COLUMNS}
    lib.t_summary(_p(labels), len(labels), n_clusters, _p(sim), _p(pmz), _p(rt), *(_p(out[k]) for k, _ in COLUMNS))
    return {k: v[:n_clusters] for k, v in out.items()}
