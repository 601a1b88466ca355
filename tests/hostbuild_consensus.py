"""Host build of `csrc/consensus.h` for the CPU tests: the header the kernels of consensus.hip include, compiled with the host
C++ compiler behind one `extern "C"` entry point that pools, sorts (by the header's key) and walks every cluster with the
header's functions.  Compiler discovery and flags as in tests/hostbuild.py (`-ffp-contract=off`: products and sums must not
fuse)."""
import ctypes as C

import numpy as np

from tests.hostbuild import compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "consensus.h"

extern "C" {

int t_cons_lds_peaks() { return fal::kConsLdsPeaks; }

// the contract of fal_consensus_spectra with room for every peak; -> peaks written
int64_t t_consensus(const float* mz, const float* it, const int64_t* ptr, int64_t n, const int32_t* labels, const int32_t* medoids,
                    int64_t nc, double tol, double q, int64_t* out_ptr, float* out_mz, float* out_it, int32_t* status) {
    std::vector<std::vector<int64_t>> members(nc);
    for (int64_t r = 0; r < n; ++r)
        if (labels[r] >= 0 && labels[r] < nc) members[labels[r]].push_back(r);
    int64_t w = 0;
    out_ptr[0] = 0;
    for (int64_t c = 0; c < nc; ++c) {
        const int64_t m = (int64_t)members[c].size();
        status[c] = 0;
        bool done = false;
        if (m == 1) {
            const int64_t r = members[c][0];
            for (int64_t j = ptr[r]; j < ptr[r + 1]; ++j, ++w) out_mz[w] = mz[j], out_it[w] = it[j];
            done = true;
        } else if (m >= 2) {
            std::vector<int64_t> pool;                       // CSR positions in (row, peak index) order
            for (int64_t r : members[c])
                for (int64_t j = ptr[r]; j < ptr[r + 1]; ++j) pool.push_back(j);
            std::stable_sort(pool.begin(), pool.end(),
                             [&](int64_t a, int64_t b) { return fal::cons_mz_key(mz[a]) < fal::cons_mz_key(mz[b]); });
            const int64_t need = fal::cons_need(q, m), first = w;
            std::vector<double> raw;
            for (size_t k = 0; k < pool.size();) {
                fal::ConsGroup g;
                size_t j = k;
                do {
                    fal::cons_group_add(g, mz[pool[j]], it[pool[j]]);
                    ++j;
                } while (j < pool.size() && !fal::cons_new_group(mz[pool[j]], mz[pool[j - 1]], tol));
                if (fal::cons_group_kept(g, m, need)) {
                    out_mz[w++] = fal::cons_group_mz(g);
                    raw.push_back(fal::cons_group_raw(g, m));
                }
                k = j;
            }
            if (!raw.empty()) {
                double norm2 = 0.0;
                for (double r : raw) fal::cons_norm_add(norm2, r);
                for (size_t k = 0; k < raw.size(); ++k) out_it[first + (int64_t)k] = fal::cons_intensity(raw[k], norm2);
                done = true;
            }
        }
        if (!done) {
            const int64_t r = medoids[c];
            if (r >= 0 && r < n)                             // (a medoid that is no row copies nothing: cons_out_counts_kernel)
                for (int64_t j = ptr[r]; j < ptr[r + 1]; ++j, ++w) out_mz[w] = mz[j], out_it[w] = it[j];
            status[c] = FAL_CONS_ST_FALLBACK;
        }
        out_ptr[c + 1] = w;
    }
    return w;
}

}  // extern "C"
"""


def build(tmp_dir, extra_flags=()):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "consensus_shim", SHIM, extra_flags)
    p = C.c_void_p
    lib.t_cons_lds_peaks.restype = C.c_int
    lib.t_consensus.argtypes = [p, p, p, C.c_int64, p, p, C.c_int64, C.c_double, C.c_double, p, p, p, p]
    lib.t_consensus.restype = C.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def consensus(lib, mz, intensity, indptr, labels, medoids, fragment_tol, min_fraction):
    """-> (indptr i64[n_clusters+1], mz f32, intensity f32, status i32[n_clusters]) of the host build"""
    mz, it = np.ascontiguousarray(mz, np.float32), np.ascontiguousarray(intensity, np.float32)
    ptr = np.ascontiguousarray(indptr, np.int64)
    labels, medoids = np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(medoids, np.int32)
    # room: every peak once, and once more the medoid's of a cluster that falls back to a row of another cluster
    inside = medoids[(medoids >= 0) & (medoids < len(labels))]
    nc, cap = len(medoids), max(len(mz) + int(np.diff(ptr)[inside].sum()), 1)
    out_ptr, out_mz, out_it = np.zeros(nc + 1, np.int64), np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    status = np.zeros(max(nc, 1), np.int32)
    w = lib.t_consensus(_p(mz), _p(it), _p(ptr), len(labels), _p(labels), _p(medoids), nc, float(fragment_tol),
                        float(min_fraction), _p(out_ptr), _p(out_mz), _p(out_it), _p(status))
    return out_ptr, out_mz[:w], out_it[:w], status[:nc]
