"""Host build of the library's pure, shared functions for the CPU tests: `csrc/peakmatch.h` (the matched-peak cosine with its
Hungarian solver) and `csrc/inflate.h` (the zlib inflater) compiled with the host C++ compiler into a small shared object
behind `extern "C"` entry points and loaded with ctypes.  The headers are the ones the kernels include: nothing is copied.
`-ffp-contract=off` as in the library's own build (float32 products and float64 sums must not fuse)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "falcon_amd", "csrc")

SHIM = r"""
#include <stdint.h>
#include "peakmatch.h"
#include "inflate.h"

extern "C" {

int t_max_comp() { return fal::kMaxComp; }

// pair k = spectra (2k, 2k + 1) of the CSR (query first); ok[k] = 0 when a component exceeds kMaxComp
void t_pair_scores(const float* mz, const float* it, const int64_t* ptr, int64_t n_pairs, double tol, double* score, int32_t* n_match,
                   int32_t* ok) {
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int64_t a0 = ptr[2 * k], b0 = ptr[2 * k + 1], b1 = ptr[2 * k + 2];
        const fal::PeakLists s{mz + a0, it + a0, mz + b0, it + b0};
        int nm = 0;
        ok[k] = fal::pair_score(s, (int)(b0 - a0), (int)(b1 - b0), tol, &score[k], &nm) ? 1 : 0;
        n_match[k] = nm;
    }
}

double t_pair_distance(double score, int n_match, int min_matches) { return fal::pair_distance(score, n_match, min_matches); }

// the same pairs through exact_distance (sorted rows 2k < 2k + 1 of an identity order)
void t_exact_distances(const float* mz, const float* it, const int64_t* ptr, const int64_t* order, int64_t n_pairs, double tol,
                       int min_matches, double* dist, int32_t* ok) {
    fal::ExactPeaks pk{mz, it, ptr, order, tol, min_matches, nullptr};
    for (int64_t k = 0; k < n_pairs; ++k) {
        bool good = true;
        dist[k] = fal::exact_distance(pk, 2 * k, 2 * k + 1, &good);
        ok[k] = good ? 1 : 0;
    }
}

int t_inflate(const uint8_t* in, int64_t in_len, uint8_t* out, int64_t out_cap) {
    fal::HuffLds h;
    return fal::inflate_stream(in, in_len, out, out_cap, h);
}

}  // extern "C"
"""


def _compiler():
    """-> (argv prefix, is_hipcc): the host C++ compiler, else hipcc compiling the host side only; None when neither exists"""
    for cc in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cc and shutil.which(cc):
            return [shutil.which(cc)], False
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.isfile(hipcc):
        return [hipcc, "--offload-host-only", "-x", "hip"], True
    return None


def have_compiler() -> bool:
    return _compiler() is not None


def compile_shim(tmp_dir, name, source, extra_flags=()):
    """`source` written to `tmp_dir`/`name`.cpp and compiled into lib`name`.so with the host build's flags -> ctypes library"""
    cc = _compiler()
    assert cc is not None, "no host C++ compiler and no hipcc"
    src = os.path.join(str(tmp_dir), name + ".cpp")
    so = os.path.join(str(tmp_dir), "lib" + name + ".so")
    with open(src, "w") as f:
        f.write(source)
    cmd = cc[0] + ["-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, *extra_flags, src, "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr[-4000:]}"
    return C.CDLL(so)


def build(tmp_dir, extra_flags=()):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "host_shim", SHIM, extra_flags)
    p = C.c_void_p
    lib.t_max_comp.restype = C.c_int
    lib.t_pair_scores.argtypes = [p, p, p, C.c_int64, C.c_double, p, p, p]
    lib.t_pair_scores.restype = None
    lib.t_pair_distance.argtypes = [C.c_double, C.c_int, C.c_int]
    lib.t_pair_distance.restype = C.c_double
    lib.t_exact_distances.argtypes = [p, p, p, p, C.c_int64, C.c_double, C.c_int, p, p]
    lib.t_exact_distances.restype = None
    lib.t_inflate.argtypes = [p, C.c_int64, p, C.c_int64]
    lib.t_inflate.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pair_scores(lib, mz, it, ptr, tol):
    """pairs (2k, 2k + 1) of the CSR -> (score f64 before clipping, n_match i32, ok bool)"""
    mz, it = np.ascontiguousarray(mz, np.float32), np.ascontiguousarray(it, np.float32)
    ptr = np.ascontiguousarray(ptr, np.int64)
    n = (len(ptr) - 1) // 2
    score, nm, ok = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.t_pair_scores(_p(mz), _p(it), _p(ptr), n, float(tol), _p(score), _p(nm), _p(ok))
    return score, nm, ok.astype(bool)


def exact_distances(lib, mz, it, ptr, tol, min_matches):
    mz, it = np.ascontiguousarray(mz, np.float32), np.ascontiguousarray(it, np.float32)
    ptr = np.ascontiguousarray(ptr, np.int64)
    n = (len(ptr) - 1) // 2
    order = np.arange(2 * n, dtype=np.int64)
    dist, ok = np.zeros(n), np.zeros(n, np.int32)
    lib.t_exact_distances(_p(mz), _p(it), _p(ptr), _p(order), n, float(tol), int(min_matches), _p(dist), _p(ok))
    return dist, ok.astype(bool)


def inflate(lib, data: bytes, out_cap: int, guard: int = 64):
    """-> (status, output bytes [out_cap], guard bytes intact?)"""
    src = np.frombuffer(data, np.uint8) if len(data) else np.zeros(0, np.uint8)
    buf = np.full(out_cap + guard, 0xA5, np.uint8)
    st = lib.t_inflate(_p(src) if len(src) else None, len(src), _p(buf), int(out_cap))
    return st, buf[:out_cap].tobytes(), bool((buf[out_cap:] == 0xA5).all())
