"""Host build of `csrc/mgfwrite.h` (the MGF writer's number text, its length function, the entry layout and the power-of-five
tables) for the CPU tests: the header the kernels include, compiled by the host C++ compiler behind `extern "C"` entry points
(`tests/hostbuild.py`'s compiler choice and flags)."""
import ctypes as C

import numpy as np

from tests.hostbuild import _p, compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include "mgfwrite.h"

extern "C" {

int t_num_max() { return fal::kMgfNumMax; }
int t_pow5_count(int inv) { return inv ? fal::kMgfPow5InvCount : fal::kMgfPow5Count; }
void t_pow5(int inv, int i, uint64_t* lo_hi) {
    lo_hi[0] = inv ? fal::kMgfPow5Inv[i][0] : fal::kMgfPow5[i][0];
    lo_hi[1] = inv ? fal::kMgfPow5Inv[i][1] : fal::kMgfPow5[i][1];
}

// numbers: text of x[k] at out[k * stride ..], its length and what the length function says
void t_numbers(const float* x, int64_t n, int stride, uint8_t* out, int32_t* len, int32_t* len_only) {
    for (int64_t k = 0; k < n; ++k) {
        len[k] = fal::mgf_write_num(out + k * stride, x[k]);
        len_only[k] = fal::mgf_num_len(x[k]);
    }
}

int64_t t_entry_len(int64_t title_len, float pm, int32_t charge, float rt, int64_t cluster, const float* mz, const float* it, int64_t np) {
    return fal::mgf_entry_len(title_len, pm, charge, rt, cluster, mz, it, np);
}

int64_t t_entry(uint8_t* dst, const uint8_t* title, int64_t title_len, float pm, int32_t charge, float rt, int64_t cluster,
                const float* mz, const float* it, int64_t np) {
    return fal::mgf_write_entry(dst, title, title_len, pm, charge, rt, cluster, mz, it, np);
}

}  // extern "C"
"""

STRIDE = 32          # bytes per number in t_numbers' output: the bound plus guard bytes
GUARD = 0xA5


def build(tmp_dir):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "mgfwrite_shim", SHIM)
    p = C.c_void_p
    lib.t_num_max.restype = C.c_int
    lib.t_pow5_count.argtypes, lib.t_pow5_count.restype = [C.c_int], C.c_int
    lib.t_pow5.argtypes, lib.t_pow5.restype = [C.c_int, C.c_int, p], None
    lib.t_numbers.argtypes, lib.t_numbers.restype = [p, C.c_int64, C.c_int, p, p, p], None
    lib.t_entry_len.argtypes = [C.c_int64, C.c_float, C.c_int32, C.c_float, C.c_int64, p, p, C.c_int64]
    lib.t_entry_len.restype = C.c_int64
    lib.t_entry.argtypes = [p, p, C.c_int64, C.c_float, C.c_int32, C.c_float, C.c_int64, p, p, C.c_int64]
    lib.t_entry.restype = C.c_int64
    return lib


def pow5_table(lib, inv: bool):
    out = []
    w = np.zeros(2, np.uint64)
    for i in range(lib.t_pow5_count(int(inv))):
        lib.t_pow5(int(inv), i, _p(w))
        out.append(int(w[0]) | (int(w[1]) << 64))
    return out


def numbers(lib, x):
    """float32 array -> (texts as bytes, lengths the length function gives, guard bytes behind the bound intact)"""
    x = np.ascontiguousarray(x, np.float32)
    n = len(x)
    out = np.full(n * STRIDE, GUARD, np.uint8)
    ln, lo = np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.t_numbers(_p(x), n, STRIDE, _p(out), _p(ln), _p(lo))
    rows = out.reshape(n, STRIDE)
    intact = bool((rows[:, lib.t_num_max():] == GUARD).all())
    raw = out.tobytes()
    return [raw[k * STRIDE:k * STRIDE + ln[k]] for k in range(n)], lo, intact


def entry(lib, title: bytes, pm, charge, rt, cluster, mz, it):
    """one entry -> (bytes, the length function's count, guard intact)"""
    mz, it = np.ascontiguousarray(mz, np.float32), np.ascontiguousarray(it, np.float32)
    t = np.frombuffer(title + b"\x00", np.uint8).copy()
    want = int(lib.t_entry_len(len(title), pm, charge, rt, cluster, _p(mz), _p(it), len(mz)))
    buf = np.full(want + 64, GUARD, np.uint8)
    got = int(lib.t_entry(_p(buf), _p(t), len(title), pm, charge, rt, cluster, _p(mz), _p(it), len(mz)))
    return buf[:got].tobytes(), want, bool((buf[got:] == GUARD).all())
