"""Host build of `csrc/csvwrite.h` (the CSV writer's comparator, number text, quoting and row layout) for the CPU tests: the header
the kernels include, compiled by the host C++ compiler behind `extern "C"` entry points (`tests/hostbuild.py`'s compiler choice
and flags)."""
import ctypes as C

import numpy as np

from tests.hostbuild import _p, compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include "csvwrite.h"

extern "C" {

int t_num_max() { return fal::kCsvNumMax; }
int t_fixed_max() { return fal::kCsvFixedMax; }

// numbers: text of x[k] at out[k * stride ..], its length and what the length function says
void t_numbers(const float* x, int64_t n, int stride, uint8_t* out, int32_t* len, int32_t* len_only) {
    for (int64_t k = 0; k < n; ++k) {
        len[k] = fal::csv_write_num(out + k * stride, x[k]);
        len_only[k] = fal::csv_num_len(x[k]);
    }
}

// every ordered pair (i, j) of the strings -> cmp[i * n + j]
void t_cmp_all(const uint8_t* blob, const int64_t* ptr, int64_t n, int32_t* cmp) {
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j)
            cmp[i * n + j] = fal::csv_natural_cmp(blob + ptr[i], ptr[i + 1] - ptr[i], blob + ptr[j], ptr[j + 1] - ptr[j]);
}

int64_t t_max_digit_run(const uint8_t* a, int64_t n) { return fal::csv_max_digit_run(a, n); }

int64_t t_row_len(const uint8_t* fn, int64_t fn_n, const uint8_t* id, int64_t id_n, int32_t charge, float pm, float rt, int64_t cluster,
                  int quote_cr) {
    return fal::csv_row_len(fal::csv_row(fn, fn_n, id, id_n, charge, pm, rt, cluster, quote_cr != 0));
}

int64_t t_row(uint8_t* dst, const uint8_t* fn, int64_t fn_n, const uint8_t* id, int64_t id_n, int32_t charge, float pm, float rt,
              int64_t cluster, int quote_cr) {
    return fal::csv_write_row(dst, fal::csv_row(fn, fn_n, id, id_n, charge, pm, rt, cluster, quote_cr != 0));
}

}  // extern "C"
"""

STRIDE = 32          # bytes per number in t_numbers' output: the bound plus guard bytes
GUARD = 0xA5


def build(tmp_dir):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "csvwrite_shim", SHIM)
    p = C.c_void_p
    lib.t_num_max.restype = C.c_int
    lib.t_fixed_max.restype = C.c_int
    lib.t_numbers.argtypes, lib.t_numbers.restype = [p, C.c_int64, C.c_int, p, p, p], None
    lib.t_cmp_all.argtypes, lib.t_cmp_all.restype = [p, p, C.c_int64, p], None
    lib.t_max_digit_run.argtypes, lib.t_max_digit_run.restype = [p, C.c_int64], C.c_int64
    lib.t_row_len.argtypes = [p, C.c_int64, p, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_int64, C.c_int]
    lib.t_row_len.restype = C.c_int64
    lib.t_row.argtypes = [p, p, C.c_int64, p, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_int64, C.c_int]
    lib.t_row.restype = C.c_int64
    return lib


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


def _bytes(b: bytes):
    return np.frombuffer(b + b"\x00", np.uint8).copy()


def cmp_all(lib, strings):
    """ASCII strings -> int32[n, n] of csv_natural_cmp over every ordered pair"""
    raw = [s.encode("ascii") for s in strings]
    ptr = np.zeros(len(raw) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in raw])
    blob = _bytes(b"".join(raw))
    out = np.zeros((len(raw), len(raw)), np.int32)
    lib.t_cmp_all(_p(blob), _p(ptr), len(raw), _p(out))
    return out


def max_digit_run(lib, s: bytes) -> int:
    return int(lib.t_max_digit_run(_p(_bytes(s)), len(s)))


def row(lib, fn: bytes, ident: bytes, charge, pm, rt, cluster, quote_cr):
    """one row -> (bytes, the length function's count, guard intact)"""
    f, i = _bytes(fn), _bytes(ident)
    want = int(lib.t_row_len(_p(f), len(fn), _p(i), len(ident), charge, pm, rt, cluster, int(quote_cr)))
    buf = np.full(want + 64, GUARD, np.uint8)
    got = int(lib.t_row(_p(buf), _p(f), len(fn), _p(i), len(ident), charge, pm, rt, cluster, int(quote_cr)))
    return buf[:got].tobytes(), want, bool((buf[got:] == GUARD).all())
