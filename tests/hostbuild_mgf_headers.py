"""Host build of `csrc/mgfkeys.h` (the per-line functions of `fal_mgf_headers`: the table key of a header line and the integer
fast form) for the CPU tests: the header the kernel includes, compiled by the host C++ compiler behind `extern "C"` entry points
(`tests/hostbuild.py`'s compiler choice and flags)."""
import ctypes as C

import numpy as np

from tests.hostbuild import _p, compile_shim, have_compiler  # noqa: F401
from tests.hostbuild_mgf import _pack

SHIM = r"""
#include <stdint.h>
#include <string.h>
#include "mgfkeys.h"

extern "C" {

int t_max_keys() { return fal::kMgfMaxKeys; }
int t_max_key_bytes() { return fal::kMgfMaxKeyBytes; }

// lines: text[off[k], off[k + 1]) -> the index of the line's key in the table (keys back to back, key_ptr), -1: none; and the
// value's range inside the line.  Every line is taken as a header line: the classifier is mgfparse.h's and has its own tests.
void t_table_keys(const uint8_t* text, const int64_t* off, int64_t n, const uint8_t* keys, const int64_t* key_ptr, int n_keys,
                  int32_t* idx, int32_t* vlo, int32_t* vhi) {
    fal::MgfKeyTable table;
    memset(&table, 0, sizeof(table));
    table.n = n_keys;
    for (int k = 0; k < n_keys; ++k) {
        table.len[k] = (int32_t)(key_ptr[k + 1] - key_ptr[k]);
        memcpy(table.bytes[k], keys + key_ptr[k], (size_t)table.len[k]);
    }
    for (int64_t k = 0; k < n; ++k) {
        const uint8_t* p = text + off[k];
        int lo = 0, hi = (int)(off[k + 1] - off[k]), klo, khi, a, b;
        fal::mgf_strip(p, &lo, &hi);
        fal::mgf_split(p, lo, hi, &klo, &khi, &a, &b);
        idx[k] = fal::mgf_table_key(p + klo, khi - klo, table.bytes, table.len, n_keys);
        vlo[k] = a;
        vhi[k] = b;
    }
}

void t_parse_ints(const uint8_t* text, const int64_t* off, int64_t n, int64_t* out, int32_t* ok) {
    for (int64_t k = 0; k < n; ++k) {
        int64_t v = 0;
        ok[k] = fal::mgf_parse_int(text + off[k], (int)(off[k + 1] - off[k]), &v) ? 1 : 0;
        out[k] = v;
    }
}

}  // extern "C"
"""


def build(tmp_dir):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "mgf_headers_shim", SHIM)
    p = C.c_void_p
    lib.t_max_keys.restype = lib.t_max_key_bytes.restype = C.c_int
    lib.t_table_keys.argtypes = [p, p, C.c_int64, p, p, C.c_int, p, p, p]
    lib.t_parse_ints.argtypes = [p, p, C.c_int64, p, p]
    lib.t_table_keys.restype = lib.t_parse_ints.restype = None
    return lib


def table_keys(lib, lines, keys):
    """-> list of (table key or None, value text) per line, every line taken as a header line"""
    text, off = _pack(lines)
    blob, ptr = _pack(keys)
    n = len(lines)
    idx, vlo, vhi = (np.zeros(n, np.int32) for _ in range(3))
    lib.t_table_keys(_p(text), _p(off), n, _p(blob), _p(ptr), len(keys), _p(idx), _p(vlo), _p(vhi))
    return [(keys[idx[k]] if idx[k] >= 0 else None, bytes(text[off[k] + vlo[k]:off[k] + vhi[k]]).decode("latin-1")) for k in range(n)]


def parse_ints(lib, tokens):
    """-> (int64 values, decided bool)"""
    text, off = _pack(tokens)
    out, ok = np.zeros(len(tokens), np.int64), np.zeros(len(tokens), np.int32)
    lib.t_parse_ints(_p(text), _p(off), len(tokens), _p(out), _p(ok))
    return out, ok.astype(bool)
