"""Host build of `csrc/mgfparse.h` (the MGF reader's per-line functions: number conversion, line classifier, header key, CHARGE
fast form) for the CPU tests: the header the kernels include, compiled by the host C++ compiler behind `extern "C"` entry points
(`tests/hostbuild.py`'s compiler choice and flags, `-ffp-contract=off` included)."""
import ctypes as C

import numpy as np

from tests.hostbuild import _p, compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include "mgfparse.h"

extern "C" {

int t_max_line() { return fal::kMgfMaxLine; }

// tokens: text[off[k], off[k + 1]) -> value bits and decided flag
void t_parse_doubles(const uint8_t* text, const int64_t* off, int64_t n, double* out, int32_t* ok) {
    for (int64_t k = 0; k < n; ++k) {
        double v = 0.0;
        ok[k] = fal::mgf_parse_double(text + off[k], (int)(off[k + 1] - off[k]), &v) ? 1 : 0;
        out[k] = v;
    }
}

void t_parse_charges(const uint8_t* text, const int64_t* off, int64_t n, int32_t* out, int32_t* ok) {
    for (int64_t k = 0; k < n; ++k) {
        int32_t v = 0;
        ok[k] = fal::mgf_parse_charge(text + off[k], (int)(off[k + 1] - off[k]), &v) ? 1 : 0;
        out[k] = v;
    }
}

// lines: kind (MGF_*), and for a header line its key (MGF_KEY_*) and the value's range inside the line
void t_classify(const uint8_t* text, const int64_t* off, int64_t n, int32_t* kind, int32_t* key, int32_t* vlo, int32_t* vhi) {
    for (int64_t k = 0; k < n; ++k) {
        int lo, hi;
        kind[k] = fal::mgf_classify(text + off[k], (int)(off[k + 1] - off[k]), &lo, &hi);
        key[k] = -1;
        vlo[k] = vhi[k] = 0;
        if ((kind[k] & fal::MGF_KIND) == fal::MGF_HEADER) {
            int a, b;
            key[k] = fal::mgf_header(text + off[k], lo, hi, &a, &b);
            vlo[k] = a;
            vhi[k] = b;
        }
    }
}

}  // extern "C"
"""

SKIP, BEGIN, END, HEADER, PEAK, KIND, LONG = 0, 1, 2, 3, 4, 7, 8
KEYS = {0: None, 1: "title", 2: "pepmass", 3: "charge", 4: "rtinseconds"}


def build(tmp_dir):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "mgf_shim", SHIM)
    p = C.c_void_p
    lib.t_max_line.restype = C.c_int
    lib.t_parse_doubles.argtypes = [p, p, C.c_int64, p, p]
    lib.t_parse_charges.argtypes = [p, p, C.c_int64, p, p]
    lib.t_classify.argtypes = [p, p, C.c_int64, p, p, p, p]
    for fn in (lib.t_parse_doubles, lib.t_parse_charges, lib.t_classify):
        fn.restype = None
    return lib


def _pack(tokens):
    """byte strings -> (u8 text with a guard byte, i64 offsets)"""
    raw = [t if isinstance(t, bytes) else t.encode("latin-1") for t in tokens]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(t) for t in raw], out=off[1:])
    return np.frombuffer(b"".join(raw) + b"\xa5", np.uint8).copy(), off


def parse_doubles(lib, tokens):
    """-> (float64 values, decided bool)"""
    text, off = _pack(tokens)
    out, ok = np.zeros(len(tokens)), np.zeros(len(tokens), np.int32)
    lib.t_parse_doubles(_p(text), _p(off), len(tokens), _p(out), _p(ok))
    return out, ok.astype(bool)


def parse_charges(lib, tokens):
    text, off = _pack(tokens)
    out, ok = np.zeros(len(tokens), np.int32), np.zeros(len(tokens), np.int32)
    lib.t_parse_charges(_p(text), _p(off), len(tokens), _p(out), _p(ok))
    return out, ok.astype(bool)


def classify(lib, lines):
    """-> list of (kind, key name or None, value text or None) per line"""
    text, off = _pack(lines)
    n = len(lines)
    kind, key, vlo, vhi = (np.zeros(n, np.int32) for _ in range(4))
    lib.t_classify(_p(text), _p(off), n, _p(kind), _p(key), _p(vlo), _p(vhi))
    out = []
    for k in range(n):
        if (kind[k] & KIND) == HEADER:
            raw = bytes(text[off[k] + vlo[k]:off[k] + vhi[k]]).decode("latin-1")
            out.append((int(kind[k]), KEYS[int(key[k])], raw))
        else:
            out.append((int(kind[k]), None, None))
    return out
