"""Host build of `csrc/mspparse.h` (the MSP reader's per-line functions: line kind, the split at the first ':', the peak segments
of a line and their two tokens, the Num Peaks fast form) for the CPU tests: the header the kernels include, compiled by the host
C++ compiler behind `extern "C"` entry points (`tests/hostbuild.py`'s compiler choice and flags)."""
import ctypes as C

import numpy as np

from tests.hostbuild import _p, compile_shim, have_compiler  # noqa: F401
from tests.hostbuild_mgf import _pack

SHIM = r"""
#include <stdint.h>
#include "mspparse.h"

extern "C" {

// lines: text[off[k], off[k + 1]) -> kind (MSP_*), whether the line has a ':', and the key's and the value's range inside the line
void t_msp_lines(const uint8_t* text, const int64_t* off, int64_t n, int32_t* kind, int32_t* colon, int32_t* klo, int32_t* khi,
                 int32_t* vlo, int32_t* vhi) {
    for (int64_t k = 0; k < n; ++k) {
        const uint8_t* p = text + off[k];
        int lo, hi, a, b, c, d;
        kind[k] = fal::msp_classify(p, (int)(off[k + 1] - off[k]), &lo, &hi);
        colon[k] = fal::msp_split(p, lo, hi, &a, &b, &c, &d) ? 1 : 0;
        klo[k] = a;
        khi[k] = b;
        vlo[k] = c;
        vhi[k] = d;
    }
}

// lines -> their peak segment counts, and (up to cap per line) the token ranges of every segment: tok[(k * cap + j) * 4 + {0..3}]
void t_msp_segments(const uint8_t* text, const int64_t* off, int64_t n, int cap, int32_t* count, int32_t* walked, int32_t* tok) {
    for (int64_t k = 0; k < n; ++k) {
        const uint8_t* p = text + off[k];
        const int len = (int)(off[k + 1] - off[k]);
        count[k] = fal::msp_segments(p, len);
        const int end = fal::msp_peak_end(p, 0, len);
        int pos = 0, a, b, j = 0;
        while (fal::msp_segment(p, &pos, end, &a, &b)) {
            if (j < cap) {
                int32_t* t = tok + (k * cap + j) * 4;
                int t0, t1, u0, u1;
                fal::msp_peak_tokens(p, a, b, &t0, &t1, &u0, &u1);
                t[0] = t0;
                t[1] = t1;
                t[2] = u0;
                t[3] = u1;
            }
            ++j;
        }
        walked[k] = j;
    }
}

void t_msp_counts(const uint8_t* text, const int64_t* off, int64_t n, int32_t* out, int32_t* ok) {
    for (int64_t k = 0; k < n; ++k) {
        int32_t v = 0;
        ok[k] = fal::msp_parse_count(text + off[k], (int)(off[k + 1] - off[k]), &v) ? 1 : 0;
        out[k] = v;
    }
}

}  // extern "C"
"""

BLANK, NAME, NUMPEAKS, HEADER, OTHER, KIND, LONG = 0, 1, 2, 3, 4, 7, 8


def build(tmp_dir):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "msp_shim", SHIM)
    p = C.c_void_p
    lib.t_msp_lines.argtypes = [p, p, C.c_int64, p, p, p, p, p, p]
    lib.t_msp_segments.argtypes = [p, p, C.c_int64, C.c_int, p, p, p]
    lib.t_msp_counts.argtypes = [p, p, C.c_int64, p, p]
    lib.t_msp_lines.restype = lib.t_msp_segments.restype = lib.t_msp_counts.restype = None
    return lib


def lines(lib, texts):
    """-> list of (kind, key text or None when the line has no ':', value text) per line"""
    text, off = _pack(texts)
    n = len(texts)
    kind, colon, klo, khi, vlo, vhi = (np.zeros(n, np.int32) for _ in range(6))
    lib.t_msp_lines(_p(text), _p(off), n, _p(kind), _p(colon), _p(klo), _p(khi), _p(vlo), _p(vhi))
    cut = lambda k, a, b: bytes(text[off[k] + a[k]:off[k] + b[k]]).decode("latin-1")      # noqa: E731
    return [(int(kind[k]), cut(k, klo, khi) if colon[k] else None, cut(k, vlo, vhi)) for k in range(n)]


def segments(lib, texts, cap=16):
    """-> list of (segment count, [(m/z token, intensity token)] of the walk) per line"""
    text, off = _pack(texts)
    n = len(texts)
    count, walked, tok = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, cap, 4), np.int32)
    lib.t_msp_segments(_p(text), _p(off), n, cap, _p(count), _p(walked), _p(tok))
    assert np.array_equal(count, walked)
    cut = lambda k, a, b: bytes(text[off[k] + a:off[k] + b]).decode("latin-1")            # noqa: E731
    return [(int(count[k]), [(cut(k, t[0], t[1]), cut(k, t[2], t[3])) for t in tok[k, :min(count[k], cap)]]) for k in range(n)]


def counts(lib, tokens):
    """-> (int32 values, decided bool)"""
    text, off = _pack(tokens)
    out, ok = np.zeros(len(tokens), np.int32), np.zeros(len(tokens), np.int32)
    lib.t_msp_counts(_p(text), _p(off), len(tokens), _p(out), _p(ok))
    return out, ok.astype(bool)
