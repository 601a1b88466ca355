"""Host build of `csrc/numpress.h` (the MS-Numpress decoders of the peak-file decode kernel) and of `csrc/inflate.h`'s
upper-bound form for the CPU tests, as `hostbuild.py` builds `inflate.h`: the headers the kernels include, compiled with the
host C++ compiler into a small shared object behind `extern "C"` entry points.  `-ffp-contract=off` as in the library's build."""
import ctypes as C

import numpy as np

from tests.hostbuild import _p, compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include "inflate.h"
#include "numpress.h"

extern "C" {

int t_numpress(int64_t codec, const uint8_t* in, int64_t len, double* out, int64_t count, int64_t* n_out) {
    return fal::numpress_decode(codec, in, len, out, count, n_out);
}

int64_t t_numpress_max_bytes(int64_t codec, int64_t count) { return fal::numpress_max_bytes(codec, count); }

int t_inflate_upto(const uint8_t* in, int64_t in_len, uint8_t* out, int64_t out_cap, int exact, int64_t* out_len) {
    fal::HuffLds h;
    return fal::inflate_stream_upto(in, in_len, out, out_cap, exact != 0, out_len, h);
}

}  // extern "C"
"""

GUARD = 8                     # float64 slots behind the output


def build(tmp_dir):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "numpress_shim", SHIM)
    p = C.c_void_p
    lib.t_numpress.argtypes = [C.c_int64, p, C.c_int64, p, C.c_int64, p]
    lib.t_numpress.restype = C.c_int
    lib.t_numpress_max_bytes.argtypes = [C.c_int64, C.c_int64]
    lib.t_numpress_max_bytes.restype = C.c_int64
    lib.t_inflate_upto.argtypes = [p, C.c_int64, p, C.c_int64, C.c_int, p]
    lib.t_inflate_upto.restype = C.c_int
    return lib


def _src(data: bytes):
    """the stream in a buffer of exactly its length (a read behind it lands outside the array)"""
    return np.frombuffer(data, np.uint8).copy() if len(data) else np.zeros(0, np.uint8)


def decode(lib, codec: int, data: bytes, count: int):
    """-> (status, values written f64[n], guard slots behind out[count] intact?)"""
    src = _src(data)
    buf = np.frombuffer(b"\xa5" * (8 * (count + GUARD)), np.float64).copy()
    n = C.c_int64(-1)
    st = lib.t_numpress(int(codec), _p(src) if len(src) else None, len(src), _p(buf), int(count), C.byref(n))
    assert 0 <= n.value <= count
    return st, buf[:n.value].copy(), bool((buf[count:].view(np.uint8) == 0xA5).all() and (buf[n.value:count].view(np.uint8) == 0xA5).all())


def inflate_upto(lib, data: bytes, out_cap: int, exact: bool, guard: int = 64):
    """-> (status, reported length, output bytes [out_cap], guard bytes intact?)"""
    src = _src(data)
    buf = np.full(out_cap + guard, 0xA5, np.uint8)
    n = C.c_int64(-1)
    st = lib.t_inflate_upto(_p(src) if len(src) else None, len(src), _p(buf), int(out_cap), int(exact), C.byref(n))
    return st, n.value, buf[:out_cap].tobytes(), bool((buf[out_cap:] == 0xA5).all())
