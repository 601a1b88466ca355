"""Host build of `csrc/mzmlscan.h` (the mzML reader's tag classifier, attribute reader and spectrum walker) for the CPU tests: the
header the kernels include, compiled by the host C++ compiler behind one `extern "C"` entry point that runs the whole scan as a
host loop -- find every '<', classify every tag, pair the spectrum markers, walk every spectrum, check the binary text
(`tests/hostbuild.py`'s compiler choice and flags).  `scan` returns what `Context.scan_mzml` returns, the payload as a host array;
`FakeContext` stands in for a device context in `mzml_io.read_chunks_device`."""
import ctypes as C

import numpy as np

from tests.hostbuild import _p, compile_shim, have_compiler  # noqa: F401

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "mzmlscan.h"

using namespace fal;

extern "C" {

// counts[4] = {spectra, tags inside spectra, flags (1 STRUCT, 2 MARKUP, 4 TAGS), tags}; the outputs have room for cap spectra;
// arrays[2 s + a] = {text position of the array's base64, its length, count, flags}
void t_mzml_scan(const uint8_t* text, int64_t n, int64_t cap, int64_t* counts, int32_t* status, int64_t* id, int64_t* span, double* pmz,
                 int32_t* charge, double* rt, int64_t* arrays) {
    std::vector<int32_t> pos;
    for (int64_t i = 0; i < n; ++i)
        if (text[i] == '<') pos.push_back((int32_t)i);
    const int64_t tags = (int64_t)pos.size();
    pos.push_back((int32_t)n);
    counts[0] = counts[1] = counts[2] = 0;
    counts[3] = tags;
    if (tags > n / 4 + 2) {
        counts[2] = 4;
        return;
    }
    std::vector<MzTag> recs(tags);
    std::vector<int32_t> opens, closes;
    int64_t flags = 0, balance = 0;
    for (int64_t k = 0; k < tags; ++k) {
        mzml_classify_tag(text + pos[k], pos[k + 1] - pos[k], pos[k], &recs[k]);
        if (recs[k].info & MZ_MARKUP) flags |= 2;
        if (mz_kind(recs[k]) == MZ_SPECTRUM && mz_form(recs[k]) == MZ_OPEN) {
            if (balance != 0) flags |= 1;
            ++balance;
            opens.push_back((int32_t)k);
        } else if (mz_kind(recs[k]) == MZ_SPECTRUM && mz_form(recs[k]) == MZ_CLOSE) {
            if (balance != 1) flags |= 1;
            --balance;
            closes.push_back((int32_t)k);
        }
    }
    if (opens.size() != closes.size()) flags |= 1;
    counts[2] = flags;
    if (flags || (int64_t)opens.size() > cap) return;
    counts[0] = (int64_t)opens.size();
    for (size_t s = 0; s < opens.size(); ++s) {
        const int64_t k0 = opens[s], k1 = closes[s];
        counts[1] += k1 - k0 - 1;
        MzSpectrum r;
        mzml_walk(text, recs.data(), pos.data(), k0, k1, &r);
        if (r.status == MZ_ST_OK) {                  // the gather's byte check: HOST keeps its place in the payload, nothing else
            for (int a = 0; a < 2; ++a)
                for (int32_t i = r.text_lo[a]; i < r.text_hi[a]; ++i)
                    if (!mzml_binary_byte(text[i])) r.status = MZ_ST_HOST;
            if (r.status != MZ_ST_OK) {
                r.id_lo = r.id_hi = r.charge = 0;
                r.pmz = r.rt = 0.0;
            }
        }
        status[s] = r.status;
        id[2 * s] = r.id_lo;
        id[2 * s + 1] = r.id_hi;
        span[2 * s] = pos[k0];
        span[2 * s + 1] = (int64_t)recs[k1].end + 1;
        pmz[s] = r.pmz;
        charge[s] = r.status == MZ_ST_OK ? r.charge : 0;
        rt[s] = r.rt;
        for (int a = 0; a < 2; ++a) {
            int64_t* row = arrays + 4 * (2 * s + a);
            row[0] = r.text_lo[a];
            row[1] = r.text_hi[a] - r.text_lo[a];
            row[2] = r.count[a];
            row[3] = r.flags[a];
        }
    }
}

}  // extern "C"
"""

FLAG_STRUCT, FLAG_MARKUP, FLAG_TAGS = 1, 2, 4
OK, SKIP, HOST = 0, 1, 2


def build(tmp_dir):
    """compile the shim into `tmp_dir` -> ctypes library with argument types set"""
    lib = compile_shim(tmp_dir, "mzml_shim", SHIM)
    lib.t_mzml_scan.argtypes = [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 8
    lib.t_mzml_scan.restype = None
    return lib


def scan(lib, text):
    """the whole scan of `text` (bytes) on the host -> the dict of `Context.scan_mzml`; the payload is a uint8 host array laid
    out as the gather kernel lays it out (8-byte aligned arrays in spectrum order, gaps zero)"""
    raw = np.frombuffer(bytes(text) + b"\xa5", np.uint8).copy()                 # (a guard byte behind the text)
    n = len(raw) - 1
    cap = n // 21 + 2
    counts = np.zeros(4, np.int64)
    status, charge = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    ident, span = np.zeros((cap, 2), np.int64), np.zeros((cap, 2), np.int64)
    pmz, rt = np.zeros(cap), np.zeros(cap)
    arrays = np.zeros((2 * cap, 4), np.int64)
    lib.t_mzml_scan(_p(raw), n, cap, _p(counts), _p(status), _p(ident), _p(span), _p(pmz), _p(charge), _p(rt), _p(arrays))
    k, inside, flags, tags = (int(c) for c in counts)
    if flags:
        return dict(flags=flags, tags=tags)
    arrays = arrays[:2 * k].copy()
    rounded = (arrays[:, 1] + 7) // 8 * 8
    offset = np.concatenate([[0], np.cumsum(rounded)])
    payload = np.zeros(int(offset[-1]), np.uint8)
    for row, at in zip(arrays, offset[:-1]):
        payload[at:at + row[1]] = raw[row[0]:row[0] + row[1]]
    arrays[:, 0] = offset[:-1]
    arrays[np.repeat(status[:k] != OK, 2)] = 0
    return dict(flags=0, tags=tags, inside=inside, status=status[:k], id=ident[:k], span=span[:k], precursor_mz=pmz[:k], charge=charge[:k],
                retention_time=rt[:k], arrays=arrays, payload=payload)


class FakeContext:
    """`scan_mzml` by the host shim: what `mzml_io.read_chunks_device` needs of a context"""

    def __init__(self, lib):
        self.lib = lib
        self.texts = []

    def scan_mzml(self, text):
        self.texts.append(bytes(text))
        return scan(self.lib, text)
