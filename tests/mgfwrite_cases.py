"""Inputs of the MGF writer's tests, shared by the CPU tests of `csrc/mgfwrite.h` and the GPU tests of the kernels: the float32
number set and the entry cases, with `mgf_io.write_spectra` -- the writer of record -- as the expected bytes."""
import os
import tempfile

import numpy as np

from falcon_amd.ms_io import mgf_io

MANTISSAS = (0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF)


def number_set() -> np.ndarray:
    """float32 values: every biased exponent 0..255 (denormals, inf and NaN included) x the edge mantissas + 16 seeded random
    ones, both signs; the float32 neighbours of 1e-4 and 1e16 (where the layout switches); +-0.0 and a few plain values"""
    rng = np.random.default_rng(20250)
    bits = []
    for e in range(256):
        ms = list(MANTISSAS) + [int(v) for v in rng.integers(0, 1 << 23, 16)]
        for m in ms:
            for s in (0, 1):
                bits.append((s << 31) | (e << 23) | m)
    out = [np.array(bits, np.uint32).view(np.float32)]
    for edge in (1e-4, 1e16):
        c = np.float32(edge)
        lo = hi = c
        near = [c]
        for _ in range(3):
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
            near += [lo, hi]
        out.append(np.array(near + [-v for v in near], np.float32))
    out.append(np.array([0.0, -0.0, 290.0, 1500.0, 16777216.0], np.float32))
    return np.concatenate(out)


def random_bits(n: int, seed: int = 20251) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def expected_number(x) -> bytes:
    return repr(float(np.float32(x))).encode("ascii")


class Entries:
    """columns of n entries over a peak CSR (the writer's inputs, as numpy arrays); `rows[k]`: the CSR row of entry k"""

    def __init__(self, mz, intensity, indptr, rows, precursor_mz, retention_time, charge, cluster, title):
        self.mz, self.intensity = np.asarray(mz, np.float32), np.asarray(intensity, np.float32)
        self.indptr, self.rows = np.asarray(indptr, np.int64), np.asarray(rows, np.int32)
        self.precursor_mz, self.retention_time = np.asarray(precursor_mz, np.float32), np.asarray(retention_time, np.float32)
        self.charge, self.cluster = np.asarray(charge, np.int32), np.asarray(cluster, np.int64)
        self.title = np.asarray(title, dtype=str) if len(title) else np.zeros(0, dtype=str)

    def __len__(self):
        return len(self.rows)

    def dicts(self):
        """what falcon hands `write_spectra`: Python floats for the precursor and RT, float32 arrays for the peaks"""
        for k, r in enumerate(self.rows):
            a, b = self.indptr[r], self.indptr[r + 1]
            yield {"identifier": str(self.title[k]), "precursor_mz": float(self.precursor_mz[k]),
                   "precursor_charge": int(self.charge[k]) if self.charge[k] else None,
                   "retention_time": float(self.retention_time[k]), "mz": self.mz[a:b], "intensity": self.intensity[a:b],
                   "cluster": int(self.cluster[k])}

    def expected(self) -> bytes:
        """the bytes `write_spectra` writes"""
        with tempfile.TemporaryDirectory() as d:
            fn = os.path.join(d, "want.mgf")
            mgf_io.write_spectra(fn, self.dicts())
            with open(fn, "rb") as f:
                return f.read()

    def take(self, ks):
        ks = np.asarray(ks, np.int64)
        return Entries(self.mz, self.intensity, self.indptr, self.rows[ks], self.precursor_mz[ks], self.retention_time[ks],
                       self.charge[ks], self.cluster[ks], self.title[ks])


def _csr(sizes, rng, lo=1e-3, hi=2000.0):
    indptr = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=indptr[1:])
    nnz = int(indptr[-1])
    mz = np.exp(rng.uniform(np.log(lo), np.log(hi), nnz)).astype(np.float32)
    it = np.exp(rng.uniform(np.log(lo), np.log(hi), nnz)).astype(np.float32)
    return mz, it, indptr


PEAK_COUNTS = (0, 1, 63, 64, 65, 200, 5000)
TITLE_LENGTHS = (0, 1, 255, 2047, 2048, 2049, 5000)      # (2,048: the title bytes the write kernel appends per piece)


def entry_cases() -> Entries:
    """peaks of 0, 1, 63, 64, 65, 200 and 5,000 (a raw-sized entry); charge none / positive / negative / two-digit; cluster ids 0
    and 2^40; titles of 0, 1, 255, 2,047, 2,048, 2,049 and 5,000 bytes and a non-ASCII UTF-8 one; retention time -1.0.  Values
    lie in [1e-3, 2000]: the reader's fast forms (the round trip reads them back)."""
    rng = np.random.default_rng(7)
    sizes = list(PEAK_COUNTS) + [3, 17, 5, 0, 9, 2, 0, 4]
    mz, it, indptr = _csr(sizes, rng)
    n = len(sizes)
    charge = np.array([0, 2, -1, 12, 3, -14, 0, 2, 2, 3, 1, 2, 2, 0, 3], np.int32)[:n]
    cluster = np.array([0, 1 << 40, 5, 6, 7, 8, 9, 10, 11, 12, 13, 123456789012, 14, 15, 16], np.int64)[:n]
    # (the two titles the device reader leaves to the host -- a line above its limit, a non-ASCII byte -- sit on small entries)
    title = ["", "x", "t" * 255, "id3", "id4", "mzspec:PXD000001:run:scan:7", "a=b c", "  padded",
             "L" * 5000, "spéctre 质谱 μ", "id10", "id11", "A" * 2047, "B" * 2048, "C" * 2049][:n]
    assert sorted(len(t) for t in title if len(t) in TITLE_LENGTHS) == sorted(TITLE_LENGTHS)
    pm = np.exp(rng.uniform(np.log(50.0), np.log(2000.0), n)).astype(np.float32)
    rt = rng.uniform(0.0, 2000.0, n).astype(np.float32)
    rt[2], rt[7] = -1.0, -1.0
    return Entries(mz, it, indptr, np.arange(n, dtype=np.int32), pm, rt, charge, cluster, title)


def number_entries() -> Entries:
    """the number set as the peaks (m/z and intensity) of a handful of entries, and as their precursor and RT columns"""
    x = number_set()
    n = 7
    cut = np.linspace(0, len(x), n + 1).astype(np.int64)
    rng = np.random.default_rng(8)
    return Entries(x, x[::-1].copy(), cut, np.arange(n, dtype=np.int32), x[rng.integers(0, len(x), n)], x[rng.integers(0, len(x), n)],
                   np.array([0, 1, -2, 3, 0, 10, -11], np.int32), np.arange(n, dtype=np.int64) * 1000003, [f"numbers {k}" for k in range(n)])


def shuffled_rows() -> Entries:
    """the medoid form: `rows` neither monotone nor unique"""
    rng = np.random.default_rng(9)
    sizes = rng.integers(0, 150, 40)
    sizes[[3, 11]] = [64, 128]
    mz, it, indptr = _csr(sizes, rng)
    rows = rng.permutation(40).astype(np.int32)[:30]
    rows = np.concatenate([rows, rows[[0, 5, 5, 17]]]).astype(np.int32)
    n = len(rows)
    return Entries(mz, it, indptr, rows, rng.uniform(100, 1500, n), rng.uniform(0, 3000, n), rng.integers(0, 5, n), rng.permutation(n) + 100,
                   [f"scan={k} file.mgf" for k in range(n)])
