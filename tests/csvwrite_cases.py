"""Case sets of the CSV writer's tests (tests/test_csvwrite_cpu.py on the host build, tests/test_gpu_csvwrite.py on the device):
float32 values against `str(np.float32(x))`, strings against `falcon._natural_key`, rows against `falcon._write_cluster_info`."""
import numpy as np

COLUMN_ROW = b"filename,spectrum_id,precursor_charge,precursor_mz,retention_time,cluster\n"
NUMPY_EIGHT_DIGITS = (0x0F800000, 0x6B000000, 0x6C800000)      # powers of two where numpy prints 8 digits, not the rounded 9


def _ulps(bits, span):
    """uint32 bit patterns -> every pattern within `span` ulps of them that is a finite positive float32"""
    b = (np.asarray(bits, np.int64)[:, None] + np.arange(-span, span + 1)[None, :]).ravel()
    return b[(b >= 0) & (b < 0x7F800000)].astype(np.uint32)


def number_set() -> np.ndarray:
    """every power of two +- 2 ulp, denormals 1..3000 and the largest, d 10^k (d 1..999, k -12..19) +- 1 ulp, 1e-4 and 1e16 +- 2
    ulp, +-0, nan, +-inf, the largest finite, the three patterns where numpy prints 8 digits; each also negated"""
    pow2 = _ulps(np.arange(1, 255, dtype=np.int64) << 23, 2)
    den = np.concatenate([np.arange(1, 3001), [0x7FFFFF]]).astype(np.uint32)
    with np.errstate(over="ignore"):
        dk = (np.arange(1, 1000, dtype=np.float64)[:, None] * 10.0 ** np.arange(-12, 20)[None, :]).ravel().astype(np.float32)
    dk = _ulps(dk[np.isfinite(dk)].view(np.uint32), 1)
    edge = _ulps(np.array([1e-4, 1e16], np.float32).view(np.uint32), 2)
    special = np.array([0, 0x7F800000, 0x7FC00000, 0x7F7FFFFF, *NUMPY_EIGHT_DIGITS], np.uint32)
    pos = np.unique(np.concatenate([pow2, den, dk, edge, special]))
    return np.concatenate([pos, pos | np.uint32(0x80000000)]).view(np.float32)


def random_bits(n: int, seed: int = 11) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def expected_number(v) -> bytes:
    return str(np.float32(v)).encode("ascii")


# ---- the comparator ---------------------------------------------------------------------------------------------------------------
def compare_strings():
    base = ["", "1", "01", "001", "a", "a1", "a01", "a!", "a1b", "a9", "a10", "a1b2", "a1b10", "ab", "ab1", "abc1",
            "0", "00", "a0", "a00", "a0b", "a~", "a/", "a:", "A1", " 1", "1 ", "1a", "01a", "1b", "10", "9", "2a10", "2a9"]
    forty = "1234567890" * 4
    long_runs = ["x" + forty, "x" + forty[:-1] + "1", "x" + forty[:-1] + "9", "x0" + forty, "x000" + forty[:-1] + "1",
                 "x" + forty + "y", "x" + forty[:-1], "x00" + forty[:-1], "x" + forty + "0"]
    zeros = ["scan=7", "scan=07", "scan=007", "scan=70", "scan=070", "scan=0", "scan=00", "scan=", "scan", "scan=7.1", "scan=07.01",
             "scan=7.10", "scan=9", "scan=10", "scan=09", "scan=010"]
    titles = ['run "A", fraction 2.17.17.2 File:"run A.raw", NativeID:"controllerType=0 controllerNumber=1 scan=17"',
              'run "A", fraction 2.17.17.2 File:"run A.raw", NativeID:"controllerType=0 controllerNumber=1 scan=9"',
              'run "A", fraction 2.9.9.2 File:"run A.raw", NativeID:"controllerType=0 controllerNumber=1 scan=9"',
              'run "A", fraction 10.9.9.2 File:"run A.raw", NativeID:"controllerType=0 controllerNumber=1 scan=9"',
              'run "A",fraction 2.9.9.2', 'run "A"', 'run "B", 1', "controllerType=0 controllerNumber=1 scan=9",
              "controllerType=0 controllerNumber=1 scan=10", "controllerType=0 controllerNumber=01 scan=10",
              "controllerType=0 controllerNumber=1 scan=10 ", "controllerType=0 controllerNumber=1  scan=10"]
    return base + long_runs + zeros + titles


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
class Rows:
    """the CSV's columns, text fields as lists of str (a numpy str array would drop a trailing NUL)"""

    def __init__(self, filename, identifier, charge, precursor_mz, retention_time, cluster):
        self.filename, self.identifier = list(filename), list(identifier)
        self.charge = np.asarray(charge, np.int32)
        self.precursor_mz, self.retention_time = np.asarray(precursor_mz, np.float32), np.asarray(retention_time, np.float32)
        self.cluster = np.asarray(cluster, np.int64)
        assert len({len(self.filename), len(self.identifier), len(self.charge), len(self.precursor_mz), len(self.retention_time),
                    len(self.cluster)}) == 1

    def __len__(self):
        return len(self.filename)

    def take(self, idx):
        idx = np.asarray(idx, np.int64)
        return Rows([self.filename[i] for i in idx], [self.identifier[i] for i in idx], self.charge[idx], self.precursor_mz[idx],
                    self.retention_time[idx], self.cluster[idx])

    def tuples(self, through_numpy: bool = False):
        """the tuples falcon appends to `rows_all`; `through_numpy`: the text fields as a partition's str arrays hold them"""
        fn, ident = self.filename, self.identifier
        if through_numpy:
            fn, ident = np.array(fn, dtype=str), np.array(ident, dtype=str)
        return [(str(fn[i]), str(ident[i]), "None" if self.charge[i] == 0 else str(int(self.charge[i])), np.float32(self.precursor_mz[i]),
                 np.float32(self.retention_time[i]), int(self.cluster[i])) for i in range(len(self))]

    def block(self):
        """a column block as falcon collects it for the device writer (one charge)"""
        assert len(set(self.charge.tolist())) == 1
        return dict(filename=np.array(self.filename, dtype=str), identifier=np.array(self.identifier, dtype=str), charge=int(self.charge[0]),
                    precursor_mz=self.precursor_mz, retention_time=self.retention_time, cluster=self.cluster)


def body_of(tuples, tmp_dir) -> bytes:
    """`falcon._write_cluster_info`'s file for the tuples, less its header: the rows' bytes"""
    import os
    from falcon_amd import falcon
    from falcon_amd.config import config
    out = os.path.join(str(tmp_dir), "body")
    config.parse(["in.mgf", out])
    if os.path.exists(out + ".csv"):
        os.remove(out + ".csv")
    falcon._write_cluster_info(tuples)
    raw = open(out + ".csv", "rb").read()
    return raw[raw.index(COLUMN_ROW) + len(COLUMN_ROW):]


def host_writes_nul() -> bool:
    """csv.writer of CPython before 3.11 raises on a NUL in a field ("need to escape, but no escapechar set"): there the writer of
    record has no bytes for it"""
    import csv
    import io
    try:
        csv.writer(io.StringIO(), quoting=csv.QUOTE_MINIMAL, lineterminator="\n").writerow(["\x00", ""])
    except csv.Error:
        return False
    return True


def ascii_rows() -> Rows:
    """every ASCII byte except the newline (and except NUL where the host's csv.writer refuses it) once as a one-character id and
    once as a file name; fields of only quotes; empty ids; charge 0 and negative charges; clusters up to 2^62; numbers of every
    layout"""
    chars = [chr(c) for c in range(0 if host_writes_nul() else 1, 128) if c != 0x0A]
    ident = chars + ["scan=1"] * len(chars) + ['"', '""', '"""', "", "", ",", ",,", '","', 'a"b,c', " lead", "trail ", "a\rb"]
    fn = ["f.mzML"] * len(chars) + chars + ['"', '""', "", "", 'a "b".mgf', "x,y.mgf", "", "f", "f", "f", "f", "f"]
    n = len(ident)
    assert len(fn) == n
    rng = np.random.default_rng(5)
    charge = rng.integers(-3, 8, n).astype(np.int32)
    charge[:4] = [0, -1, 2 ** 31 - 1, -2 ** 31]
    values = np.array([0.0, -0.0, 1e-4, 9.999999e15, 1e16, 0.1, 1.5, 123456.79, 3.4028235e38, 1e-45, -1.0, np.inf, -np.inf, np.nan, 500.25,
                       1234.5677], np.float32)
    pm, rt = values[np.arange(n) % len(values)], values[(np.arange(n) * 7 + 3) % len(values)]
    cluster = rng.integers(0, 5000, n).astype(np.int64)
    cluster[:4] = [0, 2 ** 62, -1, 2 ** 40]
    return Rows(fn, ident, charge, pm, rt, cluster)


def number_rows() -> Rows:
    """the edge numbers through the device compile of the formatter: powers of two +- 1 ulp and the layout switches"""
    x = number_set()
    x = x[::7][:4000]
    n = len(x)
    return Rows(["numbers.mgf"] * n, [f"scan={i}" for i in range(n)], np.full(n, 2), x, x[::-1], np.arange(n))


def long_rows() -> Rows:
    """rows longer than a write tile next to short ones: ids of 0 / 1 / 127 / 128 / 5,000 / 20,000 bytes with quotes inside, so that a
    tile of 64 rows fits, fits in part or holds one row that does not fit at all"""
    lens = [0, 1, 127, 128, 129, 5000, 3, 20000, 2, 8100, 8200, 60, 61]
    ident = [('ab"c,' * (m // 5 + 1))[:m] for m in lens] + [f"scan={i}" for i in range(150)]
    n = len(ident)
    rng = np.random.default_rng(6)
    return Rows(["long.mgf"] * n, ident, rng.integers(0, 4, n), rng.uniform(100, 2000, n), rng.uniform(0, 9000, n), rng.integers(0, 99, n))


ROW_SETS = ["ascii_rows", "number_rows", "long_rows"]


# ---- the order ----------------------------------------------------------------------------------------------------------------------
def order_pool(n: int, seed: int = 7):
    """-> (file_rank i32[n], ids: list of n ASCII str) with 3 ranks, long shared prefixes, many exact duplicates and leading-zero
    ties, shuffled"""
    rng = np.random.default_rng(seed + n)
    prefix = ["controllerType=0 controllerNumber=1 scan=", "controllerType=0 controllerNumber=01 scan=", "run.17.", 'run "A", f', ""]
    pool = []
    for p in prefix:
        for k in (0, 1, 7, 9, 10, 11, 99, 100, 101, 12345678901234567890):
            pool += [f"{p}{k}", f"{p}0{k}", f"{p}00{k} ", f"{p}{k}.{k}", f"{p}{k}a", f"{p}{k}!"]
    pool += [f"{prefix[0]}{k}" for k in range(max(n // 3, 1))]
    ids = [pool[i] for i in rng.integers(0, len(pool), n)]
    return rng.integers(0, 3, n).astype(np.int32), ids


def host_order(file_rank, ids):
    from falcon_amd.falcon import _natural_key
    keys = [_natural_key(s) for s in ids]
    return sorted(range(len(ids)), key=lambda i: (int(file_rank[i]), keys[i]))
