"""Corpora for the library (`--library`) and representative (`--assign_to`) MGF readers: a writer of GNPS-style entries with the
designed cases of the readers' rules among clean ones, and a canonical form of the readers' results (host dicts, or the device
reader's chunks through `mgf_io.chunk_entries`) in which two readers are compared field by field, floats by their bits."""
import os

import numpy as np

KEYS = ("SPECTRUMID", "NAME", "COMPOUND_NAME", "ADDUCT", "SMILES", "INCHIKEY", "IONMODE")


def clean_entry(rng, i, n_peaks=None):
    """one GNPS-style entry inside the device grammar and the fast forms: no TITLE, all seven keys, repr() numbers"""
    n_peaks = int(rng.integers(1, 40)) if n_peaks is None else n_peaks
    mz = np.sort(rng.uniform(50, 1500, n_peaks))
    it = rng.uniform(1, 1e5, n_peaks)
    head = [f"PEPMASS={float(rng.uniform(100, 1500))!r}", f"CHARGE={rng.choice(['1', '1+', '2+', '1-', '0'])}", "MSLEVEL=2",
            f"IONMODE={rng.choice(['Positive', 'Negative'])}", f"NAME=compound {i} [M+H]+", f"COMPOUND_NAME=cmp {i}",
            f"ADDUCT={rng.choice(['[M+H]+', '[M-H]-', 'M+Na'])}", f"SMILES=C{'C' * int(rng.integers(0, 30))}(=O)O{i}",
            f"INCHIKEY=KEY{i:08d}-UHFFFAOYSA-N", f"SPECTRUMID=CCMSLIB{i:011d}", f"SCANS={i}"]
    head = [head[k] for k in rng.permutation(len(head))]
    return ["BEGIN IONS"] + head + [f"{float(m)!r}\t{float(v)!r}" for m, v in zip(mz, it)] + ["END IONS", ""]


def _e(*lines, pep="PEPMASS=500.5", peaks=("100.5 1.0", "200.25 3.5", "150.125 2.0"), end=True):
    return ["BEGIN IONS"] + ([pep] if pep else []) + list(lines) + list(peaks) + (["END IONS", ""] if end else [])


# the designed cases, in file order (an entry the readers skip still takes an entry number)
DESIGNED = [
    _e("SPECTRUMID=", "TITLE=the title stands in", "NAME=a"),                          # empty SPECTRUMID, then TITLE
    _e("NAME=skipped: no precursor", pep=None),
    _e("NAME=skipped: zero", pep="PEPMASS=0"),
    _e("NAME=fallback id behind skipped entries"),                                      # neither SPECTRUMID nor TITLE
    _e("SPECTRUMID=S1", "NAME=", "COMPOUND_NAME=the compound name stands in"),
    _e("SPECTRUMID=S2", "CHARGE="), _e("SPECTRUMID=S3", "CHARGE=0"), _e("SPECTRUMID=S4", "CHARGE=1-"),
    _e("SPECTRUMID=S5", "CHARGE=2+ and 3+"),
    _e("SPECTRUMID=S6", pep="PEPMASS=-5"), _e("SPECTRUMID=S7", pep="PEPMASS=nan"), _e("SPECTRUMID=S8", pep="PEPMASS=500.5 1e5"),
    _e("SPECTRUMID=S9", peaks=("100.5 1.0", "abc def")),                                # a malformed peak line
    ["BEGIN IONS", "SPECTRUMID=lost", "PEPMASS=1.5", "77.0 1"] + _e("SPECTRUMID=S10", "Name = second BEGIN wins"),
    _e("SPECTRUMID=S11", "SMILES=C=O", "smiles = CC=O ", "Inchikey=MixedCase", "NAMES=not a name", "ADDUCT=first", "ADDUCT=last"),
    _e("SPECTRUMID=S12", "SMILES=" + "C" * 300, "NAME=" + "n" * 256, "INCHIKEY=" + "k" * 257),      # longer than a row
    _e("SPECTRUMID=S13", "NAME=" + "x" * 5000),                                         # a header line the kernels leave to the host
    _e("TITLE=only a title", "RTINSECONDS=12-13"),
    _e("SPECTRUMID=S14", "PEPMASS=1e40", pep=None), _e("SPECTRUMID=S15", peaks=()),
    _e("SPECTRUMID=S16", peaks=("300.5 1", "100.25 2", "100.25 3", "nan 4")),
]


def clean_text(n, seed, first=0):
    rng = np.random.default_rng(seed)
    return "\n".join(l for i in range(n) for l in clean_entry(rng, first + i)) + "\n"


def write_corpus(folder):
    """two library files: about 300 entries, the designed cases between clean ones, an unterminated last entry in the first
    file and a non-ASCII name in the middle of the second -> their paths"""
    rng = np.random.default_rng(17)
    lines = ["# a library", "COM=header outside an entry", ""]
    for k, case in enumerate(DESIGNED):
        for j in range(7):
            lines += clean_entry(rng, 10 * k + j)
        lines += case
    lines += _e("SPECTRUMID=unterminated", end=False)
    one = os.path.join(str(folder), "lib_one.mgf")
    with open(one, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode("ascii"))
    lines = []
    for i in range(60):
        lines += clean_entry(rng, 1000 + i)
    lines += _e("NAME=fallback id in front of the name outside the grammar")
    lines += _e("SPECTRUMID=S100", "NAME=caféine")
    lines += _e("NAME=fallback id behind it", pep="PEPMASS=0") + _e("NAME=and its numbering goes on")
    for i in range(60):
        lines += clean_entry(rng, 2000 + i)
    two = os.path.join(str(folder), "lib_two.mgf")
    with open(two, "wb") as f:
        f.write(("\r\n".join(lines) + "\r\n").encode("utf-8"))
    return [one, two]


def canonical(specs):
    """reader dicts -> tuples of plain values: strings, ints, the bits of the floats; peaks sorted by m/z (stable) as
    `mgf_io.raw_csr` sorts them; the file by its base name; no charge and charge 0 are one"""
    out = []
    for s in specs:
        mz, it = np.asarray(s["mz"], np.float64), np.asarray(s["intensity"], np.float32)
        order = np.argsort(mz, kind="stable")
        row = [("identifier", str(s["identifier"])), ("precursor_mz", float(s["precursor_mz"]).hex()),
               ("precursor_charge", int(s["precursor_charge"] or 0)), ("retention_time", float(s["retention_time"]).hex()),
               ("mz", mz[order].tobytes().hex()), ("intensity", it[order].tobytes().hex()), ("filename", os.path.basename(s["filename"]))]
        row += [(k, s[k] if k == "cluster" else str(s[k])) for k in ("name", "adduct", "smiles", "inchikey", "ionmode", "cluster") if k in s]
        out.append(tuple(row))
    return out


# ---- representative MGFs ------------------------------------------------------------------------------------------------------
def rep(title, cluster, *lines, pep="PEPMASS=400.25", peaks=("100.5 1.0", "200.25 3.5")):
    """one entry of a representative MGF; `cluster`: the text behind CLUSTER=, None: no such line"""
    return "\n".join(["BEGIN IONS", f"TITLE={title}"] + ([pep] if pep else []) + list(lines) +
                     ([f"CLUSTER={cluster}"] if cluster is not None else []) + list(peaks) + ["END IONS", ""]) + "\n"
