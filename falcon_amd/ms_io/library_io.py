"""`--library`: the file beside the cluster CSV, written on the host (DESIGN.md "Library search").

`<output>.library.csv`: one row per hit of a cluster representative in the reference library, in (cluster, rank) order.  It
carries the cluster CSV's `#` header followed by the library option lines.  float32 columns are written as `str(np.float32(x))`
(their shortest round-trip form, as in the cluster CSV); quoting is `csv.QUOTE_MINIMAL` (compound names hold commas and quotes).

A block is one charge partition: dict(charge (the CSV's text: "2", "None"), first (the global id of the charge's cluster 0),
cluster i32[m] (cluster indices of the charge), library i32[m] (rows of the charge's library), similarity f32[m], matched i32[m],
delta_mz f32[m] = float32(representative's precursor - library precursor), in (cluster, rank) order, and the charge's library
columns by row: library_id, name, library_file, adduct, smiles, inchikey (str) and library_precursor_mz f32).  Blocks are given
in the order of their cluster ids."""
import csv

import numpy as np

COLUMNS = ["cluster", "precursor_charge", "rank", "library_id", "name", "library_file", "library_precursor_mz", "delta_mz", "cosine",
           "matched_peaks", "adduct", "smiles", "inchikey"]


def _f32(x) -> str:
    return str(np.float32(x))


def write_hits(f, header, blocks) -> None:
    """the hits of `blocks` into the text file `f` behind the `#` lines of `header`"""
    for line in header:
        f.write(f"# {line}\n")
    f.write("#\n")
    w = csv.writer(f, quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
    w.writerow(COLUMNS)
    for b in blocks:
        first, rank, last = int(b["first"]), 0, None
        for e in range(len(b["cluster"])):
            c, r = int(b["cluster"][e]), int(b["library"][e])
            rank = rank + 1 if c == last else 1
            last = c
            w.writerow([first + c, b["charge"], rank, str(b["library_id"][r]), str(b["name"][r]), str(b["library_file"][r]),
                        _f32(b["library_precursor_mz"][r]), _f32(b["delta_mz"][e]), _f32(b["similarity"][e]), int(b["matched"][e]),
                        str(b["adduct"][r]), str(b["smiles"][r]), str(b["inchikey"][r])])


def write(output_filename: str, header, blocks) -> None:
    """`<output_filename>.library.csv`"""
    with open(f"{output_filename}.library.csv", "w", newline="") as f:
        write_hits(f, header, blocks)
