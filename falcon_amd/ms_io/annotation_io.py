"""`--library_propagate`: the file beside the cluster CSV, written on the host (DESIGN.md "Annotation propagation").

`<output>.annotations.csv`: one row per cluster that has a library hit (hops 0) or was reached from one through the links of its
molecular family, in cluster-id order.  It carries the cluster CSV's `#` header followed by the network, family, library and
propagation option lines.  float32 columns are written as `str(np.float32(x))` (their shortest round-trip form, as in the cluster
CSV); quoting is `csv.QUOTE_MINIMAL` (compound names hold commas and quotes).

A block is one charge partition: dict(charge (the CSV's text: "2", "None"), first (the global id of the charge's cluster 0),
n_families (the charge's families: a charge's family ids count from 0, the file carries the global ids of
<output>.families.csv), and per row, in ascending cluster order: cluster, hops, source, via i32 (cluster indices of the charge;
via -1 at hops 0), family i32 (-1: none), score, delta_mz f32 = float32(precursor of the cluster's medoid - precursor of the
source's), library i32 (the row of the source's rank-1 hit in the charge's library), library_cosine f32 (that hit's); and the
charge's library columns by row: library_id, name, library_file, adduct, smiles, inchikey (str)).  Blocks are given in the order
of their cluster ids."""
import csv

import numpy as np

COLUMNS = ["cluster", "precursor_charge", "family", "hops", "source_cluster", "via_cluster", "path_score", "delta_mz", "library_id",
           "name", "library_file", "library_cosine", "adduct", "smiles", "inchikey"]


def _f32(x) -> str:
    return str(np.float32(x))


def write_annotations(f, header, blocks) -> None:
    """the rows of `blocks` into the text file `f` behind the `#` lines of `header`"""
    for line in header:
        f.write(f"# {line}\n")
    f.write("#\n")
    w = csv.writer(f, quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
    w.writerow(COLUMNS)
    base = 0
    for b in blocks:
        first = int(b["first"])
        for e in range(len(b["cluster"])):
            fam, via, r = int(b["family"][e]), int(b["via"][e]), int(b["library"][e])
            w.writerow([first + int(b["cluster"][e]), b["charge"], base + fam if fam >= 0 else -1, int(b["hops"][e]),
                        first + int(b["source"][e]), first + via if via >= 0 else "", _f32(b["score"][e]), _f32(b["delta_mz"][e]),
                        str(b["library_id"][r]), str(b["name"][r]), str(b["library_file"][r]), _f32(b["library_cosine"][e]),
                        str(b["adduct"][r]), str(b["smiles"][r]), str(b["inchikey"][r])])
        base += int(b["n_families"])


def write(output_filename: str, header, blocks) -> None:
    """`<output_filename>.annotations.csv`"""
    with open(f"{output_filename}.annotations.csv", "w", newline="") as f:
        write_annotations(f, header, blocks)
