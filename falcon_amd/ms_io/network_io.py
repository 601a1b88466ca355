"""`--network`: the file beside the cluster CSV, written on the host (DESIGN.md "Representative network").

`<output>.network.csv`: one row per link between two clusters of one precursor charge, in (cluster_a, cluster_b) order.  It
carries the cluster CSV's `#` header followed by the network option lines.  float32 columns are written as `str(np.float32(x))`
(their shortest round-trip form, as in the cluster CSV); quoting is `csv.QUOTE_MINIMAL`.

A block is one charge partition: dict(charge (the CSV's text: "2", "None"), first (the global id of the charge's cluster 0),
a, b i32[m] (cluster indices of the charge, a < b, in (a, b) order), similarity f32[m], matched i32[m], delta_mz f32[m]).
Blocks are given in the order of their cluster ids."""
import csv

import numpy as np

COLUMNS = ["cluster_a", "cluster_b", "precursor_charge", "delta_mz", "cosine", "matched_peaks"]


def _f32(x) -> str:
    return str(np.float32(x))


def write_network(f, header, blocks) -> None:
    """the links of `blocks` into the text file `f` behind the `#` lines of `header`"""
    for line in header:
        f.write(f"# {line}\n")
    f.write("#\n")
    w = csv.writer(f, quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
    w.writerow(COLUMNS)
    for b in blocks:
        first = int(b["first"])
        for e in range(len(b["a"])):
            w.writerow([first + int(b["a"][e]), first + int(b["b"][e]), b["charge"], _f32(b["delta_mz"][e]), _f32(b["similarity"][e]),
                        int(b["matched"][e])])


def write(output_filename: str, header, blocks) -> None:
    """`<output_filename>.network.csv`"""
    with open(f"{output_filename}.network.csv", "w", newline="") as f:
        write_network(f, header, blocks)
