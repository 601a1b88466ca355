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


# `--network_families` (DESIGN.md "Molecular families").  A block then holds the surviving links only and, beside the columns
# above, family i32[m] (the family of a link's two clusters), node_family / node_size i32[clusters of the charge] (-1 / 1: a
# cluster without a surviving link) and n_families.  A charge's family ids count from 0; the files carry global ids: a charge's
# families follow those of the blocks in front of it.
FAMILY_COLUMNS = ["cluster", "precursor_charge", "family", "family_size"]


def _family_bases(blocks):
    """the global id of every block's family 0"""
    bases, base = [], 0
    for b in blocks:
        bases.append(base)
        base += int(b["n_families"])
    return bases


def write_network_with_families(f, header, blocks) -> None:
    """`write_network` with a seventh column `family`"""
    for line in header:
        f.write(f"# {line}\n")
    f.write("#\n")
    w = csv.writer(f, quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
    w.writerow(COLUMNS + ["family"])
    for b, base in zip(blocks, _family_bases(blocks)):
        first = int(b["first"])
        for e in range(len(b["a"])):
            w.writerow([first + int(b["a"][e]), first + int(b["b"][e]), b["charge"], _f32(b["delta_mz"][e]), _f32(b["similarity"][e]),
                        int(b["matched"][e]), base + int(b["family"][e])])


def write_families(f, header, blocks) -> None:
    """one row per cluster in cluster-id order: its family (-1: none) and the family's clusters (1 then)"""
    for line in header:
        f.write(f"# {line}\n")
    f.write("#\n")
    w = csv.writer(f, quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
    w.writerow(FAMILY_COLUMNS)
    for b, base in zip(blocks, _family_bases(blocks)):
        first = int(b["first"])
        for c in range(len(b["node_family"])):
            fam = int(b["node_family"][c])
            w.writerow([first + c, b["charge"], base + fam if fam >= 0 else -1, int(b["node_size"][c])])


def write_with_families(output_filename: str, header, blocks) -> None:
    """`<output_filename>.network.csv` with the family column and `<output_filename>.families.csv`"""
    with open(f"{output_filename}.network.csv", "w", newline="") as f:
        write_network_with_families(f, header, blocks)
    with open(f"{output_filename}.families.csv", "w", newline="") as f:
        write_families(f, header, blocks)
