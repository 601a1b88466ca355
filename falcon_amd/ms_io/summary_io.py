"""`--cluster_summary`: the two files beside the cluster CSV, written on the host (DESIGN.md "Member scores and cluster summary").

`<output>.clusters.csv`: one row per cluster in cluster-id order; `<output>.scores.csv`: one row per spectrum, grouped by cluster
id, inside a cluster in the row order of its charge partition.  Both carry the cluster CSV's `#` header.  float32 columns are
written as `str(np.float32(x))` (their shortest round-trip form, as in the cluster CSV), the float64 mean as `repr(float(x))`;
quoting is `csv.QUOTE_MINIMAL`.

A block is one charge partition: dict(charge (the CSV's text: "2", "None"), cluster i64[n_clusters] (the global ids, ascending),
labels i64[n] (global id per row), filename, identifier str[n], medoids i[n_clusters] (rows), similarity f32[n], matched i32[n]
and the per-cluster columns size, sim_min, worst_row, sim_mean, pmz_min, pmz_max, rt_min, rt_max).  Blocks are given in the
order of their cluster ids."""
import csv

import numpy as np

CLUSTER_COLUMNS = ["cluster", "precursor_charge", "size", "representative", "sim_min", "sim_mean", "worst", "pmz_min", "pmz_max",
                   "rt_min", "rt_max"]
SCORE_COLUMNS = ["cluster", "filename", "identifier", "similarity", "matched_peaks"]


def _f32(x) -> str:
    return str(np.float32(x))


def _writer(f, header, columns):
    for line in header:
        f.write(f"# {line}\n")
    f.write("#\n")
    w = csv.writer(f, quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
    w.writerow(columns)
    return w


def write_clusters(f, header, blocks) -> None:
    """the per-cluster table of `blocks` into the text file `f` behind the `#` lines of `header`"""
    w = _writer(f, header, CLUSTER_COLUMNS)
    for b in blocks:
        ident = b["identifier"]
        for c in range(len(b["cluster"])):
            worst = int(b["worst_row"][c])
            w.writerow([int(b["cluster"][c]), b["charge"], int(b["size"][c]), str(ident[int(b["medoids"][c])]), _f32(b["sim_min"][c]),
                        repr(float(b["sim_mean"][c])), str(ident[worst]) if worst >= 0 else "", _f32(b["pmz_min"][c]),
                        _f32(b["pmz_max"][c]), _f32(b["rt_min"][c]), _f32(b["rt_max"][c])])


def write_scores(f, header, blocks) -> None:
    """the per-spectrum table of `blocks` into the text file `f` behind the `#` lines of `header`"""
    w = _writer(f, header, SCORE_COLUMNS)
    for b in blocks:
        labels = np.asarray(b["labels"], np.int64)
        for i in np.argsort(labels, kind="stable"):          # by cluster id, then partition row
            w.writerow([int(labels[i]), str(b["filename"][i]), str(b["identifier"][i]), _f32(b["similarity"][i]),
                        int(b["matched"][i])])


def write(output_filename: str, header, blocks) -> None:
    """`<output_filename>.clusters.csv` and `<output_filename>.scores.csv`"""
    with open(f"{output_filename}.clusters.csv", "w", newline="") as f:
        write_clusters(f, header, blocks)
    with open(f"{output_filename}.scores.csv", "w", newline="") as f:
        write_scores(f, header, blocks)
