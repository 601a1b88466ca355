"""`falcon` command line entry point: same contract as reference falcon/falcon.py:33-244
(`main(args) -> int`, console script `falcon = falcon.falcon:main`, setup.cfg:43-45):
read peak files, preprocess, cluster every precursor charge independently through
`cluster.generate_clusters` (the seam the HIP path sits behind), write `<out>.csv`
(+ optional `<out>.mgf` of cluster representatives).

Differences kept deliberately small and listed in DESIGN.md: spectra are held in memory /
`.npz` files in `work_dir` instead of Lance datasets (lance is not available), the mzML / mzXML readers are stdlib
XML passes whose binary arrays are decoded on the device (`fal_decode_peaks`), and `process_spectrum` runs as one batched
device call per peak file (`fal_process_spectra`) instead of a Python loop over spectra.
"""
from __future__ import annotations

import glob
import json
import logging
import os
import re
import shutil
import random
import sys
import tempfile
import threading
from typing import Dict, List, Union

import numpy as np

from . import __version__
from .cluster import cluster, spectrum
from .config import config
from .ms_io import annotation_io, csv_io, graphml_io, library_io, mgf_io, ms_io, network_io, summary_io

logger = logging.getLogger("falcon")

random.seed(42)            # the reference seeds `random` and NumPy with 42 on import (falcon/seed.py, falcon.py:30);
np.random.seed(42)         # the device path itself draws no random numbers


def _natural_key(s: str):
    """natural sort key (natsort is absent): digit runs compare as numbers (falcon.py:206-208)."""
    return [(0, int(t)) if t.isdigit() else (1, t) for t in re.split(r"(\d+)", str(s))]


def main(args: Union[str, List[str], None] = None) -> int:
    logging.captureWarnings(True)
    root = logging.getLogger()
    root.setLevel(logging.DEBUG)
    handler = logging.StreamHandler(sys.stderr)
    handler.setLevel(logging.DEBUG)
    handler.setFormatter(logging.Formatter(
        "{asctime} {levelname} [{name}/{processName}] {module}.{funcName} : {message}", style="{"))
    root.addHandler(handler)
    try:
        return _run(args)
    finally:
        root.removeHandler(handler)


def _option_lines(header: bool = False) -> List[str]:
    """the option lines of the log; header=True: those of the output files' `#` header -- the same without `cluster_summary`
    and the `network` lines, which add files and change none (the cluster CSV is byte for byte the same with the flags)"""
    c = config
    # (the consensus options are listed only when chosen: the default header stays what it was)
    extra = ([f"representatives = {c.representatives}", f"consensus_min_fraction = {c.consensus_min_fraction:.3f}"]
             if c.representatives == "consensus" else [])
    if c.assign_to:          # (likewise: without the option every output is what it was)
        extra.append(f"assign_to = {' '.join(c.assign_to)}")
    if c.cluster_summary and not header:
        extra.append(f"cluster_summary = {c.cluster_summary}")
    if c.network and not header:
        extra += _network_lines() + _family_lines()
        if c.network_graphml:            # (in the log alone: no file's `#` header carries it)
            extra.append(f"network_graphml = {c.network_graphml}")
    if c.library and not header:
        extra += _library_lines() + _propagate_lines()
    return [
        f"work_dir = {c.work_dir}", f"overwrite = {c.overwrite}",
        f"export_representatives = {c.export_representatives}",
        f"precursor_tol = {c.precursor_tol[0]:.2f} {c.precursor_tol[1]}", f"rt_tol = {c.rt_tol}",
        f"fragment_tol = {c.fragment_tol:.2f}", f"linkage = {c.linkage}",
        f"distance_threshold = {c.distance_threshold:.3f}", f"min_matched_peaks = {c.min_matched_peaks}",
        f"batch_size = {c.batch_size}", f"min_peaks = {c.min_peaks}", f"min_mz_range = {c.min_mz_range:.2f}",
        f"min_mz = {c.min_mz:.2f}", f"max_mz = {c.max_mz:.2f}",
        f"remove_precursor_tol = {c.remove_precursor_tol:.2f}", f"min_intensity = {c.min_intensity:.2f}",
        f"max_peaks_used = {c.max_peaks_used}", f"scaling = {c.scaling}",
        # nearest-neighbour options (README.md:101-117)
        f"eps = {c.eps:.3f}", f"n_probe = {c.n_probe}", f"n_neighbors = {c.n_neighbors}",
        f"n_neighbors_ann = {c.n_neighbors_ann}", f"low_dim = {c.low_dim}", f"mz_interval = {c.mz_interval}",
        f"rescore = {c.rescore}", f"clustering = {c.clustering}", f"dtype = {c.dtype}",
        f"exact = {c.exact}",
    ] + extra


def _network_lines() -> List[str]:
    """the option lines of `--network`: in the log and in the `#` header of <output>.network.csv alone"""
    c = config
    return [f"network = {c.network}", f"network_min_cosine = {c.network_min_cosine:.3f}",
            f"network_min_matched_peaks = {c.network_min_matched_peaks}", f"network_top_k = {c.network_top_k}",
            f"network_max_shift = {c.network_max_shift:.3f}"]


def _library_lines() -> List[str]:
    """the option lines of `--library`: in the log and in the `#` header of <output>.library.csv alone"""
    c = config
    return [f"library = {' '.join(c.library)}", f"library_analog = {c.library_analog}", f"library_max_shift = {c.library_max_shift:.3f}",
            f"library_min_cosine = {c.library_min_cosine:.3f}", f"library_min_matched_peaks = {c.library_min_matched_peaks}",
            f"library_top_n = {c.library_top_n}"]


def _propagate_lines() -> List[str]:
    """the option lines of `--library_propagate`, none without the flag: behind `_library_lines()` in the log and at the end of
    the `#` header of <output>.annotations.csv"""
    c = config
    if not c.library_propagate:
        return []
    return [f"library_propagate = {c.library_propagate}", f"library_propagate_hops = {c.library_propagate_hops}",
            f"library_propagate_min_score = {c.library_propagate_min_score:.3f}"]


def _family_lines() -> List[str]:
    """the option lines of `--network_families`, none without the flag: behind `_network_lines()` in the log and in the `#`
    headers of <output>.network.csv and <output>.families.csv"""
    c = config
    if not c.network_families:
        return []
    return [f"network_families = {c.network_families}", f"network_max_family_size = {c.network_max_family_size}",
            f"network_family_delta = {c.network_family_delta:.3f}"]


def _run(args) -> int:
    config.parse(args)
    logger.info("falcon version %s", str(__version__))
    for line in _option_lines():
        logger.debug(line)
    logger.debug("mgf_reader = %s", config.mgf_reader)       # (no output depends on it: not an option line of the CSV header)
    logger.debug("mzml_reader = %s", config.mzml_reader)     # (the same)
    logger.debug("msp_reader = %s", config.msp_reader)       # (the same)
    logger.debug("mgf_writer = %s", config.mgf_writer)       # (the same)
    logger.debug("csv_writer = %s", config.csv_writer)       # (the same)
    logger.debug("graphml_writer = %s", config.graphml_writer)       # (the same)
    if config.distributed:
        return _run_distributed()

    rm_work_dir, exit_code = _setup_work_dir()
    if exit_code:
        return exit_code
    spectra_dir = os.path.join(config.work_dir, "spectra")
    pipe = cluster.ClusterPipeline(device=config.device)
    pipe.ctx.plan(0)                 # the kernels' code objects, once per process: not between the kernels of the first charge's pass
    charges = _load_or_prepare(spectra_dir, pipe.ctx)

    ann = _ann_params()
    rows_all, current_label, representatives = [], 0, []
    csv_blocks = [] if config.csv_writer == "device" else None       # column blocks instead of a tuple per spectrum
    library = {}
    summaries = [] if config.cluster_summary else None
    networks = [] if config.network else None
    hits = [] if config.library else None
    annotations = [] if config.library_propagate else None
    graphs = [] if config.network_graphml else None
    reference = _load_annotation_library(pipe.ctx) if config.library else None
    if config.assign_to:
        library, current_label = _load_library(spectra_dir, pipe.ctx)
    for charge in charges:                                                                     # falcon.py:153
        part = np.load(os.path.join(spectra_dir, f"spectra_charge_{charge}.npz"))     # plain arrays: no pickle
        n = len(part["precursor_mz"])
        if n == 0:
            continue
        if charge in library:
            part = _assign_charge(pipe, part, charge, library[charge], rows_all, csv_blocks)
            if part is None:
                continue                 # every spectrum of the charge went to an existing cluster
        ds = cluster.SpectrumDataset(part["precursor_mz"], part["retention_time"], part["mz"], part["intensity"],
                                     part["indptr"])
        labels, medoids = cluster.generate_clusters(
            ds, config.linkage, config.distance_threshold, config.min_matched_peaks, config.precursor_tol[0],
            config.precursor_tol[1], config.rt_tol, config.fragment_tol, config.batch_size, ann=ann, pipeline=pipe)
        consensus = _consensus(pipe.ctx, part, charge, labels, medoids)
        if summaries is not None:
            summaries.append(_summary_block(pipe, ds, part, charge, labels, medoids, consensus, current_label))
        if networks is not None:
            networks.append(_network_block(pipe, ds, charge, medoids, consensus, current_label))
        if hits is not None:
            hits.append(_library_block(pipe, ds, charge, medoids, consensus, current_label, reference, spectra_dir))
        if annotations is not None:          # (behind the charge's network and library blocks: it joins the two)
            annotations.append(_propagate_block(pipe, ds, charge, medoids, networks[-1], hits[-1]))
        if graphs is not None:               # (behind the charge's other blocks: its nodes and edges carry their columns)
            graphs.append(_graphml_block(part, charge, labels, medoids, current_label, networks[-1], hits[-1] if hits else None,
                                         annotations[-1] if annotations else None))
        current_label = _emit_charge(part, charge, labels, medoids, current_label, rows_all, representatives, consensus,
                                     csv_blocks=csv_blocks)
    _write_outputs(rows_all, representatives, pipe.ctx, csv_blocks=csv_blocks)
    if summaries is not None:
        logger.info("Export the cluster summary to output files %s.clusters.csv and %s.scores.csv", config.output_filename,
                    config.output_filename)
        summary_io.write(config.output_filename, _header_lines(), summaries)
    if networks is not None and config.network_families:
        logger.info("Export the representative network and its families to output files %s.network.csv and %s.families.csv",
                    config.output_filename, config.output_filename)
        network_io.write_with_families(config.output_filename, _header_lines() + _network_lines() + _family_lines(), networks)
    elif networks is not None:
        logger.info("Export the representative network to output file %s.network.csv", config.output_filename)
        network_io.write(config.output_filename, _header_lines() + _network_lines(), networks)
    if hits is not None:
        logger.info("Export the library hits to output file %s.library.csv", config.output_filename)
        library_io.write(config.output_filename, _header_lines() + _library_lines(), hits)
    if annotations is not None:
        logger.info("Export the propagated annotations to output file %s.annotations.csv", config.output_filename)
        annotation_io.write(config.output_filename, _header_lines() + _network_lines() + _family_lines() + _library_lines() +
                            _propagate_lines(), annotations)
    if graphs is not None:
        logger.info("Export the network as GraphML to output file %s.network.graphml", config.output_filename)
        graphml_io.write(config.output_filename, _header_lines() + _network_lines() + _family_lines() +
                         (_library_lines() if config.library else []) + _propagate_lines(), graphs, pipe.ctx, config.graphml_writer,
                         families=config.network_families, library=bool(config.library), propagate=config.library_propagate)
    if rm_work_dir:
        shutil.rmtree(config.work_dir)
    return 0


def _load_library(spectra_dir: str, ctx):
    """`--assign_to`: the representatives of the files, preprocessed with the run's options (scaling off: exported peaks are
    already scaled) and partitioned by charge like any input -> ({charge: arrays + `cluster` ids}, first id of a new cluster).
    Each charge's library is also left in the work directory (`library_charge_<z>.npz`): what the run matched against."""
    _, min_mz, max_mz = spectrum.get_dim(config.min_mz, config.max_mz, config.fragment_tol)
    filenames = [os.path.abspath(fn) for fn in config.assign_to]
    if config.mgf_reader == "device":                    # the text parsed on the device, the peaks left there (mgf_io.read_library_chunks)
        chunks = mgf_io.read_library(filenames, ctx=ctx)
        cols, read, valid, oip, omz, oit = _process_entry_chunks(ctx, chunks, min_mz, max_mz, scaling=None)
        n_read = int(read.sum())
        logger.debug("Representative MGFs: %d entries parsed on the device", sum(len(c) for c in chunks if c.reader == "device"))
    else:
        specs = mgf_io.read_library(filenames)
        n_read = len(specs)
    logger.info("Read %d cluster representatives from %d file(s)", n_read, len(config.assign_to))
    if not n_read:
        return {}, 0
    if config.mgf_reader == "device":
        pmz, charge, ids, rt = cols["precursor_mz"], cols["precursor_charge"], cols["cluster"], cols["retention_time"].astype(np.float32)
        first_new = int(ids[read].max()) + 1
        logger.info("Skipped %d representatives the preprocessing rejects", int((read & ~valid).sum()))
    else:
        first_new = max(s["cluster"] for s in specs) + 1
        mz, it, indptr = _raw_csr(specs)
        pmz = np.array([s["precursor_mz"] for s in specs], np.float64)
        charge = np.array([int(s["precursor_charge"]) if s.get("precursor_charge") else 0 for s in specs], np.int32)
        valid, oip, omz, oit = _process(ctx, mz, it, indptr, pmz, charge, min_mz, max_mz, scaling=None)
        logger.info("Skipped %d representatives the preprocessing rejects", int((~valid).sum()))
        ids = np.array([s["cluster"] for s in specs], np.int64)
        rt = np.array([s.get("retention_time", -1) for s in specs], np.float32)
    library = {}
    for z in np.unique(charge[valid]):
        rows = np.flatnonzero(valid & (charge == z))
        pos, off = _take_rows(oip, rows)
        key = "None" if z == 0 else str(int(z))
        library[key] = dict(precursor_mz=pmz[rows].astype(np.float32), retention_time=rt[rows], mz=omz[pos].astype(np.float32),
                            intensity=oit[pos].astype(np.float32), indptr=off, cluster=ids[rows])
        np.savez(os.path.join(spectra_dir, f"library_charge_{key}.npz"), **library[key])
    return library, first_new


def _dataset(part):
    return cluster.SpectrumDataset(part["precursor_mz"], part["retention_time"], part["mz"], part["intensity"], part["indptr"])


def _assign_charge(pipe, part, charge, lib, rows_all, csv_blocks=None):
    """`--assign_to`, one charge: every spectrum whose nearest representative lies within the threshold takes that cluster's id
    (its CSV row is written here: a tuple in `rows_all`, or with `csv_blocks` one column block for the device writer) -> the
    partition of the spectra that are left (same columns, rows in order), None when none is left"""
    n = len(part["precursor_mz"])
    best_row, _, _, assigned = cluster.assign_to_library(
        _dataset(part), _dataset(lib), config.eps, config.precursor_tol[0], config.precursor_tol[1], config.rt_tol,
        config.fragment_tol, config.min_matched_peaks, pipeline=pipe)
    ids = lib["cluster"][best_row[assigned]]
    logger.info("Charge %s: assigned %d of %d spectra to %d existing clusters", charge, int(assigned.sum()), n, len(np.unique(ids)))
    if csv_blocks is not None:
        took = np.flatnonzero(assigned)
        csv_blocks.append(csv_io.column_block(part["filename"][took], part["identifier"][took], charge, part["precursor_mz"][took],
                                              part["retention_time"][took], np.asarray(ids, np.int64)))
    for i, cid in zip(np.flatnonzero(assigned) if csv_blocks is None else (), ids):
        rows_all.append((str(part["filename"][i]), str(part["identifier"][i]), charge, np.float32(part["precursor_mz"][i]),
                         np.float32(part["retention_time"][i]), int(cid)))
    rest = np.flatnonzero(~assigned)
    if len(rest) == 0:
        return None
    pos, off = _take_rows(part["indptr"], rest)
    return dict(identifier=part["identifier"][rest], filename=part["filename"][rest], precursor_mz=part["precursor_mz"][rest],
                retention_time=part["retention_time"][rest], mz=part["mz"][pos], intensity=part["intensity"][pos], indptr=off)


def _setup_work_dir():
    """falcon.py:70-122: the work directory (a temporary one unless --work_dir) and the refusal to clobber existing outputs
    unless --overwrite -> (remove the work directory at the end, exit code or 0)"""
    rm_work_dir = False
    if config.work_dir is None:
        config.work_dir = tempfile.mkdtemp()
        rm_work_dir = True
    elif os.path.isdir(config.work_dir):
        logging.warning("Working directory %s already exists, previous results might get overwritten",
                        config.work_dir)
    spectra_dir = os.path.join(config.work_dir, "spectra")
    os.makedirs(spectra_dir, exist_ok=True)

    # falcon.py:86-122: refuse to clobber existing outputs unless --overwrite
    exit_exists = False
    outputs = [(".csv", "cluster assignments"), (".mgf", "cluster representatives")]
    if config.cluster_summary:
        outputs += [(".clusters.csv", "cluster summary"), (".scores.csv", "member scores")]
    if config.network:
        outputs += [(".network.csv", "representative network")]
    if config.network_families:
        outputs += [(".families.csv", "molecular families")]
    if config.network_graphml:
        outputs += [(".network.graphml", "representative network as GraphML")]
    if config.library:
        outputs += [(".library.csv", "library hits")]
    if config.library_propagate:
        outputs += [(".annotations.csv", "propagated annotations")]
    for ext, what in outputs:
        fn = f"{config.output_filename}{ext}"
        if os.path.isfile(fn):
            if config.overwrite:
                logger.warning("Output file %s (%s) already exists and will be overwritten", fn, what)
                os.remove(fn)
            else:
                logger.error("Output file %s (%s) already exists, aborting...", fn, what)
                exit_exists = True
    return rm_work_dir, 1 if exit_exists else 0


def _load_or_prepare(spectra_dir: str, ctx) -> List[str]:
    """the charge partitions of the work directory: read back, or prepared from the peak files (falcon.py:124-149)"""
    _, min_mz, max_mz = spectrum.get_dim(config.min_mz, config.max_mz, config.fragment_tol)   # falcon.py:124-126
    if config.overwrite:
        for fn in os.listdir(spectra_dir):
            os.remove(os.path.join(spectra_dir, fn))
    charge_path = os.path.join(spectra_dir, "charges.json")
    if os.path.isfile(charge_path) and not config.overwrite:                                   # falcon.py:143-149
        with open(charge_path) as f:
            charges = json.load(f)
    else:
        charges = _prepare_spectra(spectra_dir, min_mz, max_mz, ctx)
        with open(charge_path, "w") as f:
            json.dump(charges, f)
    return charges


def _ann_params():
    return cluster.AnnParams(eps=config.eps, low_dim=config.low_dim, n_probe=config.n_probe,
                            n_neighbors=config.n_neighbors, n_neighbors_ann=config.n_neighbors_ann,
                            mz_interval=config.mz_interval, min_mz=config.min_mz, max_mz=config.max_mz,
                            rescore=config.rescore, clustering=config.clustering, dtype=config.dtype,
                            exact=config.exact)


def _consensus(ctx, part, charge, labels, medoids):
    """`--representatives consensus`: the consensus peaks of one charge's clusters (`fal_consensus_spectra`) as host arrays
    (indptr, mz, intensity); None with medoid representatives"""
    if config.representatives != "consensus" or not config.export_representatives:
        return None
    from ._lib import CONS_FALLBACK, CONS_GLOBAL
    indptr, mz, it, status = ctx.consensus_spectra(part["mz"], part["intensity"], part["indptr"], labels, medoids,
                                                   config.fragment_tol, config.consensus_min_fraction)
    status = status.cpu().numpy()
    # (CONS_GLOBAL only says which sort a large cluster took; the peak count given as capacity always suffices, so the
    # capacity bit -- or a bit this code does not know -- is an error)
    bad = status & ~(CONS_FALLBACK | CONS_GLOBAL)
    if bad.any():
        raise RuntimeError(f"consensus representatives of charge {charge}: status bits {int(np.bitwise_or.reduce(bad))} on "
                           f"{int((bad != 0).sum())} clusters")
    logger.info("Consensus representatives of charge %s: %d clusters, %d fell back to their medoid (no merged peak reached "
                "the quorum)", charge, len(status), int(((status & CONS_FALLBACK) != 0).sum()))
    return indptr.cpu().numpy(), mz.cpu().numpy(), it.cpu().numpy()


def _summary_block(pipe, ds, part, charge, labels, medoids, consensus, current_label):
    """`--cluster_summary`, one charge: the members scored against their representatives (the medoids, or the consensus peaks
    the exported MGF holds) and the per-cluster columns -> the charge's block of `summary_io`"""
    cols = cluster.cluster_summary(ds, labels, medoids, config.fragment_tol, consensus=consensus, pipeline=pipe)
    cols.update(charge=charge, cluster=np.arange(len(medoids), dtype=np.int64) + current_label,
                labels=np.asarray(labels, np.int64) + current_label, filename=part["filename"], identifier=part["identifier"],
                medoids=np.asarray(medoids, np.int64))
    logger.info("Cluster summary of charge %s: %d clusters, mean member similarity %.4f", charge, len(medoids),
                float(np.mean(cols["similarity"], dtype=np.float64)))
    return cols


def _network_block(pipe, ds, charge, medoids, consensus, current_label):
    """`--network`, one charge: the links between its clusters' representatives (the medoids, or the consensus peaks the exported
    MGF holds) -> the charge's block of `network_io`"""
    cols = cluster.representative_network(ds, medoids, config.fragment_tol, config.network_max_shift, config.network_min_cosine,
                                          config.network_min_matched_peaks, config.network_top_k, consensus=consensus, pipeline=pipe,
                                          on_device=config.network_families)
    logger.info("Representative network of charge %s: %d clusters, %d links", charge, len(medoids), len(cols["a"]))
    if config.network_families:          # (the links stay on the device from the edge kernels to the family ids)
        cols = cluster.network_families(cols, len(medoids), config.network_max_family_size, config.network_family_delta,
                                        pipeline=pipe)
        logger.info("Molecular families of charge %s: %d families, %d links cut in %d rounds", charge, cols["n_families"],
                    cols["n_cut"], cols["n_rounds"])
    cols.update(charge=charge, first=current_label)
    return cols


def _is_msp(filename: str) -> bool:
    return filename.lower().endswith(".msp")


def _library_columns(ctx, chunks, min_mz, max_mz):
    """the `EntryChunk`s of the library readers, preprocessed -> `_load_annotation_library`'s dict"""
    cols, read, valid, oip, omz, oit = _process_entry_chunks(ctx, chunks, min_mz, max_mz)
    text = {k: cols.get(k, cols["filename"]) for k in ("name", "adduct", "smiles", "inchikey", "ionmode")}       # (no chunk: all empty)
    text.update(library_id=cols.get("identifier", cols["filename"]), library_file=np.array([os.path.basename(fn) for fn in cols["filename"]], dtype=str))
    if not read.any():
        return dict({k: text[k][:0] for k in ("library_id", "name", "library_file", "adduct", "smiles", "inchikey", "ionmode")}, precursor_mz=np.zeros(0, np.float32), charge=np.zeros(0, np.int32),
                    mz=np.zeros(0, np.float32), intensity=np.zeros(0, np.float32), indptr=np.zeros(1, np.int64))
    logger.info("Skipped %d library spectra the preprocessing rejects", int((read & ~valid).sum()))
    rows = np.flatnonzero(valid)
    pos, off = _take_rows(oip, rows)
    return dict({k: text[k][rows] for k in ("library_id", "name", "library_file", "adduct", "smiles", "inchikey", "ionmode")},
                precursor_mz=cols["precursor_mz"][rows].astype(np.float32), charge=cols["precursor_charge"][rows],
                mz=omz[pos].astype(np.float32), intensity=oit[pos].astype(np.float32), indptr=off)


def _load_library_by_format(ctx, filenames, min_mz, max_mz):
    """a `--library` list that names an MSP file: every file by the reader of its format (`.msp`, any letter case: `msp_io` under
    `--msp_reader`; else `mgf_io` under `--mgf_reader`), in the order of the command line.  A host reader's entries become host
    `EntryChunk`s, so one preprocessing path serves every mix."""
    from .ms_io import msp_io
    chunks, entries, skipped, n_files = [], 0, 0, {"MGF": 0, "MSP": 0}
    for fn in filenames:
        fmt, io_mod, reader = ("MSP", msp_io, config.msp_reader) if _is_msp(fn) else ("MGF", mgf_io, config.mgf_reader)
        counts = {}
        if reader == "device":
            chunks += io_mod.read_annotation_library([fn], counts, ctx=ctx)
        else:
            specs = io_mod.read_annotation_library([fn], counts)
            if specs:
                chunks.append(mgf_io._host_entry_chunk(specs, mgf_io._ANNOTATION_COLUMNS, fn))
        logger.debug("Library %s %s: %d entries by the %s reader, %d of them decided by the host rule", fmt, fn, counts["entries"], reader,
                     counts.get("host", counts["entries"]))
        entries, skipped = entries + counts["entries"], skipped + counts["skipped"]
        n_files[fmt] += 1
    logger.info("Read %d library spectra from %d file(s) (%d MGF, %d MSP), skipped %d entries without a usable precursor or with "
                "malformed peaks", entries - skipped, len(filenames), n_files["MGF"], n_files["MSP"], skipped)
    return _library_columns(ctx, chunks, min_mz, max_mz)


def _load_annotation_library(ctx):
    """`--library`: the entries of the reference library files, preprocessed with the run's options (scaling included: a
    reference library holds raw intensities, unlike `--assign_to`'s exported representatives) -> dict of host columns by entry
    that survived: the peak CSR, precursor_mz f32, charge i32 (0: none) and the annotation strings.  A file named `.msp` is read
    as an MSP library (`_load_library_by_format`), every other one as MGF."""
    _, min_mz, max_mz = spectrum.get_dim(config.min_mz, config.max_mz, config.fragment_tol)
    counts = {}
    filenames = [os.path.abspath(fn) for fn in config.library]
    if any(_is_msp(fn) for fn in filenames):
        return _load_library_by_format(ctx, filenames, min_mz, max_mz)
    if config.mgf_reader == "device":                    # the text parsed on the device, the peaks left there (mgf_io.read_annotation_chunks)
        chunks = mgf_io.read_annotation_library(filenames, counts, ctx=ctx)
        logger.info("Read %d library spectra from %d file(s), skipped %d entries without a usable precursor or with a malformed "
                    "peak line", counts["entries"] - counts["skipped"], len(config.library), counts["skipped"])
        logger.debug("Library MGFs: %d of %d entries decided by the host reader", counts["host"], counts["entries"])
        return _library_columns(ctx, chunks, min_mz, max_mz)
    specs = mgf_io.read_annotation_library(filenames, counts)
    logger.info("Read %d library spectra from %d file(s), skipped %d entries without a usable precursor or with a malformed peak "
                "line", len(specs), len(config.library), counts["skipped"])
    text = lambda k: np.array([str(s[k]) for s in specs], dtype=str)
    cols = dict(library_id=text("identifier"), name=text("name"), library_file=np.array([os.path.basename(s["filename"]) for s in specs],
                                                                                        dtype=str),
                adduct=text("adduct"), smiles=text("smiles"), inchikey=text("inchikey"), ionmode=text("ionmode"))
    pmz = np.array([s["precursor_mz"] for s in specs], np.float64)
    charge = np.array([int(s["precursor_charge"]) for s in specs], np.int32)
    if not specs:
        return dict(cols, precursor_mz=np.zeros(0, np.float32), charge=charge, mz=np.zeros(0, np.float32),
                    intensity=np.zeros(0, np.float32), indptr=np.zeros(1, np.int64))
    mz, it, indptr = _raw_csr(specs)
    valid, oip, omz, oit = _process(ctx, mz, it, indptr, pmz, charge, min_mz, max_mz)
    logger.info("Skipped %d library spectra the preprocessing rejects", int((~valid).sum()))
    rows = np.flatnonzero(valid)
    pos, off = _take_rows(oip, rows)
    return dict({k: v[rows] for k, v in cols.items()}, precursor_mz=pmz[rows].astype(np.float32), charge=charge[rows],
                mz=omz[pos].astype(np.float32), intensity=oit[pos].astype(np.float32), indptr=off)


def _library_block(pipe, ds, charge, medoids, consensus, current_label, reference, spectra_dir):
    """`--library`, one charge: the best hits of its clusters' representatives (the medoids, or the consensus peaks the exported
    MGF holds) among the library entries of the charge and those without one -> the charge's block of `library_io`.  The
    charge's library is also left in the work directory (`reference_charge_<z>.npz`): what the run searched"""
    z = 0 if charge == "None" else int(charge)
    rows = np.flatnonzero((reference["charge"] == z) | (reference["charge"] == 0))
    pos, off = _take_rows(reference["indptr"], rows)
    lib = dict({k: reference[k][rows] for k in ("library_id", "name", "library_file", "adduct", "smiles", "inchikey", "ionmode",
                                                "charge")},
               precursor_mz=reference["precursor_mz"][rows], retention_time=np.full(len(rows), -1.0, np.float32),
               mz=reference["mz"][pos], intensity=reference["intensity"][pos], indptr=off)
    np.savez(os.path.join(spectra_dir, f"reference_charge_{charge}.npz"), **lib)
    cols = cluster.library_search(ds, medoids, _dataset(lib), config.fragment_tol, config.precursor_tol[0], config.precursor_tol[1],
                                  config.library_analog, config.library_max_shift, config.library_min_cosine,
                                  config.library_min_matched_peaks, config.library_top_n, consensus=consensus, pipeline=pipe)
    logger.info("Library search of charge %s: %d clusters against %d library spectra, %d hits for %d clusters", charge, len(medoids),
                len(rows), len(cols["cluster"]), len(np.unique(cols["cluster"])))
    cols.update({k: lib[k] for k in ("library_id", "name", "library_file", "adduct", "smiles", "inchikey")},
                library_precursor_mz=lib["precursor_mz"], charge=charge, first=current_label)
    return cols


def _propagate_block(pipe, ds, charge, medoids, network, hits):
    """`--library_propagate`, one charge: the names of its clusters' rank-1 library hits carried along the surviving links of its
    families (`network` and `hits` are the charge's blocks of `network_io` and `library_io`) -> the charge's block of
    `annotation_io`"""
    cols = cluster.propagate_annotations(network, hits, len(medoids), config.library_propagate_hops,
                                         config.library_propagate_min_score, pipeline=pipe)
    logger.info("Annotation propagation of charge %s: %d annotated clusters, %d more reached in %d levels", charge, cols["n_seeds"],
                cols["n_reached"], cols["n_levels"])
    pmz = np.asarray(ds.precursor_mz, np.float32)[np.asarray(medoids, np.int64)]
    hit = cols["hit"]
    cols.update({k: hits[k] for k in ("library_id", "name", "library_file", "adduct", "smiles", "inchikey")},
                family=network["node_family"][cols["cluster"]], n_families=network["n_families"],
                delta_mz=pmz[cols["cluster"]] - pmz[cols["source"]], library=hits["library"][hit],
                library_cosine=hits["similarity"][hit], charge=charge, first=network["first"])
    return cols


def _graphml_block(part, charge, labels, medoids, current_label, network, hits, annotations):
    """`--network_graphml`, one charge: per cluster the representative's precursor m/z and retention time (float32, as the cluster
    CSV prints them) and the member count, beside the charge's blocks of `network_io`, `library_io` and `annotation_io` (None
    without their options) -> the charge's block of `graphml_io`"""
    m = np.asarray(medoids, np.int64)
    return dict(charge=charge, first=current_label, precursor_mz=np.asarray(part["precursor_mz"])[m].astype(np.float32),
                retention_time=np.asarray(part["retention_time"])[m].astype(np.float32),
                size=np.bincount(np.asarray(labels, np.int64), minlength=len(m)).astype(np.int32), network=network, library=hits,
                annotations=annotations)


def _emit_charge(part, charge, labels, medoids, current_label, rows_all, representatives, consensus=None, csv_blocks=None) -> int:
    """one charge's labels (by row of its partition) and medoid rows -> CSV rows and the charge's block of representatives; ->
    the next label.  consensus (indptr, mz, intensity by cluster): the representatives' peaks; everything else stays the medoid's.
    csv_blocks (a list): the CSV rows as one column block for the device writer instead of a tuple per spectrum in `rows_all`"""
    n = len(part["precursor_mz"])
    labels = labels + current_label                                                            # falcon.py:189-193
    current_label = int(labels.max()) + 1
    if csv_blocks is not None:
        csv_blocks.append(csv_io.column_block(part["filename"], part["identifier"], charge, part["precursor_mz"], part["retention_time"],
                                              np.asarray(labels, np.int64)))
    for i in range(n if csv_blocks is None else 0):
        # float32 columns keep their own (shortest round-trip) text form, as pandas' to_csv prints them
        rows_all.append((str(part["filename"][i]), str(part["identifier"][i]), charge,
                         np.float32(part["precursor_mz"][i]), np.float32(part["retention_time"][i]), int(labels[i])))
    if config.export_representatives:                                                          # falcon.py:198-203
        # one block of arrays per charge: the peaks CSR (the partition's, with the medoid rows; or the consensus, one row per
        # cluster) and the medoids' columns
        m = np.asarray(medoids, np.int64)
        if consensus is None:
            indptr, mz, intensity, rows = part["indptr"], part["mz"], part["intensity"], m.astype(np.int32)
        else:
            indptr, mz, intensity = consensus
            rows = np.arange(len(m), dtype=np.int32)
        representatives.append(dict(
            indptr=indptr, mz=mz, intensity=intensity, rows=rows, identifier=part["identifier"][m],
            precursor_mz=part["precursor_mz"][m], retention_time=part["retention_time"][m],
            charge=None if charge == "None" else int(charge), cluster=labels[m].astype(np.int64)))
    return current_label


def _block_columns(b):
    """a block of `_emit_charge` -> the columns `mgf_io.write_representatives` / `mgf_io.entry_dicts` take in front of the titles"""
    return (b["mz"], b["intensity"], b["indptr"], b["rows"], b["precursor_mz"], b["retention_time"],
            np.full(len(b["rows"]), b["charge"] or 0, np.int32), b["cluster"])


def _representative_spectra(blocks):
    """the blocks of `_emit_charge` -> the dicts the host writer takes, in the blocks' order"""
    for b in blocks:
        yield from mgf_io.entry_dicts(*_block_columns(b), b["identifier"])


def _device_writable(blocks) -> bool:
    """the device writer formats float32 columns and int32 charges: the partitions' own types"""
    f32 = all(np.asarray(b[c]).dtype == np.float32 for b in blocks for c in ("mz", "intensity", "precursor_mz", "retention_time"))
    return f32 and all(b["charge"] is None or (b["charge"] != 0 and abs(b["charge"]) < 2 ** 31) for b in blocks)


def _write_representatives(filename: str, blocks, ctx) -> None:
    """the MGF of representatives: block after block through the device writer (`--mgf_writer device`, with `ctx`), or every
    entry through the host writer (also where a title is outside what the device path mirrors); the same bytes"""
    blobs = None
    if config.mgf_writer == "device" and ctx is not None and _device_writable(blocks):
        blobs = [mgf_io.title_blob(b["identifier"]) for b in blocks]
    if blobs is None or any(t is None for t in blobs):
        ms_io.write_spectra(filename, _representative_spectra(blocks))
        return
    open(filename, "wb").close()
    for b, titles in zip(blocks, blobs):
        ms_io.write_representatives(filename, ctx, *_block_columns(b), titles, append=True)


def _write_cluster_info_device(blocks, ctx) -> bool:
    """the CSV of the column blocks through the device writer: the header as host text, the rows sorted and formatted on `ctx`
    (`csv_io`) -> True; False, with one debug line and nothing written, where the file is the host writer's"""
    why = "no device context" if ctx is None else None
    cols = order = None
    if why is None:
        cols, why = csv_io.device_columns(blocks, _natural_key)
    if why is None:
        order = csv_io.sort_rows(ctx, cols)
        if order is None:
            why = "an identifier holds a digit run longer than int() takes"
    if why is not None:
        logger.debug("csv_writer: the host writer writes %s.csv: %s", config.output_filename, why)
        return False
    with open(f"{config.output_filename}.csv", "a", newline="") as f:
        _write_csv_header(f)
        f.flush()
        csv_io.write_rows(f.buffer, ctx, cols, order)
    return True


def _write_outputs(rows_all, representatives, ctx=None, csv_blocks=None) -> None:
    """falcon.py:206-244: the CSV on a worker thread, the MGF of representatives on the calling one (the device writer runs on
    `ctx`; a new thread would not inherit the device).  csv_blocks: the CSV's rows as column blocks (`--csv_writer device`):
    sorted and formatted on `ctx`, on the calling thread too, or turned into tuples where the host writer has to write them"""
    if csv_blocks:
        n_rows = len(rows_all) + sum(len(b["cluster"]) for b in csv_blocks)
        n_clusters = len(np.unique(np.concatenate([np.asarray(b["cluster"], np.int64) for b in csv_blocks] +
                                                  [np.array([r[5] for r in rows_all], np.int64)])))
    else:
        n_rows, n_clusters = len(rows_all), len({r[5] for r in rows_all})
    logger.info("Export cluster assignments of %d spectra to %d unique clusters to output file %s",
                n_rows, n_clusters, f"{config.output_filename}.csv")
    if csv_blocks is not None:
        if not rows_all and _write_cluster_info_device(csv_blocks, ctx):
            if config.export_representatives:
                _export_representatives(representatives, ctx)
            return
        rows_all = list(rows_all) + list(csv_io.block_tuples(csv_blocks))
    rows_all.sort(key=lambda r: (_natural_key(r[0]), _natural_key(r[1])))                      # falcon.py:206-208
    csv_worker = threading.Thread(target=_write_cluster_info, args=(rows_all,), daemon=True)
    csv_worker.start()
    try:
        if config.export_representatives:
            _export_representatives(representatives, ctx)
    finally:
        csv_worker.join()


def _export_representatives(representatives, ctx) -> None:
    logger.info("Export %d cluster representative spectra to output file %s",
                sum(len(b["rows"]) for b in representatives), f"{config.output_filename}.mgf")
    _write_representatives(f"{config.output_filename}.mgf", representatives, ctx)


def _run_distributed() -> int:
    """`--distributed`: one rank of a job launched by `python -m torch.distributed.run --module falcon_amd.falcon ...`.
    Rank 0 sets the work directory up, checks the outputs and prepares the charge partitions; every rank then clusters its
    share of every partition (`PartitionRunner.run(shard=(rank, world))`: precursor windows / buckets dealt on the cost
    model of the mode, exact or nearest-neighbour), one all-gatherv round assembles every partition on every rank
    (`distributed.gather_partitions`) and rank 0 writes the outputs.  Cluster ids are rank-major; the partition and the
    representatives are those of one process.  Backend RCCL ("nccl"), or gloo with FALCON_DIST_BACKEND=gloo; device
    LOCAL_RANK, or FALCON_DIST_DEVICE (RCCL refuses two ranks on one device: the gloo + one-device form is for tests).
    Every rank reads the partitions from rank 0's work directory: the ranks must share a filesystem (one node, or a
    `--work_dir` on a shared mount)."""
    import torch
    import torch.distributed as dist
    from . import distributed as fdist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    device = int(os.environ.get("FALCON_DIST_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    backend = "gloo" if os.environ.get("FALCON_DIST_BACKEND") == "gloo" else "nccl"
    torch.cuda.set_device(device)
    dev = torch.device("cuda", device)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        state = [None, 0, False]                                  # work_dir, exit code, remove the work dir at the end
        if rank == 0:
            rm_work_dir, exit_code = _setup_work_dir()
            state = [config.work_dir, exit_code, rm_work_dir]
            if not exit_code:
                # a context of its own for the preprocessing, released before the clustering (the runner's slots make theirs)
                from .device import Context
                prep = Context(device)
                try:
                    _load_or_prepare(os.path.join(config.work_dir, "spectra"), prep)
                finally:
                    prep.close()
                    torch.cuda.empty_cache()
        dist.broadcast_object_list(state, src=0)
        dist.barrier()
        if state[1]:
            return state[1]
        config.work_dir = state[0]
        spectra_dir = os.path.join(config.work_dir, "spectra")
        with open(os.path.join(spectra_dir, "charges.json")) as f:
            charges = json.load(f)
        p = cluster.resolve_params(config.linkage, config.distance_threshold, config.min_matched_peaks, _ann_params())
        parts, sets = [], []
        for charge in charges:
            part = np.load(os.path.join(spectra_dir, f"spectra_charge_{charge}.npz"))
            parts.append(part)
            sets.append(cluster.SpectrumDataset(part["precursor_mz"], part["retention_time"], part["mz"], part["intensity"],
                                                part["indptr"]))                      # host-resident: a rank uploads its rows
        runner = cluster.PartitionRunner(device, 2)
        try:
            outs = runner.run(sets, config.precursor_tol[0], config.precursor_tol[1], config.rt_tol, config.fragment_tol,
                              config.batch_size, p, shard=(rank, world))
            merged = fdist.gather_partitions(outs, runner.lasts, [len(ds) for ds in sets],
                                             dev if backend == "nccl" else torch.device("cpu"))
        finally:
            runner.close()
        if rank == 0:
            rows_all, current_label, representatives = [], 0, []
            csv_blocks = [] if config.csv_writer == "device" else None
            # a context of rank 0's own for the consensus and for the device writers, as for the preparation of the partitions
            out_ctx = None
            if csv_blocks is not None or (config.export_representatives and
                                          (config.representatives == "consensus" or config.mgf_writer == "device")):
                from .device import Context
                out_ctx = Context(device)
            try:
                for charge, part, (labels, medoids) in zip(charges, parts, merged):
                    if len(labels):
                        cons = (_consensus(out_ctx, part, charge, labels, medoids)
                                if out_ctx is not None and config.representatives == "consensus" else None)
                        current_label = _emit_charge(part, charge, labels, medoids, current_label, rows_all, representatives, cons,
                                                     csv_blocks=csv_blocks)
                _write_outputs(rows_all, representatives, out_ctx, csv_blocks=csv_blocks)
            finally:
                if out_ctx is not None:
                    out_ctx.close()
        dist.barrier()
        if rank == 0 and state[2]:
            shutil.rmtree(config.work_dir)
        return 0
    finally:
        dist.destroy_process_group()


def _raw_csr(specs):
    """spectra read from one peak file -> raw CSR (peaks sorted by m/z inside every spectrum, which is
    what spectrum_utils does when the reference constructs an MsmsSpectrum)."""
    return mgf_io.raw_csr(specs)


def _take_rows(indptr: np.ndarray, rows: np.ndarray):
    """positions of the peaks of `rows` in CSR order, and the CSR offsets of the selection"""
    cnt = indptr[rows + 1] - indptr[rows]
    out = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(cnt, out=out[1:])
    pos = np.repeat(indptr[rows] - out[:-1], cnt) + np.arange(out[-1])
    return pos, out


def _process(ctx, mz, it, indptr, pmz, charge, min_mz, max_mz, scaling="config"):
    """`fal_process_spectra` over one raw CSR (host or device arrays) -> valid, out indptr, mz, intensity as host arrays"""
    if scaling == "config":
        scaling = None if config.scaling == "off" else config.scaling
    valid, oip, omz, oit = ctx.process_spectra(
        mz, it, indptr, pmz, charge, config.min_peaks, config.min_mz_range, min_mz, max_mz,
        config.remove_precursor_tol, config.min_intensity, config.max_peaks_used, scaling)
    return valid.cpu().numpy(), oip.cpu().numpy(), omz.cpu().numpy(), oit.cpu().numpy()


def _process_entry_chunks(ctx, chunks, min_mz, max_mz, scaling="config"):
    """`fal_process_spectra` over every `mgf_io.EntryChunk` of a library or representative reader, the peaks of a device chunk
    left on the device (preprocessing is per spectrum: the chunks' results side by side are one call's) -> the chunks' columns
    side by side (plus `filename`), `read` (False: a row the reader dropped), valid (False for those too), and the out indptr,
    mz and intensity over all rows as host arrays"""
    names = list(chunks[0].columns) if chunks else []
    cols = {k: np.concatenate([c.columns[k] for c in chunks]) for k in names}
    cols["filename"] = np.concatenate([np.array([c.filename] * len(c), dtype=str) for c in chunks]) if chunks else np.zeros(0, dtype=str)
    read = np.concatenate([~c.dropped for c in chunks]) if chunks else np.zeros(0, bool)
    valid, sizes, mzs, its = [], [], [], []
    for c in chunks:
        v, oip, omz, oit = _process(ctx, c.mz, c.intensity, c.indptr, c.columns["precursor_mz"], c.columns["precursor_charge"],
                                    min_mz, max_mz, scaling)
        valid.append(v & ~c.dropped)
        sizes.append(np.diff(oip))
        mzs.append(omz[:oip[-1]])
        its.append(oit[:oip[-1]])
    indptr = np.zeros(len(read) + 1, np.int64)
    if chunks:
        np.cumsum(np.concatenate(sizes), out=indptr[1:])
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)          # noqa: E731
    return cols, read, cat(valid, bool), indptr, cat(mzs, np.float32), cat(its, np.float32)


def _partition(parts, fn, ident, pmz, rt, charge, valid, oip, omz, oit) -> None:
    """append the valid spectra of one batch to their charge partitions"""
    for z in np.unique(charge[valid]):
        rows = np.flatnonzero(valid & (charge == z))
        pos, off = _take_rows(oip, rows)
        p = parts.setdefault("None" if z == 0 else str(int(z)),
                             dict(identifier=[], filename=[], precursor_mz=[], retention_time=[], mz=[], intensity=[],
                                  counts=[]))
        p["identifier"].append(ident[rows])
        p["filename"].append(np.array([fn] * len(rows), dtype=str))
        p["precursor_mz"].append(pmz[rows].astype(np.float32))
        p["retention_time"].append(rt[rows])
        p["mz"].append(omz[pos])
        p["intensity"].append(oit[pos])
        p["counts"].append(np.diff(off))


def _prepare_chunk(chunk, fn, parts, min_mz, max_mz, ctx) -> int:
    """one PeakChunk of an mzML / mzXML file: `fal_decode_peaks` -> `fal_process_spectra` with the peaks left on the device
    -> charge partitions.  A spectrum whose arrays do not decode is dropped and logged.  -> the low-quality count (spectra
    process_spectrum rejects, undecodable ones and those the reader skipped as unsupported)."""
    from ._lib import PEAK_STATUS
    for reason, k in sorted(chunk.skipped.items()):
        logger.warning("Skipped %d spectra of %s: %s", k, fn, reason)
    dropped = sum(chunk.skipped.values())
    if not len(chunk):
        return dropped
    payload, arrays, spec = chunk.tables()
    indptr, mz, it, status = ctx.decode_peaks(payload, arrays, spec)
    pmz = np.array(chunk.precursor_mz, np.float64)
    charge = np.array([int(c) if c else 0 for c in chunk.precursor_charge], np.int32)
    valid, oip, omz, oit = _process(ctx, mz, it, indptr, pmz, charge, min_mz, max_mz)
    status = status.cpu().numpy()
    bad = status != 0
    if bad.any():
        for bit, what in PEAK_STATUS.items():
            k = int(((status & bit) != 0).sum())
            if k:
                logger.warning("Skipped %d spectra of %s: binary array not decoded (%s)", k, fn, what)
        valid = valid & ~bad
    ident = np.array(chunk.identifier, dtype=str)
    rt = np.array(chunk.retention_time, np.float32)
    _partition(parts, fn, ident, pmz, rt, charge, valid, oip, omz, oit)
    return dropped + int((~valid).sum())


def _prepare_mgf_chunk(chunk, fn, parts, min_mz, max_mz, ctx) -> int:
    """one MgfChunk of the device reader: `fal_process_spectra` with the peaks left on the device -> charge partitions.
    Spectra the host reader rejects are no spectra (they are skipped silently, as `get_spectra` skips them).
    -> the low-quality count"""
    if not len(chunk):
        return 0
    valid, oip, omz, oit = _process(ctx, chunk.mz, chunk.intensity, chunk.indptr, chunk.precursor_mz, chunk.precursor_charge,
                                    min_mz, max_mz)
    _partition(parts, fn, chunk.identifier, chunk.precursor_mz, chunk.retention_time.astype(np.float32), chunk.precursor_charge,
               valid & ~chunk.dropped, oip, omz, oit)
    return int((~valid & ~chunk.dropped).sum())


def _prepare_spectra(spectra_dir: str, min_mz: float, max_mz: float, ctx) -> List[str]:
    """falcon.py:247-328: read every peak file, preprocess (`process_spectrum`, spectrum.py:73-169 -- here one
    `fal_process_spectra` call per file on the GPU), partition by precursor charge, one CSR `.npz` per charge.
    mzML / mzXML files go through their reader's chunks, `fal_decode_peaks` and `fal_process_spectra` with the peaks left on
    the device (one chunk per call; a file whose payload is larger than one chunk is split between spectra).  MGF files go
    through the device reader (`mgf_io.read_chunks`) unless `--mgf_reader host`: same spectra, same partitions."""
    filenames = [fn for pattern in config.input_filenames for fn in glob.glob(pattern)]
    logger.info("Read spectra from %d peak file(s)", len(filenames))
    parts: Dict[str, Dict[str, list]] = {}
    low_quality = 0
    for fn in filenames:
        fn = os.path.abspath(fn)
        read_chunks = ms_io.chunk_reader(fn)
        if read_chunks is not None:                      # mzML / mzXML: binary arrays decoded on the device (fal_decode_peaks)
            read_device = ms_io.device_chunk_reader(fn) if config.mzml_reader == "device" else None
            if read_device is None:
                for chunk in read_chunks(fn):
                    low_quality += _prepare_chunk(chunk, fn, parts, min_mz, max_mz, ctx)
                continue
            n_device = n_host = 0                        # mzML: the structure scanned on the device too (fal_mzml_index / _parse)
            for chunk in read_device(fn, ctx):
                low_quality += _prepare_chunk(chunk, fn, parts, min_mz, max_mz, ctx)
                n_device += getattr(chunk, "n_device", 0)
                n_host += getattr(chunk, "n_host", len(chunk))
            logger.debug("mzML file %s: %d spectra decided on the device, %d handed to the host reader", fn, n_device, n_host)
            continue
        read_mgf = ms_io.device_reader(fn) if config.mgf_reader == "device" else None
        if read_mgf is not None:                         # MGF: the text parsed on the device (fal_mgf_index / fal_mgf_parse)
            n_host = n_read = 0
            for chunk in read_mgf(fn, ctx):
                low_quality += _prepare_mgf_chunk(chunk, fn, parts, min_mz, max_mz, ctx)
                n_host, n_read = n_host + chunk.n_host, n_read + len(chunk)
            logger.debug("MGF file %s: %d spectra parsed on the device, %d of them decided by the host reader", fn, n_read, n_host)
            continue
        specs = list(ms_io.get_spectra(fn))
        if not specs:
            continue
        mz, it, indptr = _raw_csr(specs)
        pmz = np.array([s["precursor_mz"] for s in specs], np.float64)
        charge = np.array([int(s["precursor_charge"]) if s.get("precursor_charge") else 0 for s in specs], np.int32)
        valid = _process(ctx, mz, it, indptr, pmz, charge, min_mz, max_mz)
        low_quality += int((~valid[0]).sum())
        ident = np.array([str(s["identifier"]) for s in specs], dtype=str)
        rt = np.array([s.get("retention_time", -1) for s in specs], np.float32)
        _partition(parts, fn, ident, pmz, rt, charge, *valid)
    n_total = 0
    for charge, p in parts.items():
        counts = np.concatenate(p["counts"])
        indptr = np.zeros(len(counts) + 1, np.int64)
        np.cumsum(counts, out=indptr[1:])
        np.savez(os.path.join(spectra_dir, f"spectra_charge_{charge}.npz"),
                 identifier=np.concatenate(p["identifier"]), filename=np.concatenate(p["filename"]),
                 precursor_mz=np.concatenate(p["precursor_mz"]), retention_time=np.concatenate(p["retention_time"]),
                 mz=np.concatenate(p["mz"]).astype(np.float32), intensity=np.concatenate(p["intensity"]).astype(np.float32),
                 indptr=indptr)
        n_total += len(counts)
    logger.info("Read %d spectra from %d peak files", n_total, len(filenames))
    logger.info("Skipped %d low-quality spectra", low_quality)
    return sorted(parts, key=_natural_key)


def _header_lines() -> List[str]:
    """the `#` lines in front of the cluster CSV and of the cluster summary's files"""
    return [f"falcon version {__version__}"] + _option_lines(header=True)


def _write_csv_header(f):
    """the `#` lines and the column row -> the csv writer that wrote it"""
    import csv
    for line in _header_lines():
        f.write(f"# {line}\n")
    f.write("#\n")
    w = csv.writer(f, quoting=csv.QUOTE_MINIMAL, lineterminator="\n")
    w.writerow(csv_io.COLUMNS)
    return w


def _write_cluster_info(rows) -> None:
    """falcon.py:483-524: `#` header block with every option, then the CSV table (pandas `to_csv` conventions:
    minimal quoting with doubled quotes, float32 columns in their shortest round-trip form)."""
    with open(f"{config.output_filename}.csv", "a", newline="") as f:
        w = _write_csv_header(f)
        for fn, sid, charge, pmz, rt, lab in rows:
            w.writerow([fn, sid, charge, str(np.float32(pmz)), str(np.float32(rt)), lab])


if __name__ == "__main__":
    sys.exit(main())
