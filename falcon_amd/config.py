"""Command-line / INI configuration with falcon's option surface.

Mirrors reference falcon/config.py:24-212 (names, defaults, nargs, choices, `config.ini`
default file, `-c/--config`, attribute access, RuntimeError before `parse`) and ADDS the
nearest-neighbour options the README documents but the snapshot's parser lacks
(`--eps` README.md:49,73-79; `--n_probe`, `--n_neighbors`, `--n_neighbors_ann`
README.md:107-113; `--low_dim` README.md:114-117) plus the build's `--dtype`.  configargparse is not available, so
the INI layer is stdlib configparser: values from the file become defaults, the command
line overrides them (the precedence configargparse implements).
"""
from __future__ import annotations

import argparse
import configparser
import os
import shlex
from typing import List, Optional, Union

from . import __version__

_HELP_HEADER = ("falcon: Fast spectrum clustering using nearest neighbor searching\n"
                "=================================================================\n\n"
                f"falcon (MI355X build) version {__version__}\n\n"
                "Reference code website: https://github.com/bittremieux/falcon\n\n")


class Config:
    def __init__(self) -> None:
        p = argparse.ArgumentParser(description=_HELP_HEADER, formatter_class=argparse.RawDescriptionHelpFormatter)
        p.add_argument("-c", "--config", default=None, help="Config file path (default: config.ini if present).")
        # IO  (config.py:52-74)
        p.add_argument("input_filenames", nargs="+", help="Input peak files (supported formats: .mzML, .mzXML, .MGF).")
        p.add_argument("output_filename", help="Output file name.")
        p.add_argument("--work_dir", default=None, help="Working directory (default: temporary directory).")
        p.add_argument("--overwrite", action="store_true", help="Overwrite existing results.")
        p.add_argument("--export_representatives", action="store_true",
                       help="Export cluster representatives to an MGF file.")
        p.add_argument("--representatives", type=str, default="medoid", choices=["medoid", "consensus"],
                       help="Peaks of an exported representative: the cluster's medoid spectrum (default), or the consensus "
                            "of its members merged peak by peak (needs --export_representatives).")
        p.add_argument("--consensus_min_fraction", type=float, default=0.25,
                       help="Consensus representatives: a merged peak is kept when at least this fraction of the cluster's "
                            "members' worth of peaks falls into it (0 < q <= 1, default: 0.25).")
        p.add_argument("--cluster_summary", action="store_true",
                       help="Also write <output>.clusters.csv (per cluster: size, representative, smallest and mean similarity "
                            "of its members to the representative, the worst member, precursor m/z and retention-time spread) "
                            "and <output>.scores.csv (per spectrum: its similarity to its cluster's representative and the "
                            "matched peaks).  The representative is the medoid, or with --export_representatives "
                            "--representatives consensus the consensus spectrum.")
        p.add_argument("--network", action="store_true",
                       help="Also write <output>.network.csv: the molecular network of the cluster representatives.  Two clusters "
                            "of one precursor charge are linked when the greedy modified cosine of their representatives (peaks "
                            "matching at the same m/z or shifted by the precursor difference) passes the --network_* thresholds.  "
                            "The representative is the medoid, or with --export_representatives --representatives consensus the "
                            "consensus spectrum.")
        p.add_argument("--network_min_cosine", type=float, default=0.7,
                       help="--network: smallest modified cosine of a link (0 <= c <= 1, default: 0.7).")
        p.add_argument("--network_min_matched_peaks", type=int, default=6,
                       help="--network: smallest number of matched peaks of a link (default: 6).")
        p.add_argument("--network_top_k", type=int, default=10,
                       help="--network: a link is kept when it is among the top_k most similar links of both of its clusters "
                            "(default: 10; 0 = keep every link).")
        p.add_argument("--network_max_shift", type=float, default=200.0,
                       help="--network: largest precursor m/z difference of two linked clusters (default: 200.0).")
        p.add_argument("--network_families", action="store_true",
                       help="--network: also group the clusters into molecular families, the connected components of the "
                            "network, and write <output>.families.csv (per cluster: its family and the family's size).  A family "
                            "above --network_max_family_size is broken up by cutting its weakest links round by round; "
                            "<output>.network.csv then holds the surviving links only, with a family column.")
        p.add_argument("--network_max_family_size", type=int, default=100,
                       help="--network_families: the most clusters of one family (default: 100; 0 = no cap).")
        p.add_argument("--network_family_delta", type=float, default=0.02,
                       help="--network_families: a round cuts the links of an oversized family whose cosine is within this "
                            "much of the family's weakest link (default: 0.02).")
        p.add_argument("--network_graphml", action="store_true",
                       help="--network: also write <output>.network.graphml, one GraphML file for Cytoscape, Gephi or networkx: "
                            "a node per cluster (clusters without a link included), an edge per row of <output>.network.csv, "
                            "and on them the attributes of the run's other files -- the representative's precursor and the "
                            "cluster's size, with --network_families the family, with --library the rank-1 hit, with "
                            "--library_propagate the propagated annotation.")
        p.add_argument("--library", nargs="+", default=None, metavar="FILE",
                       help="Reference spectral library MGF files (GNPS style: PEPMASS, optional CHARGE, NAME= / COMPOUND_NAME=, "
                            "SPECTRUMID=): also write <output>.library.csv, for every cluster representative its best library "
                            "hits by greedy cosine among the library spectra of its charge (an entry without a charge is offered "
                            "to every charge) inside --precursor_tol.  The library is preprocessed with the run's options, "
                            "--scaling included.  The representative is the medoid, or with --export_representatives "
                            "--representatives consensus the consensus spectrum.")
        p.add_argument("--library_analog", action="store_true",
                       help="--library: analog search -- library spectra within --library_max_shift of the representative's "
                            "precursor, scored by the greedy modified cosine (peaks matching at the same m/z or shifted by the "
                            "precursor difference).")
        p.add_argument("--library_max_shift", type=float, default=200.0,
                       help="--library_analog: largest precursor m/z difference of a hit (default: 200.0).")
        p.add_argument("--library_min_cosine", type=float, default=0.7,
                       help="--library: smallest cosine of a hit (0 <= c <= 1, default: 0.7).")
        p.add_argument("--library_min_matched_peaks", type=int, default=6,
                       help="--library: smallest number of matched peaks of a hit (default: 6).")
        p.add_argument("--library_top_n", type=int, default=1,
                       help="--library: the most hits reported for one representative, best first (default: 1; 0 = all).")
        p.add_argument("--library_propagate", action="store_true",
                       help="--library with --network --network_families: also carry the library's names through the molecular "
                            "families and write <output>.annotations.csv -- for every cluster that has a library hit or lies "
                            "within --library_propagate_hops links of one, the nearest named cluster of its family, the links "
                            "between them and the product of their cosines.  Pass --network_max_family_size 0 to walk whole "
                            "components.")
        p.add_argument("--library_propagate_hops", type=int, default=3,
                       help="--library_propagate: the most links between a cluster and the named cluster its annotation comes "
                            "from (1 to 64, default: 3).")
        p.add_argument("--library_propagate_min_score", type=float, default=0.0,
                       help="--library_propagate: smallest product of the cosines along a path (0 <= s <= 1, default: 0.0).")
        p.add_argument("--assign_to", nargs="+", default=None, metavar="FILE",
                       help="Representative MGF files of earlier runs (--export_representatives output, one CLUSTER= id per "
                            "entry): a new spectrum whose nearest representative inside the precursor (and RT) tolerance lies "
                            "within the distance threshold takes that cluster's id; the rest are clustered among themselves "
                            "with ids above the files' largest.")
        # CLUSTERING  (config.py:76-124)
        p.add_argument("--precursor_tol", nargs=2, default=[20, "ppm"],
                       help='Precursor tolerance mass and mode (default: 20 ppm). Mode is "ppm" or "Da".')
        p.add_argument("--rt_tol", type=float, default=None, help="Retention time tolerance (default: none).")
        p.add_argument("--fragment_tol", type=float, default=0.05, help="Fragment mass tolerance in m/z.")
        p.add_argument("--linkage", type=str, default="complete", choices=["complete", "single", "average"],
                       help="Linkage of the hierarchical clustering (default: complete). single / average select "
                            "--clustering hierarchical when --clustering is not given (the reference honours them, "
                            "config.py:97-103); together with an explicit --clustering dbscan they are an error.")
        p.add_argument("--clustering", type=str, default=None, choices=["dbscan", "hierarchical"],
                       help="dbscan (README: density clustering of the neighbour graph, default) or hierarchical "
                            "(the snapshot's linkage + cut at the distance threshold, on the re-scored neighbour graph; "
                            "implies --rescore).")
        p.add_argument("--exact", action="store_true",
                       help="Exact mode: the matched-peak cosine of every pair inside each precursor bucket, then the "
                            "snapshot's hierarchical clustering (--linkage) on those distances; no vectors, index or "
                            "nearest-neighbour search.  Implies --clustering hierarchical.")
        p.add_argument("--distance_threshold", type=float, default=0.1,
                       help="Cosine distance threshold; alias of --eps (default: 0.1).")
        p.add_argument("--eps", type=float, default=None,
                       help="DBSCAN eps = cosine distance threshold (README); alias of --distance_threshold.")
        p.add_argument("--min_matched_peaks", type=int, default=0,
                       help="(snapshot option, accepted; unused by the nearest-neighbour path)")
        p.add_argument("--batch_size", type=int, default=2 ** 15, help="Maximum precursor-m/z block size.")
        # NEAREST NEIGHBOUR INDEXING  (README.md:101-117)
        p.add_argument("--n_probe", type=int, default=16, help="Maximum number of inverted lists to inspect.")
        p.add_argument("--n_neighbors", type=int, default=64, help="Final number of neighbours per spectrum.")
        p.add_argument("--n_neighbors_ann", type=int, default=128, help="Neighbours retrieved by the ANN search.")
        p.add_argument("--low_dim", type=int, default=400,
                       help="Low-dimensional vector length (README.md:114-117): any integer in [1, 800]. The vectors are "
                            "stored in rows of the next instantiated width (64 / 128 / 256 / 400 / 800), zero behind low_dim.")
        p.add_argument("--dtype", type=str, default="f32", choices=["f32", "f16"],
                       help="Element type of the hashed vectors: f32 (default) or f16 (half the bytes per vector; the "
                            "similarity of two float16 vectors is the float32 chain over their exact float32 images).")
        p.add_argument("--mz_interval", type=float, default=1.0,
                       help="Width in m/z of the precursor windows that bound an index (0 = off).")
        p.add_argument("--rescore", action="store_true",
                       help="Re-score the nearest neighbours with the matched-peak cosine (fragment_tol, "
                            "min_matched_peaks) before clustering.")
        p.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
        p.add_argument("--mgf_reader", type=str, default="device", choices=["device", "host"],
                       help="MGF input, --library and --assign_to files: parse the text on the GPU (device), or with the host "
                            "readers; the outputs are the same.")
        p.add_argument("--mzml_reader", type=str, default="host", choices=["device", "host"],
                       help="mzML input: scan the XML structure on the GPU (device), or with the host reader (the default until "
                            "tools/mzml_rate.py has shown the device reader faster); the outputs are the same.")
        p.add_argument("--msp_reader", type=str, default="device", choices=["device", "host"],
                       help="--library files named .msp (NIST / MoNA / MassBank style MSP libraries): parse the text on the GPU "
                            "(device), or with the host reader; the outputs are the same.")
        p.add_argument("--mgf_writer", type=str, default="device", choices=["device", "host"],
                       help="--export_representatives: format the MGF text on the GPU (device), or with the host writer; the "
                            "file is the same byte for byte.")
        p.add_argument("--csv_writer", type=str, default="device", choices=["device", "host"],
                       help="Sort the rows of the cluster CSV and format their text on the GPU (device), or with the host "
                            "writer; the file is the same byte for byte.")
        p.add_argument("--graphml_writer", type=str, default="device", choices=["device", "host"],
                       help="--network_graphml: format the node and edge text on the GPU (device), or with the host writer; the "
                            "file is the same byte for byte.")
        p.add_argument("--distributed", action="store_true",
                       help="Run as one rank of a multi-GPU job launched by `python -m torch.distributed.run --module "
                            "falcon_amd.falcon ...`: the precursor windows / buckets of every charge are dealt to the ranks, "
                            "rank 0 writes the outputs.")
        # PREPROCESSING  (config.py:126-183)
        p.add_argument("--min_peaks", default=5, type=int)
        p.add_argument("--min_mz_range", default=250.0, type=float)
        p.add_argument("--min_mz", default=101.0, type=float)
        p.add_argument("--max_mz", default=1500.0, type=float)
        p.add_argument("--remove_precursor_tol", default=1.5, type=float)
        p.add_argument("--min_intensity", default=0.01, type=float)
        p.add_argument("--max_peaks_used", default=50, type=int)
        p.add_argument("--scaling", default="off", type=str, choices=["off", "root", "log", "rank"])
        self._parser = p
        self._base_defaults = {a.dest: a.default for a in p._actions if a.dest != "help"}
        self._namespace = None

    # ------------------------------------------------------------------------------------------
    def _ini_defaults(self, path: Optional[str]) -> dict:
        if path is None:
            path = "config.ini" if os.path.isfile("config.ini") else None      # config.py:46
        if path is None:
            return {}
        if not os.path.isfile(path):
            raise FileNotFoundError(f"config file {path} not found")
        with open(path) as f:
            text = f.read()
        cp = configparser.ConfigParser()
        cp.optionxform = str
        try:
            cp.read_string(text)
        except configparser.MissingSectionHeaderError:
            cp.read_string("[falcon]\n" + text)                               # configargparse: no sections
        out = {}
        known = {a.dest: a for a in self._parser._actions}
        for sec in cp.sections():
            for k, v in cp[sec].items():
                k = k.strip().lstrip("-")
                if k not in known:
                    raise ValueError(f"unknown option {k!r} in {path}")
                a = known[k]
                if isinstance(a, argparse._StoreTrueAction):
                    out[k] = v.strip().lower() in ("1", "true", "yes", "on")
                elif a.nargs in (2, "+"):
                    out[k] = shlex.split(v.strip("[] ").replace(",", " "))
                elif a.type is not None:
                    out[k] = a.type(v)
                else:
                    out[k] = v
        return out

    def parse(self, args_str: Union[str, List[str], None] = None) -> None:
        """config.py:187-201: None -> sys.argv; a string is split shell-style."""
        if isinstance(args_str, str):
            args_str = shlex.split(args_str)
        pre = argparse.ArgumentParser(add_help=False)
        pre.add_argument("-c", "--config", default=None)
        known, _ = pre.parse_known_args(args_str)
        defaults = self._ini_defaults(known.config)
        # INI values are defaults of THIS call only: start from the built-in defaults every time (a parser keeps
        # what set_defaults gave it, and main() / parse() are called repeatedly in one process)
        self._parser.set_defaults(**self._base_defaults)
        if defaults:
            self._parser.set_defaults(**defaults)
        ns = vars(self._parser.parse_args(args_str))
        ns["precursor_tol"] = [float(ns["precursor_tol"][0]), str(ns["precursor_tol"][1])]   # config.py:199-201
        if ns["precursor_tol"][1] not in ("ppm", "Da"):
            raise ValueError('precursor_tol mode must be "ppm" or "Da"')
        if ns["eps"] is None:
            ns["eps"] = ns["distance_threshold"]
        else:
            ns["distance_threshold"] = ns["eps"]
        # the reference's --linkage values keep their meaning: a non-default linkage selects the hierarchical clustering;
        # with an explicit --clustering dbscan (which has no linkage) the command line fails here, not per charge later
        if ns["exact"]:
            if ns["clustering"] == "dbscan":
                self._parser.error("--exact clusters the all-pairs distances hierarchically: it does not combine with "
                                   "--clustering dbscan")
            ns["clustering"] = "hierarchical"
        if ns["clustering"] is None:
            ns["clustering"] = "hierarchical" if ns["linkage"] != "complete" else "dbscan"
        elif ns["clustering"] == "dbscan" and ns["linkage"] != "complete":
            self._parser.error(f"--linkage {ns['linkage']} needs --clustering hierarchical (DBSCAN has no linkage)")
        if ns["clustering"] == "hierarchical":
            ns["rescore"] = True
        if not 0.0 < ns["consensus_min_fraction"] <= 1.0:
            self._parser.error(f"--consensus_min_fraction {ns['consensus_min_fraction']} is outside (0, 1]")
        if ns["representatives"] not in ("medoid", "consensus"):          # (a config file's value: choices guard the command line)
            self._parser.error(f"--representatives {ns['representatives']}: medoid or consensus")
        if ns["mgf_reader"] not in ("device", "host"):
            self._parser.error(f"--mgf_reader {ns['mgf_reader']}: device or host")
        if ns["mzml_reader"] not in ("device", "host"):
            self._parser.error(f"--mzml_reader {ns['mzml_reader']}: device or host")
        if ns["msp_reader"] not in ("device", "host"):
            self._parser.error(f"--msp_reader {ns['msp_reader']}: device or host")
        if ns["mgf_writer"] not in ("device", "host"):
            self._parser.error(f"--mgf_writer {ns['mgf_writer']}: device or host")
        if ns["csv_writer"] not in ("device", "host"):
            self._parser.error(f"--csv_writer {ns['csv_writer']}: device or host")
        if ns["representatives"] == "consensus" and not ns["export_representatives"]:
            self._parser.error("--representatives consensus needs --export_representatives (there is no other output it changes)")
        if ns["assign_to"] is not None and isinstance(ns["assign_to"], str):
            ns["assign_to"] = [ns["assign_to"]]
        if ns["assign_to"] and ns["distributed"]:
            self._parser.error("--assign_to does not combine with --distributed (the assignment to representatives is not sharded)")
        if ns["cluster_summary"] and ns["assign_to"]:
            self._parser.error("--cluster_summary does not combine with --assign_to (the cluster-mates of an assigned spectrum "
                               "are not in the run)")
        if ns["cluster_summary"] and ns["distributed"]:
            self._parser.error("--cluster_summary does not combine with --distributed (the summary is not sharded)")
        if not 0.0 <= ns["network_min_cosine"] <= 1.0:
            self._parser.error(f"--network_min_cosine {ns['network_min_cosine']} is outside [0, 1]")
        if ns["network_min_matched_peaks"] < 0:
            self._parser.error(f"--network_min_matched_peaks {ns['network_min_matched_peaks']} is negative")
        if ns["network_top_k"] < 0:
            self._parser.error(f"--network_top_k {ns['network_top_k']} is negative")
        if not ns["network_max_shift"] >= 0.0:
            self._parser.error(f"--network_max_shift {ns['network_max_shift']} is negative")
        if ns["network"] and ns["assign_to"]:
            self._parser.error("--network does not combine with --assign_to (the representatives of the existing clusters are "
                               "not in the run)")
        if ns["network"] and ns["distributed"]:
            self._parser.error("--network does not combine with --distributed (the network is not sharded)")
        if ns["network_families"] and not ns["network"]:
            self._parser.error("--network_families needs --network (the families are the components of its links)")
        if ns["network_graphml"] and not ns["network"]:
            self._parser.error("--network_graphml needs --network (it is the network's links and clusters in one file)")
        if ns["graphml_writer"] not in ("device", "host"):
            self._parser.error(f"--graphml_writer {ns['graphml_writer']}: device or host")
        if ns["network_max_family_size"] < 0:
            self._parser.error(f"--network_max_family_size {ns['network_max_family_size']} is negative")
        if not ns["network_family_delta"] >= 0.0:
            self._parser.error(f"--network_family_delta {ns['network_family_delta']} is negative")
        if ns["library"] is not None and isinstance(ns["library"], str):
            ns["library"] = [ns["library"]]
        if not 0.0 <= ns["library_min_cosine"] <= 1.0:
            self._parser.error(f"--library_min_cosine {ns['library_min_cosine']} is outside [0, 1]")
        if ns["library_min_matched_peaks"] < 0:
            self._parser.error(f"--library_min_matched_peaks {ns['library_min_matched_peaks']} is negative")
        if ns["library_top_n"] < 0:
            self._parser.error(f"--library_top_n {ns['library_top_n']} is negative")
        if not ns["library_max_shift"] >= 0.0:
            self._parser.error(f"--library_max_shift {ns['library_max_shift']} is negative")
        if ns["library"] and ns["assign_to"]:
            self._parser.error("--library does not combine with --assign_to (the representatives of the existing clusters are "
                               "not in the run)")
        if ns["library"] and ns["distributed"]:
            self._parser.error("--library does not combine with --distributed (the library search is not sharded)")
        if ns["library_analog"] and not ns["library"]:
            self._parser.error("--library_analog needs --library (it is a mode of the library search)")
        if ns["library_propagate"] and not ns["library"]:
            self._parser.error("--library_propagate needs --library (it carries the library's hits on)")
        if ns["library_propagate"] and not (ns["network"] and ns["network_families"]):
            self._parser.error("--library_propagate needs --network --network_families (it walks the families' links)")
        if not 1 <= ns["library_propagate_hops"] <= 64:
            self._parser.error(f"--library_propagate_hops {ns['library_propagate_hops']} is outside [1, 64]")
        if not 0.0 <= ns["library_propagate_min_score"] <= 1.0:
            self._parser.error(f"--library_propagate_min_score {ns['library_propagate_min_score']} is outside [0, 1]")
        if not 1 <= ns["low_dim"] <= 800:
            raise ValueError("low_dim must be an integer in [1, 800] (README.md:114-117; the widest rows the kernels hold)")
        if ns["n_neighbors_ann"] < ns["n_neighbors"]:
            raise ValueError("n_neighbors_ann should be equal or greater than n_neighbors (README.md:110-113)")
        self._namespace = ns

    def __getattr__(self, option):
        if option.startswith("_"):
            raise AttributeError(option)
        if self._namespace is None:
            raise RuntimeError("The configuration has not been initialized")     # config.py:203-206
        return self._namespace[option]

    def __setattr__(self, key, value):
        if key.startswith("_"):
            object.__setattr__(self, key, value)
        else:
            if self._namespace is None:
                raise RuntimeError("The configuration has not been initialized")
            self._namespace[key] = value

    def __getitem__(self, item):
        return self.__getattr__(item)


config = Config()
