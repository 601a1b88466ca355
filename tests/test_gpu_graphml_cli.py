"""`--network_graphml` through `main()`: the chains and the GNPS-style library of tests/test_gpu_propagate.py with every network
option on.  `<out>.network.graphml` is the host writer's file byte for byte, its nodes and edges carry the cells of the run's
CSVs, and no other output changes."""
import csv
import logging
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from tests.test_gpu_propagate import LIBRARY_ARGS, NETWORK_ARGS, PROPAGATE_ARGS, _write_chains_and_library
from tests.test_graphml_cpu import parse

pytestmark = pytest.mark.gpu
OTHERS = (".csv", ".mgf", ".network.csv", ".families.csv", ".library.csv", ".annotations.csv")


def _table(path):
    return list(csv.DictReader(l for l in open(path, newline="").read().split("\n") if l and not l.startswith("#")))


def _f(text):
    return float(str(np.float32(text)))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the same input with the flag (device and host writer) and without it, one work directory: the headers name it"""
    from falcon_amd.falcon import main
    tmp = tmp_path_factory.mktemp("graphml_cli")
    mgf, lib_mgf, work = str(tmp / "in.mgf"), str(tmp / "gnps_like.mgf"), str(tmp / "work")
    _write_chains_and_library(mgf, lib_mgf)
    common = ["--eps", "0.3", "--export_representatives", "--work_dir", work] + NETWORK_ARGS + ["--library", lib_mgf] + LIBRARY_ARGS + \
        PROPAGATE_ARGS
    out = {k: str(tmp / k) for k in ("without", "device", "host")}
    assert main([mgf, out["without"]] + common) == 0
    assert main([mgf, out["device"]] + common + ["--network_graphml", "--graphml_writer", "device"]) == 0
    assert main([mgf, out["host"]] + common + ["--network_graphml", "--graphml_writer", "host"]) == 0
    return dict(out, mgf=mgf, lib_mgf=lib_mgf, work=work, common=common, tmp=tmp)


def test_the_device_file_is_the_host_writers_and_nothing_else_changes(runs):
    assert not os.path.exists(runs["without"] + ".network.graphml")
    dev, host = (open(runs[k] + ".network.graphml", "rb").read() for k in ("device", "host"))
    assert dev == host and dev.count(b"<node ") > 20 and dev.count(b"<edge ") > 5
    for ext in OTHERS:
        want = open(runs["without"] + ext, "rb").read()
        for k in ("device", "host"):
            assert open(runs[k] + ext, "rb").read() == want, (k, ext)
        assert b"network_graphml" not in want and b"graphml_writer" not in want          # (no header line of any other file)


def test_nodes_and_edges_carry_the_cells_of_the_other_files(runs):
    out = runs["device"]
    nodes, edges, keys, options = parse(open(out + ".network.graphml", "rb").read())
    rows, links, fams = _table(out + ".csv"), _table(out + ".network.csv"), _table(out + ".families.csv")
    hits, anns = [r for r in _table(out + ".library.csv") if r["rank"] == "1"], _table(out + ".annotations.csv")
    clusters = sorted({int(r["cluster"]) for r in rows})
    assert list(nodes) == [str(c) for c in clusters]                               # every cluster, in id order
    # the representative's precursor and retention time: the exported MGF's entries
    reps = {}
    for entry in open(out + ".mgf").read().split("BEGIN IONS")[1:]:
        fields = dict(l.split("=", 1) for l in entry.splitlines() if "=" in l and not l[0].isdigit())
        reps[int(fields["CLUSTER"])] = (np.float32(fields["PEPMASS"]), np.float32(fields["RTINSECONDS"]))
    fam_of, hit_of, ann_of = ({int(r["cluster"]): r for r in t} for t in (fams, hits, anns))
    name_of = {r["cluster"]: r["name"] for r in hits}
    assert 0 < len(hit_of) < len(ann_of) < len(clusters)              # clusters with a hit, reached from one, and left without a name
    for c in clusters:
        mine = [r for r in rows if int(r["cluster"]) == c]
        want = dict(cluster=c, precursor_charge=mine[0]["precursor_charge"], size=len(mine), precursor_mz=_f(reps[c][0]),
                    retention_time=_f(reps[c][1]), family_size=int(fam_of[c]["family_size"]))
        if int(fam_of[c]["family"]) >= 0:
            want["family"] = int(fam_of[c]["family"])
        if c in hit_of:
            h = hit_of[c]
            want.update({k: h[k] for k in ("library_id", "name", "adduct", "smiles", "inchikey") if h[k] != ""},
                        library_cosine=_f(h["cosine"]), library_delta_mz=_f(h["delta_mz"]), library_matched_peaks=int(h["matched_peaks"]))
        if c in ann_of:
            a = ann_of[c]
            want.update(annotation_hops=int(a["hops"]), annotation_source=int(a["source_cluster"]), annotation_score=_f(a["path_score"]),
                        annotation_name=name_of[a["source_cluster"]])
        assert nodes[str(c)] == want, c
    assert [e[0] for e in edges] == [(r["cluster_a"], r["cluster_b"]) for r in links]          # the rows of the network file, in order
    for (_, got), r in zip(edges, links):
        assert got == dict(delta_mz=_f(r["delta_mz"]), cosine=_f(r["cosine"]), matched_peaks=int(r["matched_peaks"]), family=int(r["family"]))
    header = [l[2:] for l in open(out + ".annotations.csv", newline="").read().split("\n") if l.startswith("# ")]
    assert options == ["\n".join(header)]


def test_the_network_alone_has_only_its_own_keys(runs):
    from falcon_amd.falcon import main
    out = str(runs["tmp"] / "alone")
    args = [runs["mgf"], out, "--eps", "0.3", "--work_dir", runs["work"], "--network", "--network_min_cosine", "0.5",
            "--network_min_matched_peaks", "4", "--network_graphml"]
    assert main(args) == 0
    nodes, edges, keys, _ = parse(open(out + ".network.graphml", "rb").read())
    assert list(keys) == ["v_cluster", "v_precursor_charge", "v_precursor_mz", "v_retention_time", "v_size", "e_delta_mz", "e_cosine",
                          "e_matched_peaks", "g_options"]
    assert len(edges) == len(_table(out + ".network.csv")) > 0 and all(len(d) == 5 for d in nodes.values())
    assert main(args) == 1                                                         # the files are there: refused without --overwrite
    os.remove(out + ".csv"), os.remove(out + ".network.csv")
    assert main(args) == 1                                                         # the GraphML file alone refuses too


def test_a_forbidden_character_in_a_library_name_goes_to_the_host_writer(runs, caplog):
    from falcon_amd.falcon import main
    lib = str(runs["tmp"] / "odd_library.mgf")
    text = open(runs["lib_mgf"]).read()
    assert "NAME=Compound 0," in text
    open(lib, "w").write(text.replace("NAME=Compound 0,", "NAME=Compound\x01 0,"))
    out = str(runs["tmp"] / "odd")
    common = [c if c != runs["lib_mgf"] else lib for c in runs["common"]]
    with caplog.at_level(logging.DEBUG, logger="falcon"):
        assert main([runs["mgf"], out] + common + ["--network_graphml", "--graphml_writer", "device"]) == 0
    said = [r.getMessage() for r in caplog.records if "the host writer writes" in r.getMessage() and "graphml" in r.getMessage()]
    assert len(said) == 1 and "name" in said[0] and "forbids" in said[0]
    raw = open(out + ".network.graphml", "rb").read()
    ET.fromstring(raw)
    assert "Compound\ufffd 0,".encode() in raw and b"\x01" not in raw
