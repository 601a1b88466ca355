"""The GraphML writer without a GPU: the host writer of record (`graphml_io.write_graphml`) against XML parsers, the pure functions
of the device's record writer (`csrc/recwrite.h`, built for the host) against the host writer unit for unit, and the command
line's errors."""
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from falcon_amd.ms_io import graphml_io as G
from tests import graphml_cases as K
from tests import hostbuild_records as H

NS = "{http://graphml.graphdrawing.org/xmlns}"
CASES = [(name, n) for name in K.DEVICE_SETS for n in K.SIZES]
HOST_ONLY = sorted(K.host_only_strings())
_TYPES = {"long": int, "int": int, "double": float, "string": str}


def _blocks(name, n):
    return K.DEVICE_SETS[name](n)


def _fffd(s: str) -> str:
    return G._FORBIDDEN.sub("\ufffd", s)


def parse(raw: bytes):
    """ElementTree's reading of the file -> ({node id: attributes}, [((source, target), attributes)], key table, options)"""
    root = ET.fromstring(raw)
    keys = {k.get("id"): (k.get("for"), k.get("attr.name"), _TYPES[k.get("attr.type")]) for k in root.findall(NS + "key")}
    graph = root.find(NS + "graph")
    assert graph.get("edgedefault") == "undirected"
    read = lambda el, kind: {keys[d.get("key")][1]: keys[d.get("key")][2](d.text or "") for d in el.findall(NS + "data")
                             if keys[d.get("key")][0] == kind}
    nodes = {el.get("id"): read(el, "node") for el in graph.findall(NS + "node")}
    edges = [((el.get("source"), el.get("target")), read(el, "edge")) for el in graph.findall(NS + "edge")]
    options = [d.text for d in graph.findall(NS + "data")]
    return nodes, edges, keys, options


@pytest.mark.parametrize("name,n", CASES)
def test_host_writer_parses_with_elementtree(name, n):
    blocks = _blocks(name, n)
    raw = K.host_bytes(blocks)
    assert raw.startswith(b'<?xml version="1.0" encoding="UTF-8"?>\n<graphml xmlns="http://graphml.graphdrawing.org/xmlns">\n<key id="v_cluster"')
    assert raw.endswith(b"</graph>\n</graphml>\n") and b"\r" not in raw
    nodes, edges, keys, options = parse(raw)
    want_nodes, want_edges = K.expected_graph(blocks)
    assert nodes == want_nodes and len(nodes) == n
    assert len(edges) == n and dict(edges) == want_edges
    assert [e[0] for e in edges] == [(str(int(b["first"]) + int(x)), str(int(b["first"]) + int(y))) for b in blocks
                                     for x, y in zip(b["network"]["a"], b["network"]["b"])]
    node_keys, edge_keys = G.keys(K.SWITCHES)
    assert [k for k in keys] == [f"v_{k}" for k, _ in node_keys] + [f"e_{k}" for k, _ in edge_keys] + ["g_options"]
    assert options == ["\n".join(K.HEADER)]


@pytest.mark.parametrize("kind", HOST_ONLY)
def test_host_writer_writes_fffd_for_what_xml_forbids(kind):
    blocks = K.host_only(kind)
    raw = K.host_bytes(blocks)
    assert "\ufffd".encode() in raw and b"\x01" not in raw
    nodes, edges, _, _ = parse(raw)
    want_nodes, want_edges = K.expected_graph(blocks, readable=_fffd)
    assert nodes == want_nodes and dict(edges) == want_edges
    assert G.tables(blocks, None, *K.SWITCHES)[0] is None and "forbids" in G.tables(blocks, None, *K.SWITCHES)[1]


def test_keys_follow_the_switches():
    blocks = K.plain(5)
    for b in blocks:
        b["library"] = b["annotations"] = None
        b["network"] = {k: v for k, v in b["network"].items() if k not in ("family", "node_family", "node_size", "n_families")}
    import io
    f = io.StringIO()
    G.write_graphml(f, [], blocks)
    nodes, edges, keys, options = parse(f.getvalue().encode())
    assert list(keys) == ["v_cluster", "v_precursor_charge", "v_precursor_mz", "v_retention_time", "v_size", "e_delta_mz", "e_cosine",
                          "e_matched_peaks", "g_options"]
    assert options == [] and len(nodes) == 5 and all(set(d) == {"delta_mz", "cosine", "matched_peaks"} for _, d in edges)


@pytest.mark.parametrize("name,n", [(name, n) for name in K.DEVICE_SETS for n in (65, 257)])
def test_networkx_reads_back_what_went_in(name, n, tmp_path):
    nx = pytest.importorskip("networkx")
    blocks = _blocks(name, n)
    path = tmp_path / "g.graphml"
    path.write_bytes(K.host_bytes(blocks))
    g = nx.read_graphml(path)
    want_nodes, want_edges = K.expected_graph(blocks)
    assert not g.is_directed() and set(g.nodes) == set(want_nodes) and g.number_of_edges() == len(want_edges) == n
    for node, want in want_nodes.items():
        assert dict(g.nodes[node]) == want, node
    for (a, b), want in want_edges.items():
        assert dict(g.edges[a, b]) == want, (a, b)
    assert g.graph["options"] == "\n".join(K.HEADER)


# ---- the record writer's pure functions, built for the host ----------------------------------------------------------------------------
needs_compiler = pytest.mark.skipif(not H.have_compiler(), reason="no host C++ compiler and no hipcc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("records_shim"))


@needs_compiler
def test_limits_and_field_layout(lib):
    import ctypes as C
    from falcon_amd import _lib
    assert lib.t_field_bytes() == C.sizeof(_lib.RecField) == 64
    assert [lib.t_limits(i) for i in range(4)] == [_lib.REC_MAX_FIELDS, _lib.REC_MAX_LITERALS, 20, 5]


@needs_compiler
@pytest.mark.parametrize("name,n", CASES)
def test_host_build_gives_the_host_writers_units(lib, name, n):
    blocks = _blocks(name, n)
    tables, why = G.tables(blocks, None, *K.SWITCHES)
    assert why is None
    for table, want in zip(tables, K.host_units(blocks)):
        assert table["n"] == len(want) == n and len(table["fields"]) <= 32
        got, lens, bad, intact = H.units(lib, table)
        assert intact and not bad.any()
        assert lens.tolist() == [len(w) for w in want]
        for u in range(n):
            assert got[u] == want[u], (u, got[u][:200], want[u][:200])


@needs_compiler
def test_character_data_and_its_grammar(lib):
    for s in K.text_strings() + K.plain_strings():
        raw = s.encode("utf-8")
        got, only, bad = H.xml(lib, raw)
        assert got == G.xml_text(s).encode("utf-8") and only == len(got) and not bad
    for c in range(0x20):
        got, only, bad = H.xml(lib, b"a" + bytes([c]) + b"b")
        assert bad == (c not in (9, 10, 13)), c
    assert H.xml(lib, bytes(range(0x20, 0x100)))[2] is False


@needs_compiler
def test_bad_rows_are_flagged_and_read_nothing(lib):
    """an index at or beyond the column, a text row that does not ascend inside its blob, a byte outside the grammar: the unit
    is flagged, the field counts as absent"""
    ptr = np.array([0, 3, 6], np.int64)
    good = dict(n=2, head=b"<", tail=b">\n", fields=[dict(kind="text", column=np.frombuffer(b"abcdef", np.uint8), ptr=ptr, index=None,
                                                             prefix=b"[", suffix=b"]")])
    assert H.units(lib, good)[0] == [b"<[abc]>\n", b"<[def]>\n"]
    for change in (dict(ptr=np.array([0, 7, 6], np.int64)), dict(ptr=np.array([-1, 3, 6], np.int64)), dict(ptr=np.array([0, 3, 2], np.int64)),
                   dict(index=np.array([0, 2], np.int32)), dict(column=np.frombuffer(b"abc\x00ef", np.uint8))):
        table = dict(good, fields=[dict(good["fields"][0], **change)])
        got, lens, bad, intact = H.units(lib, table)
        assert bad.any() and intact and all(g in (b"<[abc]>\n", b"<[def]>\n", b"<>\n") for g in got), change
    table = dict(good, fields=[dict(good["fields"][0], index=np.array([-1, 0], np.int32))])
    assert H.units(lib, table)[0] == [b"<>\n", b"<[abc]>\n"] and not H.units(lib, table)[2].any()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,message", [
    (["--network_graphml"], "--network_graphml needs --network"),
    (["--network", "--network_graphml", "--assign_to", "reps.mgf"], "--network does not combine with --assign_to"),
    (["--network", "--network_graphml", "--distributed"], "--network does not combine with --distributed"),
    (["--network", "--network_graphml", "--graphml_writer", "gpu"], "--graphml_writer"),
])
def test_parser_errors(args, message, capsys):
    from falcon_amd.config import config
    with pytest.raises(SystemExit):
        config.parse(["in.mgf", "out", *args])
    assert message in capsys.readouterr().err
    config.parse(["in.mgf", "out", "--network", "--network_graphml"])
    assert config.network_graphml and config.graphml_writer in ("device", "host")
