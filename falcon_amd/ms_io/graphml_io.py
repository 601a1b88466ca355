"""`--network_graphml`: the network as one GraphML file beside the CSVs (DESIGN.md "GraphML out of the device").

`<output>.network.graphml`: one `<node>` per cluster of every charge, in cluster-id order, clusters without a link included, and
one `<edge>` per row of `<output>.network.csv` in that file's order, each with the attributes the run's other files hold for it.
UTF-8, `\\n` line ends, every `<key>`, `<node>` and `<edge>` on a line of its own:

    <?xml version="1.0" encoding="UTF-8"?>
    <graphml xmlns="http://graphml.graphdrawing.org/xmlns">
    <key id="v_cluster" for="node" attr.name="cluster" attr.type="long"/>      (the node keys, then the edge keys, in use)
    <key id="g_options" for="graph" attr.name="options" attr.type="string"/>
    <graph id="network" edgedefault="undirected">
    <data key="g_options">...the `#` header lines of the run's files, joined by "\\n"...</data>
    <node id="17"><data key="v_cluster">17</data>...</node>
    <edge source="17" target="42"><data key="e_delta_mz">14.016</data>...</edge>
    </graph>
    </graphml>

A `<data>` element is left out whole when its value does not exist (no family, no hit, no annotation), when its float is not
finite or when its text is empty.  Integers are decimal, float32 values `str(np.float32(x))` as in the CSVs.  In text `&`, `<`,
`>` become `&amp;`, `&lt;`, `&gt;` and `\\r` becomes `&#13;`; a character XML 1.0 forbids (a control character other than tab,
line feed and carriage return, U+FFFE, U+FFFF, a lone surrogate) is written as U+FFFD.

A block is one charge partition: dict(charge (the CSV's text: "2", "None"), first (the global id of the charge's cluster 0),
precursor_mz, retention_time f32[n] (the representatives'), size i32[n] (member spectra), network (the charge's block of
`network_io`), library (that of `library_io`, or None) and annotations (that of `annotation_io`, or None)).  Blocks are given in
the order of their cluster ids.

`write_graphml` is the writer of record, plain Python per element.  `write` sends the nodes and the edges through the device's
record writer (`Context.format_records`: `tables` describes both as records of fields) and writes the few hundred bytes around
them itself; the host writer takes the whole file where a string is outside what the device mirrors (`tables` says why)."""
import logging
import re

import numpy as np

logger = logging.getLogger("falcon")

NODE_KEYS = [("cluster", "long"), ("precursor_charge", "string"), ("precursor_mz", "double"), ("retention_time", "double"),
             ("size", "int")]
FAMILY_NODE_KEYS = [("family", "long"), ("family_size", "int")]
LIBRARY_TEXT = ["library_id", "name", "adduct", "smiles", "inchikey"]
LIBRARY_NODE_KEYS = [(k, "string") for k in LIBRARY_TEXT] + [("library_cosine", "double"), ("library_delta_mz", "double"),
                                                             ("library_matched_peaks", "int")]
PROPAGATE_NODE_KEYS = [("annotation_hops", "int"), ("annotation_source", "long"), ("annotation_score", "double"),
                       ("annotation_name", "string")]
EDGE_KEYS = [("delta_mz", "double"), ("cosine", "double"), ("matched_peaks", "int")]
FAMILY_EDGE_KEYS = [("family", "long")]

_FORBIDDEN = re.compile("[\x00-\x08\x0b\x0c\x0e-\x1f\ufffe\uffff\ud800-\udfff]")


def switches(blocks, families=None, library=None, propagate=None):
    """which attribute groups the file carries: as given, else what the blocks hold -> (families, library, propagate)"""
    if families is None:
        families = any("node_family" in b["network"] for b in blocks)
    if library is None:
        library = any(b.get("library") is not None for b in blocks)
    if propagate is None:
        propagate = any(b.get("annotations") is not None for b in blocks)
    return bool(families), bool(library), bool(propagate)


def keys(sw):
    """-> (node keys, edge keys) as (name, GraphML type), in the file's order"""
    families, library, propagate = sw
    node = NODE_KEYS + (FAMILY_NODE_KEYS if families else []) + (LIBRARY_NODE_KEYS if library else []) + \
        (PROPAGATE_NODE_KEYS if propagate else [])
    return node, EDGE_KEYS + (FAMILY_EDGE_KEYS if families else [])


def xml_text(s) -> str:
    """character data: forbidden characters as U+FFFD, the three markup characters and the carriage return as entities"""
    s = _FORBIDDEN.sub("\ufffd", str(s))
    return s.replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;").replace("\r", "&#13;")


def prologue(header, sw) -> str:
    node, edge = keys(sw)
    lines = ['<?xml version="1.0" encoding="UTF-8"?>', '<graphml xmlns="http://graphml.graphdrawing.org/xmlns">']
    lines += [f'<key id="v_{k}" for="node" attr.name="{k}" attr.type="{t}"/>' for k, t in node]
    lines += [f'<key id="e_{k}" for="edge" attr.name="{k}" attr.type="{t}"/>' for k, t in edge]
    lines += ['<key id="g_options" for="graph" attr.name="options" attr.type="string"/>', '<graph id="network" edgedefault="undirected">']
    options = xml_text("\n".join(header))
    if options:
        lines.append(f'<data key="g_options">{options}</data>')
    return "\n".join(lines) + "\n"


EPILOGUE = "</graph>\n</graphml>\n"


def _data(key: str, text: str) -> str:
    return f'<data key="{key}">{text}</data>' if text != "" else ""


def _f32(key: str, x) -> str:
    x = np.float32(x)
    return _data(key, str(x)) if np.isfinite(x) else ""


def _family_bases(blocks):
    bases, base = [], 0
    for b in blocks:
        bases.append(base)
        base += int(b["network"].get("n_families", 0))
    return bases


def node_units(blocks, sw):
    """the `<node>` lines, one str per cluster"""
    families, library, propagate = sw
    for b, base in zip(blocks, _family_bases(blocks)):
        first, net, lib, ann = int(b["first"]), b["network"], b.get("library"), b.get("annotations")
        hit_of, ann_of = {}, {}
        if library and lib is not None:
            for e in range(len(lib["cluster"])):
                hit_of.setdefault(int(lib["cluster"][e]), e)                    # (cluster, rank) order: the first is rank 1
        if propagate and ann is not None:
            for e in range(len(ann["cluster"])):
                ann_of[int(ann["cluster"][e])] = e
        for c in range(len(b["size"])):
            cid = first + c
            out = [f'<node id="{cid}">', _data("v_cluster", str(cid)), _data("v_precursor_charge", xml_text(b["charge"])),
                   _f32("v_precursor_mz", b["precursor_mz"][c]), _f32("v_retention_time", b["retention_time"][c]),
                   _data("v_size", str(int(b["size"][c])))]
            if families:
                fam = int(net["node_family"][c])
                out += [_data("v_family", str(base + fam)) if fam >= 0 else "", _data("v_family_size", str(int(net["node_size"][c])))]
            if library and c in hit_of:
                e = hit_of[c]
                r = int(lib["library"][e])
                out += [_data(f"v_{k}", xml_text(lib[k][r])) for k in LIBRARY_TEXT]
                out += [_f32("v_library_cosine", lib["similarity"][e]), _f32("v_library_delta_mz", lib["delta_mz"][e]),
                        _data("v_library_matched_peaks", str(int(lib["matched"][e])))]
            if propagate and c in ann_of:
                e = ann_of[c]
                out += [_data("v_annotation_hops", str(int(ann["hops"][e]))), _data("v_annotation_source", str(first + int(ann["source"][e]))),
                        _f32("v_annotation_score", ann["score"][e]), _data("v_annotation_name", xml_text(ann["name"][int(ann["library"][e])]))]
            yield "".join(out) + "</node>\n"


def edge_units(blocks, sw):
    """the `<edge>` lines, one str per link"""
    families = sw[0]
    for b, base in zip(blocks, _family_bases(blocks)):
        first, net = int(b["first"]), b["network"]
        for e in range(len(net["a"])):
            out = [f'<edge source="{first + int(net["a"][e])}" target="{first + int(net["b"][e])}">', _f32("e_delta_mz", net["delta_mz"][e]),
                   _f32("e_cosine", net["similarity"][e]), _data("e_matched_peaks", str(int(net["matched"][e])))]
            if families:
                out.append(_data("e_family", str(base + int(net["family"][e]))))
            yield "".join(out) + "</edge>\n"


def write_graphml(f, header, blocks, families=None, library=None, propagate=None) -> None:
    """the file into the text file `f` (UTF-8, newline "\\n"); the three switches: `switches`"""
    sw = switches(blocks, families, library, propagate)
    f.write(prologue(header, sw))
    for unit in node_units(blocks, sw):
        f.write(unit)
    for unit in edge_units(blocks, sw):
        f.write(unit)
    f.write(EPILOGUE)


# ---- the device path ------------------------------------------------------------------------------------------------------------------
def text_blob(strings):
    """str array -> ((u8 blob of the strings' UTF-8 bytes back to back, i64 offsets[n + 1]), None), or (None, why the device
    writer does not mirror the host's text for them)"""
    items = np.asarray(strings, dtype=str).tolist() if len(strings) else []
    joined = "".join(items)
    if _FORBIDDEN.search(joined):
        return None, "holds a character XML 1.0 forbids or one that cannot be encoded (the host writer writes U+FFFD)"
    raw = joined.encode("utf-8")                     # (no lone surrogate is left: every str encodes)
    if len(raw) == len(joined):
        lens = np.fromiter(map(len, items), np.int64, len(items))
    else:
        lens = np.fromiter((len(s.encode("utf-8")) for s in items), np.int64, len(items))
    ptr = np.zeros(len(items) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    return (np.frombuffer(raw, np.uint8), ptr), None


def _host(a):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def _cat(parts, dtype):
    parts = [np.asarray(p, dtype) for p in parts]
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def _first_rows(cluster, n):
    """an ascending `cluster` column -> per cluster 0 .. n - 1 the first row that names it, -1: none"""
    cluster = np.asarray(cluster, np.int64)
    ids = np.arange(n, dtype=np.int64)
    pos = np.searchsorted(cluster, ids, side="left")
    has = pos < len(cluster)
    has[has] = cluster[pos[has]] == ids[has]
    return np.where(has, pos, -1)


def _global_ids(parts, ctx):
    """[(local ids, first)] per block -> the global ids i64, the blocks back to back; with `ctx` the offsets are added on the
    device and the column stays there"""
    if ctx is None:
        return _cat([np.asarray(_host(p), np.int64) + int(first) for p, first in parts], np.int64)
    import torch
    cols = [ctx.to_dev(p, torch.int64) + int(first) for p, first in parts]
    return torch.cat(cols) if cols else ctx.empty((0,), torch.int64)


def _field(key, kind, column, ptr=None, index=None, prefix=None, suffix=b"</data>"):
    return dict(kind=kind, column=column, ptr=ptr, index=index, prefix=f'<data key="{key}">'.encode("ascii") if prefix is None else prefix,
                suffix=suffix)


def tables(blocks, ctx=None, families=None, library=None, propagate=None):
    """the blocks -> ((node table, edge table) for `Context.format_records`, None), or (None, why the host writer has to write the
    file).  Every column spans all blocks; a unit finds its hit's, its library row's and its annotation's columns through an i32
    index column (-1: absent)."""
    sw = switches(blocks, families, library, propagate)
    families, library, propagate = sw
    n_of = [len(b["size"]) for b in blocks]
    n = int(sum(n_of))
    for b in blocks:
        for name in ("precursor_mz", "retention_time"):
            if np.asarray(b[name]).dtype != np.float32:
                return None, f"a {name} column is {np.asarray(b[name]).dtype}, not float32"
    charges, why = text_blob(np.array([str(b["charge"]) for b in blocks], dtype=str))
    if charges is None:
        return None, f"a charge {why}"
    cluster = _global_ids([(np.arange(k, dtype=np.int64), b["first"]) for k, b in zip(n_of, blocks)], ctx)
    node = [dict(kind="i64", column=cluster, prefix=b'<node id="', suffix=b'">'),
            _field("v_cluster", "i64", cluster),
            _field("v_precursor_charge", "text", charges[0], charges[1], index=_cat([np.full(k, i) for i, k in enumerate(n_of)], np.int32)),
            _field("v_precursor_mz", "f32", _cat([b["precursor_mz"] for b in blocks], np.float32)),
            _field("v_retention_time", "f32", _cat([b["retention_time"] for b in blocks], np.float32)),
            _field("v_size", "i32", _cat([b["size"] for b in blocks], np.int32))]
    bases = _family_bases(blocks)
    nets = [b["network"] for b in blocks]
    if families:
        fam = _cat([_host(t["node_family"]) for t in nets], np.int64)
        fam_global = _cat([np.asarray(_host(t["node_family"]), np.int64) + base for t, base in zip(nets, bases)], np.int64)
        node += [_field("v_family", "i64", fam_global, index=np.where(fam >= 0, np.arange(n), -1).astype(np.int32)),
                 _field("v_family_size", "i32", _cat([_host(t["node_size"]) for t in nets], np.int32))]
    names = lib_base = None
    if library:
        libs = [b["library"] for b in blocks]
        hit_base = np.concatenate([[0], np.cumsum([len(t["cluster"]) for t in libs])]).astype(np.int64)
        lib_base = np.concatenate([[0], np.cumsum([len(t["name"]) for t in libs])]).astype(np.int64)
        hit = [_first_rows(_host(t["cluster"]), k) for t, k in zip(libs, n_of)]
        hit_idx = _cat([np.where(h >= 0, h + hb, -1) for h, hb in zip(hit, hit_base)], np.int32)
        lib_rows = _cat([np.asarray(_host(t["library"]), np.int64) + lb for t, lb in zip(libs, lib_base)], np.int64)      # by hit
        lib_idx = np.where(hit_idx >= 0, lib_rows[np.maximum(hit_idx, 0)] if len(lib_rows) else -1, -1).astype(np.int32)
        for k in LIBRARY_TEXT:
            blob, why = text_blob(_cat([t[k] for t in libs], str))
            if blob is None:
                return None, f"a library {k} {why}"
            if k == "name":
                names = blob
            node.append(_field(f"v_{k}", "text", blob[0], blob[1], index=lib_idx))
        node += [_field("v_library_cosine", "f32", _cat([_host(t["similarity"]) for t in libs], np.float32), index=hit_idx),
                 _field("v_library_delta_mz", "f32", _cat([_host(t["delta_mz"]) for t in libs], np.float32), index=hit_idx),
                 _field("v_library_matched_peaks", "i32", _cat([_host(t["matched"]) for t in libs], np.int32), index=hit_idx)]
    if propagate and not library:
        return None, "annotations without the library blocks whose rows they name"
    if propagate:
        anns = [b["annotations"] for b in blocks]
        ann_base = np.concatenate([[0], np.cumsum([len(t["cluster"]) for t in anns])]).astype(np.int64)
        ann_idx = _cat([np.where(r >= 0, r + ab, -1) for r, ab in
                        zip((_first_rows(_host(t["cluster"]), k) for t, k in zip(anns, n_of)), ann_base)], np.int32)
        ann_lib = _cat([np.asarray(_host(t["library"]), np.int64) + lb for t, lb in zip(anns, lib_base)], np.int64)       # by annotation
        name_idx = np.where(ann_idx >= 0, ann_lib[np.maximum(ann_idx, 0)] if len(ann_lib) else -1, -1).astype(np.int32)
        node += [_field("v_annotation_hops", "i32", _cat([_host(t["hops"]) for t in anns], np.int32), index=ann_idx),
                 _field("v_annotation_source", "i64", _global_ids([(t["source"], b["first"]) for t, b in zip(anns, blocks)], ctx), index=ann_idx),
                 _field("v_annotation_score", "f32", _cat([_host(t["score"]) for t in anns], np.float32), index=ann_idx),
                 _field("v_annotation_name", "text", names[0], names[1], index=name_idx)]
    m = int(sum(len(t["a"]) for t in nets))
    edge = [dict(kind="i64", column=_global_ids([(t["a"], b["first"]) for t, b in zip(nets, blocks)], ctx), prefix=b'<edge source="', suffix=b""),
            dict(kind="i64", column=_global_ids([(t["b"], b["first"]) for t, b in zip(nets, blocks)], ctx), prefix=b'" target="', suffix=b'">'),
            _field("e_delta_mz", "f32", _cat([_host(t["delta_mz"]) for t in nets], np.float32)),
            _field("e_cosine", "f32", _cat([_host(t["similarity"]) for t in nets], np.float32)),
            _field("e_matched_peaks", "i32", _cat([_host(t["matched"]) for t in nets], np.int32))]
    if families:
        edge.append(_field("e_family", "i64", _cat([np.asarray(_host(t["family"]), np.int64) + base for t, base in zip(nets, bases)], np.int64)))
    return (dict(n=n, head=b"", tail=b"</node>\n", fields=node), dict(n=m, head=b"", tail=b"</edge>\n", fields=edge)), None


def write_device(f, header, blocks, ctx, families=None, library=None, propagate=None, max_bytes=None):
    """the file into the binary file `f` through the device's record writer -> None; or, with nothing written, why the host
    writer has to write it"""
    if ctx is None:
        return "no device context"
    sw = switches(blocks, families, library, propagate)
    both, why = tables(blocks, ctx, *sw)
    if both is None:
        return why
    f.write(prologue(header, sw).encode("utf-8"))
    for table in both:
        for chunk in ctx.format_records(table, max_bytes=max_bytes, copy=False):
            f.write(memoryview(chunk))
    f.write(EPILOGUE.encode("ascii"))
    return None


def write(output_filename: str, header, blocks, ctx=None, writer: str = "host", families=None, library=None, propagate=None) -> None:
    """`<output_filename>.network.graphml`, by the device's record writer (`writer` "device", with `ctx`) or by `write_graphml`;
    the same bytes"""
    filename = f"{output_filename}.network.graphml"
    if writer == "device":
        with open(filename, "wb") as f:
            why = write_device(f, header, blocks, ctx, families, library, propagate)
        if why is None:
            return
        logger.debug("graphml_writer: the host writer writes %s: %s", filename, why)
    with open(filename, "w", encoding="utf-8", newline="\n") as f:
        write_graphml(f, header, blocks, families, library, propagate)
