"""Exact mode (`AnnParams(exact=True)` / `--exact`) without a GPU: option parsing, argument validation before any device is
touched, and the register allocation of the all-pairs edge kernel."""
import os

import numpy as np
import pytest

from tests import isa_lint as L


def test_exact_parses_from_command_line_and_ini(tmp_path):
    from falcon_amd.config import Config
    c = Config()
    c.parse("in.mgf out")
    assert c.exact is False and c.clustering == "dbscan"
    c.parse("in.mgf out --exact --linkage average")
    assert c.exact and c.clustering == "hierarchical" and c.linkage == "average" and c.rescore
    c.parse("in.mgf out --exact --clustering hierarchical")
    assert c.exact and c.clustering == "hierarchical"
    ini = tmp_path / "exact.ini"
    ini.write_text("exact = true\nlinkage = single\n")
    c.parse(f"-c {ini} in.mgf out")
    assert c.exact and c.clustering == "hierarchical" and c.linkage == "single"
    c.parse("in.mgf out")                          # INI values are defaults of their own call only
    assert c.exact is False


def test_exact_with_dbscan_is_a_parse_error(tmp_path):
    from falcon_amd.config import Config
    c = Config()
    with pytest.raises(SystemExit):
        c.parse("in.mgf out --exact --clustering dbscan")
    ini = tmp_path / "exact.ini"
    ini.write_text("exact = true\nclustering = dbscan\n")
    with pytest.raises(SystemExit):
        c.parse(f"-c {ini} in.mgf out")


def test_exact_with_dbscan_raises_before_touching_a_device(monkeypatch):
    from falcon_amd.cluster import cluster
    from falcon_amd.cluster.cluster import AnnParams, SpectrumDataset

    def no_device(*a, **k):
        raise AssertionError("a GPU context was created before the arguments were checked")
    monkeypatch.setattr(cluster, "_default_pipeline", None)
    monkeypatch.setattr(cluster, "ClusterPipeline", no_device)
    ds = SpectrumDataset(np.array([500.0], np.float32), np.zeros(1, np.float32), np.array([200.0], np.float32),
                         np.ones(1, np.float32), np.array([0, 1], np.int64))
    with pytest.raises(ValueError, match="exact"):
        cluster.generate_clusters(ds, "complete", 0.1, 0, 20.0, "ppm", None, 0.05, 2 ** 15,
                                  ann=AnnParams(exact=True, clustering="dbscan"))


def test_exact_default_clustering_is_dbscan_until_exact():
    from falcon_amd.cluster.cluster import AnnParams
    import dataclasses
    p = AnnParams()
    assert p.clustering == "dbscan" and not p.exact
    q = dataclasses.replace(AnnParams(exact=True))
    assert q.exact and q.clustering == "dbscan"     # (generate_clusters turns the default into "hierarchical")


@pytest.mark.skipif(not os.path.exists(L.HIPCC), reason="hipcc not available")
def test_exact_edge_kernel_uses_no_scratch(tmp_path):
    """The hot loop solves 1 x 1 components inline; the Hungarian arrays belong to the fallback kernel only.  If they leak into
    the edge kernel, hipcc puts them in scratch memory and every pair pays for it."""
    asm = L.compile_to_asm("exact.hip", str(tmp_path))
    res = {k: v for k, v in L.kernel_meta(asm, "private_segment_fixed_size").items() if "exact_edges_kernel" in k}
    assert len(res) == 1, sorted(res)
    assert list(res.values()) == [0], res
    lds = {k: v for k, v in L.kernel_meta(asm, "group_segment_fixed_size").items() if "exact_edges_kernel" in k}
    assert list(lds.values())[0] <= 160 * 1024 // 3, lds        # three workgroups per CU
