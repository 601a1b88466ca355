"""Drop-in for `falcon.cluster.cluster.generate_clusters` (reference
falcon/cluster/cluster.py:24-156; call site falcon/falcon.py:178-188) with the
distance + linkage core replaced by the README's vectorise -> ANN -> DBSCAN path,
every stage of which runs in libfalcon_hip.so on one MI355X.

Host logic only: argument handling, the per-bucket `n_list` rule and the order of the
C-ABI calls.  No CPU fallback exists.
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .. import device as _device

logger = logging.getLogger("falcon")

F16_INDEX_DIMS = (64, 128, 256, 400, 800)   # row widths the float16 index kernels (assign16 / list16) are instantiated for =
                                            # the widths `device.row_width(low_dim)` pads the rows to
F16_FLAT_DIMS = (64, 128, 256, 400)         # ... the on-chip top-k of flat buckets (fused.hip) and the hi/lo split scan
FLAT_MAX = 100           # buckets up to this size use a flat (single list) index
MIN_PTS_PER_LIST = 39    # [SURVEY App. A] Faiss' minimum points per centroid
MAX_N_LIST = 1 << 17


class _DefaultClustering(str):
    """AnnParams.clustering's default "dbscan" -- equal to the string, but distinguishable from an explicit choice
    (exact mode turns the default into "hierarchical" and refuses an explicit "dbscan")"""


@dataclass
class AnnParams:
    """The README's nearest-neighbour options (README.md:73-79, 107-117) plus the build's."""
    eps: float = 0.1
    low_dim: int = 400            # any integer in [1, 800] (README.md:114-117): the hash modulus; rows are stored
                                  # `device.row_width(low_dim)` columns wide (64 / 128 / 256 / 400 / 800), zero behind low_dim
    n_probe: int = 16
    n_neighbors: int = 64
    n_neighbors_ann: int = 128
    mz_interval: float = 1.0      # fixed precursor windows in m/z (0 = off) [SURVEY 8(d)]
    kmeans_iters: int = 10        # Faiss IVF default (cp.niter = 10)
    hash_seed: int = 0
    min_mz: float = 101.0
    max_mz: float = 1500.0
    dtype: str = "f32"            # "f32", or "f16": float16 vectors (BASELINE config 5).  The similarity of two float16 vectors is
                                  # the float32 fmaf chain over their (exact) float32 images: buckets with an index run the
                                  # float32 IVF path on the images with the float16 rows as prefilter copies -- bit-identical to
                                  # the oracle's "round to float16, then the float32 path"; flat buckets are scanned on the f16
                                  # matrix cores (float32 accumulation, within 2e-6 of the chain)
    f16_index: bool = True        # dtype "f16": buckets with n_list > n_probe get their k-means index (README.md:107-113); off =
                                  # every bucket exhaustively on the f16 matrix cores (the round-2 behaviour)
    scan: str = "f32"             # flat-bucket scan arithmetic for float32 vectors: "f32" (exact fp32 MFMA) or
                                  # "f16x3" (hi/lo float16 split, 3 f16 MFMAs per step, ~3e-7 absolute error)
    prefilter: bool = False       # float32 flat buckets: keep the top-k on chip (f16-MFMA prefilter + exact float32
                                  # refinement, fused.hip); results are bit-identical with and without it.  Off by default:
                                  # at BASELINE configs[1]'s bucket sizes (<= ~1,100 rows) it is on par with the staged
                                  # scan + select, it pays on larger flat buckets
    ivf_prefilter: bool = True    # float32 buckets with an index: fine scan on the f16 matrix cores to 16-bit keys, the k-th best
                                  # key of every query bracketed from them, exact float32 work only inside the precursor
                                  # window and where it decides the k-th key (ivf16.hip); bit-identical neighbour lists
    kmeans_prefilter: bool = True # IVF buckets with <= 2,048 lists: k-means assignment on the f16 matrix cores, rows whose two
                                  # best centroids are closer than the float16 error bound re-evaluated exactly in float32
                                  # (assign16.hip): the index is identical, the build several times faster
    rescore: bool = False         # re-score the ANN neighbours with the reference's matched-peak cosine
                                  # (similarity.py:17-80) before DBSCAN; uses fragment_tol and min_matches
    min_matches: int = 0          # (set from generate_clusters' `min_matches` when rescore is on)
    clustering: str = _DefaultClustering("dbscan")    # "dbscan" (README.md:143-146) or "hierarchical": the snapshot's linkage +
                                  # fcluster at the distance threshold (cluster.py:283-290) on the re-scored neighbour graph
    linkage: str = "complete"     # (set from generate_clusters' `linkage` when clustering == "hierarchical")
    exact: bool = False           # exact mode: the matched-peak cosine of EVERY pair of each bucket (the snapshot's own
                                  # condensed matrix, cluster.py:593-639), hierarchical clustering on it; no vectors, index
                                  # or search (fal_cluster_exact).  Implies clustering "hierarchical".


def n_list_rule(sizes: np.ndarray, n_probe: int) -> np.ndarray:
    """lists per bucket: flat for tiny buckets, else 2^floor(log2(n/39)) [SURVEY App. A];
    a bucket whose lists would ALL be probed (n_list <= n_probe) is searched exhaustively
    anyway, so it is kept flat and k-means is skipped (same result)."""
    sizes = np.asarray(sizes, np.int64)
    nl = np.ones(len(sizes), np.int64)
    big = sizes > FLAT_MAX
    if big.any():
        nl[big] = 2 ** np.floor(np.log2(sizes[big] / MIN_PTS_PER_LIST)).astype(np.int64)
    nl = np.minimum(nl, MAX_N_LIST)
    nl[nl <= n_probe] = 1
    return nl.astype(np.int32)


class SpectrumDataset:
    """The five columns `generate_clusters` reads (cluster.py:73-85) in CSR form:
    precursor_mz f32[N], retention_time f32[N], mz f32[nnz], intensity f32[nnz],
    indptr i64[N+1].  Arrays may be numpy (uploaded) or tensors already on the GPU."""

    def __init__(self, precursor_mz, retention_time, mz, intensity, indptr, precursor_charge=None):
        self.precursor_mz, self.retention_time = precursor_mz, retention_time
        self.mz, self.intensity, self.indptr = mz, intensity, indptr
        self.precursor_charge = precursor_charge

    def __len__(self):
        return int(self.precursor_mz.shape[0])

    def columns(self):
        return (self.precursor_mz, self.retention_time, self.mz, self.intensity, self.indptr)

    def on_host(self) -> bool:
        """True when the columns are numpy arrays or CPU tensors (they have to cross PCIe before the path can start)"""
        return not any(t is not None and hasattr(t, "is_cuda") and t.is_cuda for t in self.columns())

    def to_device(self, dev, non_blocking: bool = True) -> "SpectrumDataset":
        """-> the same dataset with its columns on `dev`, copies enqueued on the CURRENT stream (asynchronous from pinned memory)"""
        import torch
        # the dtypes the path expects (float32 columns, int64 offsets); a column that is None (retention_time: legal, _front
        # checks for it) stays None
        want = (torch.float32, torch.float32, torch.float32, torch.float32, torch.int64)
        up = []
        for t, dt in zip(self.columns(), want):
            if t is None:
                up.append(None)
                continue
            if not isinstance(t, torch.Tensor):
                t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32 if dt == torch.float32 else np.int64))
            up.append(t.to(dev, dtype=dt, non_blocking=non_blocking))
        return SpectrumDataset(*up, self.precursor_charge)

    def take_rows(self, rows: np.ndarray) -> "SpectrumDataset":
        """Host-side CSR gather: the sub-dataset of `rows` (any order) of a HOST-resident dataset, in pinned memory where torch
        can pin it -- what one GPU of a multi-GPU job uploads instead of the whole partition (a rank touches the peaks
        of its own windows only; reference analogue: `dataset.take(idx)` per block, cluster.py:107-141)."""
        import torch
        as_np = lambda t: t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        rows = np.asarray(rows, np.int64)
        indptr = as_np(self.indptr)
        cnt = indptr[rows + 1] - indptr[rows]
        out = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(cnt, out=out[1:])
        pos = np.repeat(indptr[rows] - out[:-1], cnt) + np.arange(int(out[-1]), dtype=np.int64)

        def pick(col, idx, dt):
            src = as_np(col)
            t = torch.empty(len(idx), dtype=dt, pin_memory=torch.cuda.is_available())
            dst = t.numpy()
            if src.dtype == dst.dtype:
                np.take(src, idx, out=dst)
            else:
                dst[:] = src[idx]
            return t
        rt = None if self.retention_time is None else pick(self.retention_time, rows, torch.float32)
        return SpectrumDataset(pick(self.precursor_mz, rows, torch.float32), rt, pick(self.mz, pos, torch.float32),
                               pick(self.intensity, pos, torch.float32), torch.from_numpy(out), self.precursor_charge)

    @classmethod
    def from_table(cls, table):
        """pyarrow Table / pandas DataFrame with the Lance schema of falcon.py:275-285."""
        if hasattr(table, "to_pandas"):
            table = table.to_pandas()
        mzs = [np.asarray(x, np.float32) for x in table["mz"]]
        its = [np.asarray(x, np.float32) for x in table["intensity"]]
        indptr = np.zeros(len(mzs) + 1, np.int64)
        np.cumsum([len(x) for x in mzs], out=indptr[1:])
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.float32)
        return cls(np.asarray(table["precursor_mz"], np.float32), np.asarray(table["retention_time"], np.float32),
                   cat(mzs), cat(its), indptr,
                   np.asarray(table["precursor_charge"]) if "precursor_charge" in table else None)


class ClusterPipeline:
    """vectorise -> sort -> buckets -> IVF -> search -> filter -> DBSCAN -> refine -> medoids,
    device-resident from the first call to the last."""

    def __init__(self, ctx: Optional[_device.Context] = None, device: int = 0):
        self.ctx = ctx or _device.Context(device)
        self.last = {}

    def plan(self, n: int, batch_size: int, p: "AnnParams"):
        """`fal_ctx_plan` for a pass over `n` spectra: the kernels' code objects loaded, the shape-dependent scratch sized.  The
        reference calls generate_clusters ONCE per charge in a fresh process (falcon.py:153-193): the first pass is the only
        one, so it should not stop for either between its kernels.  Cheap when there is nothing left to do (every `run` calls it)."""
        if p.exact:
            return                       # exact mode sizes its own scratch (no vectors, index or search)
        key = (int(n), int(batch_size), p.low_dim, p.n_neighbors_ann, p.n_probe)
        if getattr(self, "_planned", None) is not None and self._planned[0] >= key[0] and self._planned[1:] == key[1:]:
            return
        self.ctx.plan(n, _device.row_width(p.low_dim), p.n_neighbors_ann, p.n_probe, batch_size)
        self._planned = key

    def trim(self):
        """`fal_ctx_trim` + torch's cache: give this pipeline's cached device memory back (between jobs of very different sizes)"""
        import torch
        for c in (self.ctx, getattr(self, "_front_ctx", None)):
            if c is not None:
                c.trim()
        self._planned = None
        torch.cuda.empty_cache()

    # The path in three phases, so that independent partitions (precursor charges, falcon.py:151-160) can be
    # pipelined: `_front` ends with the path's first host synchronisation (bucket boundaries), `_search` only
    # enqueues, `_graph` ends with the second (cluster counts).
    def _front(self, c, ds, precursor_tol_mass, precursor_tol_mode, rt_tol, batch_size, p, pmz=None):
        """sort by precursor m/z (cluster.py:73-85) + bucket boundaries (a5), on context `c`."""
        import torch
        if pmz is None:
            pmz = c.to_dev(ds.precursor_mz, torch.float32)
        order, mzs = c.sort_by_precursor(pmz)
        rts = c.gather_f32(ds.retention_time, order) if (rt_tol is not None and ds.retention_time is not None) else None
        splits = c.precursor_splits(mzs, precursor_tol_mass, precursor_tol_mode, batch_size, p.mz_interval)
        n_list = n_list_rule(np.diff(splits), p.n_probe)
        if p.dtype == "f16" and not p.f16_index:
            # float16 vectors without an index (AnnParams.f16_index off): every bucket is searched exhaustively on the f16
            # matrix cores -- a superset of what n_probe lists find
            n_list[:] = 1
        return dict(order=order, mzs=mzs, rts=rts, splits=splits, n_list=n_list)

    def plan_shards(self, c, datasets, batch_size, p, world, tol=None):
        """The deal of a multi-partition job to `world` GPUs (`distributed.deal_job`): -> [owner int32[windows] per dataset]
        (an empty array for an empty dataset).  One pass over every partition's precursor column, one wait."""
        import torch
        from .. import distributed as fdist
        # a host-resident partition crosses PCIe with its precursor column only (4 bytes per spectrum) before the deal; the
        # device copy stays with the dataset for the front end of the rank's own windows (`_front_windows`)
        for ds in datasets:
            if ds.on_host():
                ds._pmz_dev = c.to_dev(ds.precursor_mz, torch.float32)
        counts = c.window_counts([getattr(ds, "_pmz_dev", None) if ds.on_host() else ds.precursor_mz for ds in datasets],
                                 p.mz_interval)
        # (`tol` = (precursor tolerance, mode): the cost model then prices the stored neighbours too; exact mode prices the
        # pairs of every bucket instead)
        if p.exact:
            costs = fdist.exact_window_costs(counts, batch_size)
        else:
            costs = fdist.window_costs(counts, batch_size, p.n_probe, p.mz_interval, tol, p.n_neighbors_ann, p.n_neighbors)
        return fdist.deal_job(list(costs), world)

    def _front_windows(self, c, ds, precursor_tol_mass, precursor_tol_mode, rt_tol, batch_size, p, shard, owner=None):
        """The front end of ONE rank of a job that shares a dataset among `world` GPUs, without the replicated
        sort: buckets never cross a precursor window floor(mz / mz_interval) and a window's buckets depend on its own spectra
        only (`fal_precursor_splits`), so whole WINDOWS are the unit that is dealt out.  Every rank histograms the window of
        every spectrum (one pass over 4 bytes per spectrum), derives the same deal from the counts
        (`plan_shards`: `distributed.window_costs` / `deal_job` over all partitions of the job; `owner` = this partition's
        part of it), and sorts / buckets only its own spectra.  The buckets -- hence neighbour
        lists and clusters -- are exactly those of the single-GPU pass.  Reference analogue: blocks are clustered
        independently and only their labels are offset afterwards (cluster.py:107-155).
        -> the state `_restrict` returns: order = rows = dataset rows of this rank's spectra in precursor order, ..."""
        import torch
        from .. import distributed as fdist
        rank, world = shard[0], shard[1]
        pmz = ds.__dict__.pop("_pmz_dev", None) if ds.on_host() else None      # (uploaded by this pass's plan_shards)
        if pmz is None:
            pmz = c.to_dev(ds.precursor_mz, torch.float32)
        n = int(pmz.numel())
        if owner is None:
            owner = self.plan_shards(c, [ds], batch_size, p, world, tol=(precursor_tol_mass, precursor_tol_mode))[0]
        if len(owner) and (owner == rank).all():
            # the whole partition is this rank's: the single-GPU front end, every dataset row in precursor order
            st = self._front(c, ds, precursor_tol_mass, precursor_tol_mode, rt_tol, batch_size, p, pmz=pmz)
            st.update(rows=st["order"], n_total=n)
            return st
        if not (owner == rank).any():
            rows = torch.zeros(0, dtype=torch.int64, device=c.tdev)
        else:
            rows, mz_sub = c.window_select(pmz, p.mz_interval, owner, rank)         # ascending dataset rows: the sort stays stable
        if rows.numel() == 0:
            e = rows.new_zeros(0)
            return dict(order=e, mzs=pmz[:0], rts=None, splits=np.zeros(1, np.int64), n_list=np.zeros(0, np.int32), rows=e,
                        n_total=n)
        order_sub, mzs = c.sort_by_precursor(mz_sub)
        rows_sorted = rows[order_sub]
        rts = c.gather_f32(ds.retention_time, rows_sorted) if (rt_tol is not None and ds.retention_time is not None) else None
        splits = c.precursor_splits(mzs, precursor_tol_mass, precursor_tol_mode, batch_size, p.mz_interval)
        n_list = n_list_rule(np.diff(splits), p.n_probe)
        if p.dtype == "f16" and not p.f16_index:
            n_list[:] = 1
        return dict(order=rows_sorted, mzs=mzs, rts=rts, splits=splits, n_list=n_list, rows=rows_sorted, n_total=n)

    def _restrict(self, c, st, p, shard):
        """One dataset on several GPUs (reference analogue: blocks are clustered independently and only
        their labels are offset afterwards, cluster.py:115-155).  Every rank derived the SAME buckets in `_front`;
        buckets are dealt to ranks by longest-processing-time on `distributed.bucket_costs` (exact mode:
        `distributed.exact_bucket_costs`), and this rank keeps the rows of its own buckets: st becomes the state of that
        subset (buckets whole and in order), plus
        `rows` (i64, device: dataset rows of the subset in sorted order) and `n_total`."""
        import torch
        from .. import distributed as fdist
        rank, world = shard
        splits = np.asarray(st["splits"], np.int64)
        sizes = np.diff(splits)
        costs = fdist.exact_bucket_costs(sizes) if p.exact else fdist.bucket_costs(sizes, st["n_list"], p.n_probe)
        owner = fdist.shard_units(costs, world)
        first, sizes, sub_splits, mine = fdist.shard_buckets(splits, owner, rank)
        n_sub = int(sub_splits[-1])
        if n_sub:
            # sorted positions of the subset's rows, expanded on the device from the per-bucket (first, size) pairs
            shift = c.to_dev(np.stack([first - sub_splits[:-1], sizes]), torch.int64)
            pos_d = torch.repeat_interleave(shift[0], shift[1], output_size=n_sub) + torch.arange(n_sub, device=c.tdev)
        order_sub = st["order"][pos_d] if n_sub else st["order"][:0]
        rts = st["rts"]
        return dict(order=order_sub, mzs=st["mzs"][pos_d] if n_sub else st["mzs"][:0],
                    rts=None if rts is None else (rts[pos_d] if n_sub else rts[:0]), splits=sub_splits,
                    n_list=np.asarray(st["n_list"])[mine], rows=order_sub, n_total=int(st["order"].numel()),
                    buckets=mine)

    def _search(self, ds, st, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol, p, keep_intermediates):
        """a2/a3 vectorise, a6 index, a7 search, a8 filter (+ f4 re-scoring): fills st["nb_idx"], st["nb_dist"]."""
        c = self.ctx
        order, mzs, rts, splits, n_list = st["order"], st["mzs"], st["rts"], st["splits"], st["n_list"]
        n_bins, start, _ = _device.get_dim(p.min_mz, p.max_mz, fragment_tol)      # falcon.py:124-126
        all_flat = bool((n_list == 1).all())
        # `--low_dim` is a free integer (README.md:114-117): the hash runs modulo low_dim, the rows are stored W columns wide
        # (the next width the kernels are instantiated for) with zeros behind -- every kernel below sees d = W
        W = _device.row_width(p.low_dim)
        assert W in F16_INDEX_DIMS
        vec = lambda dt: c.vectorize(ds.mz, ds.intensity, ds.indptr, order, start, fragment_tol, n_bins, p.low_dim,
                                     p.hash_seed, True, dt, width=W)
        X = X16 = Xpre = Xkm = None
        which = 0
        if p.dtype not in ("f32", "f16"):
            raise ValueError(f"unknown dtype {p.dtype!r} (f32 or f16)")
        if p.dtype == "f16" and not all_flat:
            # float16 vectors with an index: the exact kernels (k-means close calls, coarse quantiser, pair chains) work on the
            # float32 image of the rounded rows, the float16 rows themselves are every prefilter copy AND the flat buckets' scan
            X, X16 = vec("f16+image")
            Xkm = X16 if p.kmeans_prefilter else None
            if p.ivf_prefilter and not keep_intermediates:
                which, Xpre = 2, X16
        elif p.dtype == "f16":
            X16 = vec("f16")
        elif p.scan == "f16x3":
            if W not in F16_FLAT_DIMS:
                raise ValueError(f"scan='f16x3' needs low_dim <= {F16_FLAT_DIMS[-1]} (got {p.low_dim})")
            X16 = vec("split16")
            if not all_flat:
                X = vec("f32")              # k-means, coarse quantiser and IVF fine scan stay exact fp32
        else:
            if p.prefilter and not keep_intermediates and W in F16_FLAT_DIMS and bool((n_list == 1).any()):
                which |= 1
            if p.ivf_prefilter and not keep_intermediates and bool((n_list > 1).any()):
                which |= 2
            want_km = p.kmeans_prefilter and bool(((n_list > 1) & (n_list <= 2048)).any())      # (scan.h kAssignMergeLists)
            if want_km or which:
                X, x16 = vec("f32+f16")            # the float16 rounding of the same rows, from the same pass over the peaks
                Xkm = x16 if want_km else None
                Xpre = x16 if which else None
            else:
                X = vec("f32")
        index = c.ivf_build(X, splits, n_list, p.kmeans_iters, X16=X16, Xpre=Xpre, Xkm=Xkm, prefilter_which=max(which, 1))
        if keep_intermediates:
            sim, idx = index.search(p.n_probe, p.n_neighbors_ann)
            nb_idx, nb_dist = c.filter_neighbors(sim, idx, mzs, rts, precursor_tol_mass, precursor_tol_mode, rt_tol,
                                                 p.n_neighbors)
            st.update(sim=sim, idx=idx)
        else:
            # production: a7 + a8 in one call, the [n, k_ann] search result never goes to HBM
            nb_idx, nb_dist = index.search_neighbors(p.n_probe, p.n_neighbors_ann, mzs, rts, precursor_tol_mass,
                                                     precursor_tol_mode, rt_tol, p.n_neighbors)
        if p.rescore:
            nb_dist = c.rescore_neighbors(nb_idx, nb_dist, ds.mz, ds.intensity, ds.indptr, order, fragment_tol,
                                          p.min_matches)
        st.update(X=X, X16=X16, Xpre=Xpre, index=index, nb_idx=nb_idx, nb_dist=nb_dist,
                  nb_count=None if keep_intermediates else index.nb_count)

    def _graph(self, st, precursor_tol_mass, precursor_tol_mode, rt_tol, p, keep_intermediates):
        """a9 DBSCAN, a10 refinement, a11/a12 medoids + labels -> (labels, medoids); `last` describes the partition."""
        c = self.ctx
        order, mzs, rts, nb_idx, nb_dist, index = (st[k] for k in ("order", "mzs", "rts", "nb_idx", "nb_dist", "index"))
        hier = p.linkage if p.clustering == "hierarchical" else None      # f4: the snapshot's linkage + cut at the threshold
        if keep_intermediates:
            # staged calls (one C-ABI call per SURVEY 8a row) so that every intermediate can be inspected
            db, n_db = c.linkage_cluster(nb_idx, nb_dist, p.eps, hier) if hier else c.dbscan(nb_idx, nb_dist, p.eps)
            last = dict(order=order, mz_sorted=mzs, rt_sorted=rts, splits=st["splits"], X=st["X"], X16=st["X16"],
                        n_list=st["n_list"], sim=st["sim"], idx=st["idx"], nb_idx=nb_idx, nb_dist=nb_dist, db=db.clone(),
                        n_db=n_db, index=index)
            lab, n_cl = c.refine_clusters(db, n_db, mzs, rts, precursor_tol_mass, precursor_tol_mode, rt_tol)
            last.update(lab_sorted=lab, n_clusters=n_cl)
            labels, medoids = c.finalize(lab, n_cl, order, nb_idx, nb_dist)
        else:
            # production: a9..a12 fused, counts stay on the device, one synchronisation
            # (after the exact re-scoring a stored neighbour may have moved beyond eps, but it is still stored: counts hold)
            labels, medoids, _, _ = c.cluster_graph(nb_idx, nb_dist, p.eps, mzs, rts, precursor_tol_mass,
                                                    precursor_tol_mode, rt_tol, order, linkage=hier, nb_count=st["nb_count"],
                                                    splits=st["splits"])      # DBSCAN: per bucket tile
            last = dict(nb_idx=nb_idx, nb_dist=nb_dist, nb_count=st["nb_count"], order=order, n_list=st["n_list"],
                        splits=st["splits"])                          # the sparse graph (exchange) + the bucket table
            index.close()
        return labels, medoids, last

    def _exact(self, ds, st, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol, p, keep_intermediates):
        """exact mode after `_front`: every pair of every bucket scored, linkage cut at eps, refinement, exact medoids, labels
        (fal_cluster_exact: the edges stay in library scratch).  With `keep_intermediates` the staged edge call runs as well
        and `last` carries its CSR; `last` always carries the bucket table."""
        c = self.ctx
        order, mzs, rts, splits = (st[k] for k in ("order", "mzs", "rts", "splits"))
        last = dict(order=order, mz_sorted=mzs, rt_sorted=rts, splits=splits, csr=None)
        if keep_intermediates:
            last["csr"] = c.exact_edges(ds.mz, ds.intensity, ds.indptr, order, splits, fragment_tol, p.min_matches, p.eps)
        labels, medoids, lab_sorted, n_cl = c.cluster_exact(ds.mz, ds.intensity, ds.indptr, order, splits, fragment_tol,
                                                            p.min_matches, p.eps, p.linkage, mzs, rts, precursor_tol_mass,
                                                            precursor_tol_mode, rt_tol)
        last.update(lab_sorted=lab_sorted, n_clusters=n_cl)
        return labels, medoids, last

    def run(self, ds: SpectrumDataset, precursor_tol_mass: float, precursor_tol_mode: str,
            rt_tol: Optional[float], fragment_tol: float, batch_size: int, p: AnnParams,
            keep_intermediates: bool = False):
        """-> (labels_dev i32[N], medoids_dev i32[n_labels]) as device tensors."""
        import torch
        c = self.ctx
        if len(ds) == 0:
            return c.empty((0,), torch.int32), c.empty((0,), torch.int32)
        self.plan(len(ds), batch_size, p)
        st = self._front(c, ds, precursor_tol_mass, precursor_tol_mode, rt_tol, batch_size, p)
        if p.exact:
            labels, medoids, self.last = self._exact(ds, st, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol, p,
                                                     keep_intermediates)
            return labels, medoids
        self._search(ds, st, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol, p, keep_intermediates)
        labels, medoids, self.last = self._graph(st, precursor_tol_mass, precursor_tol_mode, rt_tol, p, keep_intermediates)
        return labels, medoids

    def run_many(self, datasets, precursor_tol_mass: float, precursor_tol_mode: str, rt_tol: Optional[float],
                 fragment_tol: float, batch_size: int, p: AnnParams, shard: Optional[Tuple[int, int]] = None):
        """Several independent partitions, software-pipelined on one GPU: the light front end of partition i + 1
        (sort + bucket boundaries, on a second stream / context) and its host planning run while the scan of
        partition i occupies the matrix cores; all heavy kernels stay on the pipeline's own stream, in order.
        Same results as `run` per partition.  -> [(labels, medoids), ...]; `self.lasts` holds every `last`.

        `shard = (rank, world)`: every partition is ONE dataset shared by `world` GPUs; this rank runs the path on
        its own precursor buckets only (`_restrict`).  Labels / medoids then refer to the rank's rows in sorted
        order (labels[i] belongs to dataset row lasts[j]["rows"][i]; medoids index the same rows) and
        lasts[j]["rows"] (i64, device) maps them back -- the exchange step assembles the global result."""
        import torch
        c = self.ctx
        if p.exact and shard is not None and shard[1] > 1:
            return self._run_many_exact_sharded(datasets, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol,
                                                batch_size, p, shard)
        if p.exact:
            # exact mode: one partition after the other (no scan to overlap a front end with)
            outs, self.lasts = [], []
            for ds in datasets:
                outs.append(self.run(ds, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol, batch_size, p))
                self.lasts.append(self.last if len(ds) > 0 else {})
            if self.lasts:
                self.last = self.lasts[-1]
            return outs
        args = (precursor_tol_mass, precursor_tol_mode, rt_tol)
        live = [i for i, ds in enumerate(datasets) if len(ds) > 0]
        if live:
            self.plan(max(len(datasets[i]) for i in live), batch_size, p)
        if len(live) > 1 and not hasattr(self, "_front_ctx"):
            self._front_stream = torch.cuda.Stream(device=c.tdev)
            with torch.cuda.stream(self._front_stream):
                self._front_ctx = _device.Context(c.device)               # bound to the front stream
        # one partition: nothing to overlap -- its front end runs on the pipeline's own stream (a `PartitionRunner` slot must
        # not spread over more streams than it has to: HIP folds streams onto a few hardware queues, and a front end queued
        # behind another slot's scan kernel waits for it)
        front_stream = self._front_stream if len(live) > 1 else torch.cuda.current_stream(c.tdev)
        front_ctx = self._front_ctx if len(live) > 1 else c
        states = {}
        sharded = shard is not None and shard[1] > 1
        windows = sharded and bool(p.mz_interval and p.mz_interval > 0)
        owners = None
        if windows:
            # the deal covers ALL partitions of the job (a rank owns whole partitions where it can); a caller that runs the
            # partitions of one job through several pipelines (PartitionRunner) plans once and passes every call its part
            owners = shard[2] if len(shard) > 2 else None
            if owners is None:
                front_stream.wait_stream(torch.cuda.current_stream(c.tdev))
                with torch.cuda.stream(front_stream):
                    owners = self.plan_shards(front_ctx, datasets, batch_size, p, shard[1], tol=args[:2])

        def front(i):
            with torch.cuda.stream(front_stream):
                if windows:
                    st = self._front_windows(front_ctx, datasets[i], *args, batch_size, p, shard, owner=owners[i])
                else:
                    st = self._front(front_ctx, datasets[i], *args, batch_size, p)
                    if sharded:                                                # no windows: whole buckets of the sorted dataset
                        st = self._restrict(front_ctx, st, p, shard[:2])
                if sharded:
                    # labels refer to the subset's own rows; `rows` maps them to dataset rows
                    st["order"] = torch.arange(st["rows"].numel(), dtype=torch.int64, device=c.tdev)
                states[i] = st

        if live:
            # inputs may have been produced on the caller's stream
            front_stream.wait_stream(torch.cuda.current_stream(c.tdev))
            front(live[0])
        for pos, i in enumerate(live):
            if states[i]["order"].numel() > 0:
                if sharded and datasets[i].on_host():
                    # a rank touches the peaks of its own windows only -- of a HOST-resident partition it uploads just
                    # those: the rows come back (8 bytes each), the host gathers their CSR in sorted order into pinned memory
                    # (`take_rows`), and the path runs on that sub-dataset as it stands (row i = sorted position i)
                    front_stream.synchronize()
                    sub = datasets[i].take_rows(states[i]["rows"].cpu().numpy())
                    sub = SpectrumDataset(None, None, c.to_dev(sub.mz), c.to_dev(sub.intensity), c.to_dev(sub.indptr))
                    self._search(sub, states[i], *args, fragment_tol, p, False)      # (order = arange: set in front())
                elif sharded:
                    # the subset's rows in sorted order = dataset rows `rows`: vectorise gathers them from the CSR
                    st = dict(states[i], order=states[i]["rows"])
                    torch.cuda.current_stream(c.tdev).wait_stream(front_stream)
                    self._search(datasets[i], st, *args, fragment_tol, p, False)
                    st["order"] = states[i]["order"]
                    states[i] = st
                else:
                    self._search(datasets[i], states[i], *args, fragment_tol, p, False)   # enqueue only
            if pos + 1 < len(live):
                front(live[pos + 1])                                               # overlaps the scan just enqueued
        outs, self.lasts = [], []
        for i, ds in enumerate(datasets):
            if len(ds) == 0 or states[i]["order"].numel() == 0:
                outs.append((c.empty((0,), torch.int32), c.empty((0,), torch.int32)))
                self.lasts.append({"rows": c.empty((0,), torch.int64)} if sharded else {})
                continue
            labels, medoids, last = self._graph(states[i], *args, p, False)
            if sharded:
                last["rows"] = states[i]["rows"]
            outs.append((labels, medoids))
            self.lasts.append(last)
        if self.lasts:
            self.last = self.lasts[-1]
        return outs

    def _run_many_exact_sharded(self, datasets, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol, batch_size, p,
                                shard):
        """`run_many(shard=...)` in exact mode: buckets are independent (no neighbour list crosses one, there is no index), so a
        rank runs `_exact` on its own whole buckets -- windows dealt job-wide on `distributed.exact_window_costs`
        (`mz_interval` > 0, `_front_windows`), else the replicated sort and `_restrict` on `distributed.exact_bucket_costs`.
        The subset runs as a compact CSR (row i = sorted position i), so the kernel's outputs are sized to it.  Same
        contract as the nearest-neighbour path: labels / medoids over the subset, `lasts[j]["rows"]` = its dataset rows."""
        import torch
        c = self.ctx
        args = (precursor_tol_mass, precursor_tol_mode, rt_tol)
        windows = bool(p.mz_interval and p.mz_interval > 0)
        owners = shard[2] if len(shard) > 2 else None
        if windows and owners is None:
            owners = self.plan_shards(c, datasets, batch_size, p, shard[1])
        outs, self.lasts = [], []
        for j, ds in enumerate(datasets):
            st = None
            if len(ds) > 0:
                if windows:
                    st = self._front_windows(c, ds, *args, batch_size, p, shard[:2], owner=owners[j])
                else:
                    st = self._restrict(c, self._front(c, ds, *args, batch_size, p), p, shard[:2])
            if st is None or st["rows"].numel() == 0:
                outs.append((c.empty((0,), torch.int32), c.empty((0,), torch.int32)))
                self.lasts.append({"rows": c.empty((0,), torch.int64)})
                continue
            rows = st["rows"]
            st["order"] = torch.arange(rows.numel(), dtype=torch.int64, device=c.tdev)
            labels, medoids, last = self._exact(self._take_rows(c, ds, rows), st, *args, fragment_tol, p, False)
            last["rows"] = rows
            outs.append((labels, medoids))
            self.lasts.append(last)
        if self.lasts:
            self.last = self.lasts[-1]
        return outs

    @staticmethod
    def _take_rows(c, ds, rows):
        """the peaks of dataset rows `rows` (i64, device) as a compact CSR on the device: row i of the result = rows[i].
        A host-resident dataset gathers them on the host into pinned memory (`take_rows`) and uploads only those; a
        device-resident one gathers them with a few device ops (the expansion `_restrict` uses)."""
        import torch
        if ds.on_host():
            sub = ds.take_rows(rows.cpu().numpy())
            return SpectrumDataset(None, None, c.to_dev(sub.mz), c.to_dev(sub.intensity), c.to_dev(sub.indptr))
        indptr = c.to_dev(ds.indptr, torch.int64)
        start = indptr[rows]
        cnt = indptr[rows + 1] - start
        out = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=c.tdev)
        torch.cumsum(cnt, 0, out=out[1:])
        nnz = int(out[-1].item())
        pos = torch.repeat_interleave(start - out[:-1], cnt, output_size=nnz) + torch.arange(nnz, device=c.tdev)
        return SpectrumDataset(None, None, c.to_dev(ds.mz, torch.float32)[pos], c.to_dev(ds.intensity, torch.float32)[pos],
                               out)

    def run_chunked(self, datasets, precursor_tol_mass: float, precursor_tol_mode: str, rt_tol: Optional[float],
                    fragment_tol: float, batch_size: int, p: AnnParams, n_chunks: int, on_chunk=None):
        """Datasets whose working set exceeds one pass (BASELINE configs[3]: 50 M spectra need ~260 GB of vectors, index,
        keys and hand-off buffers at once): the precursor buckets are dealt into `n_chunks` shares exactly as they are
        dealt to GPUs (`_restrict`: LPT on `distributed.bucket_costs`; no neighbour pair crosses a bucket, reference
        cluster.py:107-141) and the shares run one after the other on this GPU, each through `run_many(shard=(c,
        n_chunks))`.  Same partition as one pass; cluster ids are share-major (the reference offsets the labels of its
        blocks the same way, cluster.py:144-155).  `on_chunk(c, outs, lasts)` sees every share's raw results.
        -> [(labels i32[N_j] by dataset row, medoids i32[n_labels_j] dataset rows)] per dataset."""
        import torch
        c = self.ctx
        if n_chunks <= 1 or p.exact:
            # (exact mode holds no vectors, index or hand-off buffers: its working set is the edges, one pass)
            return self.run_many(datasets, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol, batch_size, p)
        labels = [torch.full((len(ds),), -1, dtype=torch.int32, device=c.tdev) for ds in datasets]
        medoids = [[] for _ in datasets]
        off = [0] * len(datasets)
        for ch in range(n_chunks):
            outs = self.run_many(datasets, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol, batch_size, p,
                                 shard=(ch, n_chunks))
            _merge_share(labels, medoids, off, outs, self.lasts)
            if on_chunk is not None:
                on_chunk(ch, outs, self.lasts)
            del outs
        return [(labels[j], torch.cat(medoids[j]) if medoids[j] else c.empty((0,), torch.int32)) for j in range(len(datasets))]


def _merge_share(labels, medoids, off, outs, lasts):
    """one bucket share's results into the job's: labels by dataset row with share-major cluster ids (the reference offsets the
    labels of its blocks the same way, cluster.py:144-155), medoids as dataset rows; `off[j]` = clusters of partition j so far"""
    import torch
    for j, ((lab, med), last) in enumerate(zip(outs, lasts)):
        rows = last.get("rows")
        if rows is None or rows.numel() == 0:
            continue
        labels[j][rows] = lab + off[j]
        medoids[j].append(rows[med.long()].to(torch.int32))
        off[j] += int(med.numel())


class PartitionRunner:
    """Runs independent partitions (precursor charges, falcon.py:151-160) concurrently: one host
    thread + one HIP stream + one `fal_ctx` per partition slot, the way the reference clusters its
    blocks on a thread pool (cluster.py:115-136).  The GPU interleaves the streams, so the host
    planning / synchronisation gaps of one partition hide under the kernels of the other."""

    def __init__(self, device: int = 0, n_slots: int = 2):
        import threading
        from concurrent.futures import ThreadPoolExecutor
        self.device, self.n_slots = device, n_slots
        self._tls = threading.local()
        self._pool = ThreadPoolExecutor(max_workers=n_slots, thread_name_prefix="falcon-part")
        self.pipelines = []
        self._lock = threading.Lock()

    def _pipeline(self):
        import torch
        if not hasattr(self._tls, "pipe"):
            torch.cuda.set_device(self.device)
            self._tls.stream = torch.cuda.Stream(device=self.device)
            with torch.cuda.stream(self._tls.stream):
                self._tls.pipe = ClusterPipeline(device=self.device)      # binds the ctx to this stream
            with self._lock:
                self.pipelines.append(self._tls.pipe)
        return self._tls.pipe, self._tls.stream

    def _run_one(self, ds, args, kwargs, shard, arrived=None):
        import torch
        pipe, stream = self._pipeline()
        with torch.cuda.stream(stream):
            if arrived is not None:
                stream.wait_event(arrived)                     # the partition's bytes (uploaded by `run` on the copy stream)
            if shard is not None and shard[1] > 1:
                out = pipe.run_many([ds], *args, shard=shard, **kwargs)[0]       # this rank's windows of the partition
                pipe.last = pipe.lasts[0]
            else:
                out = pipe.run(ds, *args, **kwargs)
            stream.synchronize()
        return out, pipe, dict(pipe.last)        # (a snapshot: the same slot may serve another partition next)

    def run(self, datasets, *args, shard: Optional[Tuple[int, int]] = None, **kwargs):
        """-> [(labels, medoids), ...] in the order of `datasets` (largest partition is started first).  `shard = (rank,
        world)`: every partition is one dataset shared by `world` GPUs, as in `ClusterPipeline.run_many`."""
        return self.collect(self.submit(datasets, *args, shard=shard, **kwargs))

    def collect(self, handle):
        """the results of a `submit`: waits for its partitions (each slot has synchronised its own stream)"""
        futs, n, nothing = handle
        res = [futs[i].result()[::2] if i in futs else nothing() for i in range(n)]
        self.lasts = [r[1] for r in res]                           # every partition's `last`, in the order of `datasets`
        return [r[0] for r in res]

    def submit(self, datasets, *args, shard: Optional[Tuple[int, int]] = None, inputs_ready: bool = False, **kwargs):
        """`run` without the wait: the partitions are queued on the slots (behind whatever the slots are still working on -- a
        stream of jobs keeps the GPU busy across job boundaries) and a handle for `collect` comes back.  `inputs_ready`: the
        datasets were complete on the device before the call (no wait for the caller's stream)."""
        import torch
        if not inputs_ready:
            torch.cuda.current_stream(self.device).synchronize()      # inputs produced on the caller's stream
        p = args[5] if len(args) > 5 else kwargs["p"]
        order = sorted(range(len(datasets)), key=lambda i: -len(datasets[i]))
        shards = [shard] * len(datasets)
        if shard is not None and shard[1] > 1 and p.mz_interval and p.mz_interval > 0:
            # one deal for the whole job (`distributed.deal_job` over every partition's windows), then a slot per partition
            if not hasattr(self, "_planner"):
                self._planner = ClusterPipeline(device=self.device)
            owners = self._planner.plan_shards(self._planner.ctx, datasets, args[4], p, shard[1], tol=args[:2])      # (waits for the counts)
            shards = [(shard[0], shard[1], [owners[i]]) for i in range(len(datasets))]
            order = [i for i in order if (owners[i] == shard[0]).any()]        # partitions this rank has windows of
        dev = torch.device("cuda", self.device)
        # Host-resident partitions (the reference hands numpy columns over: cluster.py:73-85) cross PCIe on ONE copy stream,
        # largest partition first, each followed by an event: a partition's kernels start when ITS bytes have arrived, the
        # next partition's upload travels under them (pinned memory makes the copies asynchronous).
        arrived = {}
        sharded = shard is not None and shard[1] > 1
        if not sharded and any(datasets[i].on_host() for i in order):     # (a sharded rank uploads its own windows only: run_many)
            if not hasattr(self, "_copy_stream"):
                self._copy_stream = torch.cuda.Stream(device=self.device)
            datasets = list(datasets)
            with torch.cuda.stream(self._copy_stream):
                for i in order:
                    if datasets[i].on_host():
                        datasets[i] = datasets[i].to_device(dev)
                        arrived[i] = torch.cuda.Event()
                        arrived[i].record(self._copy_stream)
        futs = {i: self._pool.submit(self._run_one, datasets[i], args, kwargs, shards[i], arrived.get(i)) for i in order}
        nothing = lambda: ((torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)),
                           {"rows": torch.empty(0, dtype=torch.int64, device=dev)})
        return futs, len(datasets), nothing

    def plan(self, datasets, *args, **kwargs):
        """Before the first pass of a fresh process: create every slot's thread, stream and context and `fal_ctx_plan` each for the
        job's largest partition (code objects loaded once per process, scratch sized).  Optional -- `run` does the same lazily."""
        import threading
        n = max((len(ds) for ds in datasets), default=0)
        batch_size, p = args[4], args[5]
        gate = threading.Barrier(self.n_slots)

        def one():
            pipe, stream = self._pipeline()
            import torch
            with torch.cuda.stream(stream):
                pipe.plan(n, batch_size, p)
            gate.wait()                                  # (every worker thread takes exactly one of the n_slots tasks)
        for f in [self._pool.submit(one) for _ in range(self.n_slots)]:
            f.result()

    def trim(self):
        """every slot's `ClusterPipeline.trim` (the slots are idle between two `run` calls)"""
        with self._lock:
            pipes = list(self.pipelines)
        for pipe in pipes + ([self._planner] if hasattr(self, "_planner") else []):
            pipe.trim()

    def run_chunked(self, datasets, *args, n_chunks: int, on_chunk=None, **kwargs):
        """`ClusterPipeline.run_chunked` with the partitions of every bucket share on concurrent slots: the precursor windows of the
        job are dealt into `n_chunks` shares exactly as they are dealt to GPUs, the shares run one after the other, each
        through `run(shard=(c, n_chunks))`.  Same partition as one pass; cluster ids are share-major.
        -> [(labels i32[N_j] by dataset row, medoids i32[n_labels_j] dataset rows)] per dataset."""
        import torch
        if n_chunks <= 1 or (args[5] if len(args) > 5 else kwargs["p"]).exact:
            return self.run(datasets, *args, **kwargs)         # (exact mode: one pass, as ClusterPipeline.run_chunked)
        dev = torch.device("cuda", self.device)
        labels = [torch.full((len(ds),), -1, dtype=torch.int32, device=dev) for ds in datasets]
        medoids = [[] for _ in datasets]
        off = [0] * len(datasets)
        for ch in range(n_chunks):
            outs = self.run(datasets, *args, shard=(ch, n_chunks), **kwargs)
            _merge_share(labels, medoids, off, outs, self.lasts)
            if on_chunk is not None:
                on_chunk(ch, outs, self.lasts)
            del outs
        return [(labels[j], torch.cat(medoids[j]) if medoids[j] else torch.empty(0, dtype=torch.int32, device=dev))
                for j in range(len(datasets))]

    def close(self):
        self._pool.shutdown(wait=True)


_default_pipeline: Optional[ClusterPipeline] = None


def resolve_params(linkage: str, distance_threshold: float, min_matches: int, ann: Optional[AnnParams] = None) -> AnnParams:
    """The parameters a pass runs with, from `generate_clusters`' arguments (and the CLI's, single or distributed): eps =
    distance_threshold, exact mode => hierarchical, linkage / re-scoring / min_matches for the hierarchical clustering.
    Raises ValueError on a combination the path cannot honour.  Never mutates `ann`."""
    import dataclasses
    if linkage not in ("complete", "single", "average"):
        raise ValueError(f"unknown linkage {linkage!r} (choose complete, single or average; cluster.py:283-290)")
    if ann is None:
        p = AnnParams(eps=float(distance_threshold))
    else:
        if abs(float(ann.eps) - float(distance_threshold)) > 1e-12:
            raise ValueError(f"distance_threshold ({distance_threshold}) and ann.eps ({ann.eps}) differ: they name the same "
                             "cosine-distance threshold (README.md:73-79, config.py:104-111)")
        p = dataclasses.replace(ann)                 # never mutate the caller's parameters
    if p.rescore:
        p.min_matches = int(min_matches)
    if p.exact:
        if p.clustering == "dbscan" and not isinstance(p.clustering, _DefaultClustering):
            raise ValueError("exact mode clusters the all-pairs distances hierarchically (the snapshot's linkage); "
                             "AnnParams(exact=True) does not combine with clustering=\"dbscan\"")
        p.clustering = "hierarchical"
    if p.clustering not in ("dbscan", "hierarchical"):
        raise ValueError(f"unknown clustering {p.clustering!r}")
    if p.clustering == "hierarchical":
        p.linkage = linkage
        p.rescore = True                 # the linkage runs on the exact matched-peak distances (cluster.py:283-290)
        p.min_matches = int(min_matches)
    elif linkage != "complete":
        raise ValueError(f"linkage={linkage!r} only applies to the hierarchical clustering of the exact distances "
                         "(AnnParams(clustering=\"hierarchical\", rescore=True) / --clustering hierarchical); the default "
                         "nearest-neighbour path clusters with DBSCAN and would ignore it")
    return p


def generate_clusters(dataset, linkage: str, distance_threshold: float, min_matches: int,
                      precursor_tol_mass: float, precursor_tol_mode: str, rt_tol: Optional[float],
                      fragment_tol: float, batch_size: int, *, ann: Optional[AnnParams] = None,
                      pipeline: Optional[ClusterPipeline] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Same call as the reference (cluster.py:24-34).  `distance_threshold` is the cosine
    distance threshold and plays the role of DBSCAN's eps (README.md:73-79); `linkage` and
    `min_matches` belong to the snapshot's exact-cosine path: `min_matches` is used when `ann.rescore` is on
    (matched-peak re-scoring of the ANN neighbours, similarity.py:17-80); `linkage` selects the hierarchical
    clustering of those exact distances when `ann.clustering == "hierarchical"` and is an error otherwise unless
    it is the reference default "complete".

    Returns (labels int32[N] by dataset row with noise renumbered as singletons --
    cluster.py:144-155 --, medoids int32[n_labels]: medoids[c] = dataset row representing
    cluster c, usable as `dataset.take(medoids)`, falcon.py:198-203)."""
    global _default_pipeline
    if not isinstance(dataset, SpectrumDataset):
        dataset = SpectrumDataset.from_table(
            dataset.to_table(columns=["precursor_mz", "precursor_charge", "retention_time", "mz", "intensity"])
            if hasattr(dataset, "to_table") else dataset)
    p = resolve_params(linkage, distance_threshold, min_matches, ann)
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    logger.info("Cluster %d spectra: low_dim=%d n_probe=%d n_neighbors=%d/%d eps=%.3f", len(dataset), p.low_dim,
                p.n_probe, p.n_neighbors, p.n_neighbors_ann, p.eps)
    labels, medoids = pipe.run(dataset, precursor_tol_mass, precursor_tol_mode, rt_tol, fragment_tol, batch_size, p)
    return labels.cpu().numpy(), medoids.cpu().numpy()


def consensus_spectra(dataset, labels, medoids, fragment_tol: float, min_fraction: float = 0.25,
                      pipeline: Optional[ClusterPipeline] = None):
    """Consensus representatives of the clusters `generate_clusters` returned for `dataset` (a SpectrumDataset on the host or the
    device, or what `generate_clusters` accepts): every cluster's members merged peak by peak (`fal_consensus_spectra`; DESIGN.md
    "Consensus representatives").  A merged peak is kept when min(its peaks, members) >= max(1, ceil(min_fraction * members)).

    Returns (indptr int64[n_clusters + 1], mz float32[], intensity float32[], status int32[n_clusters]): cluster c's consensus
    peaks are mz / intensity[indptr[c]:indptr[c + 1]] in m/z order, L2-normalised; status bit `_lib.CONS_FALLBACK` marks the
    clusters without a kept peak, which carry their medoid's peaks; a cluster of one member carries that member's peaks."""
    global _default_pipeline
    if not isinstance(dataset, SpectrumDataset):
        dataset = SpectrumDataset.from_table(
            dataset.to_table(columns=["precursor_mz", "precursor_charge", "retention_time", "mz", "intensity"])
            if hasattr(dataset, "to_table") else dataset)
    if not 0.0 < float(min_fraction) <= 1.0:
        raise ValueError("min_fraction must lie in (0, 1]")
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    indptr, mz, intensity, status = pipe.ctx.consensus_spectra(dataset.mz, dataset.intensity, dataset.indptr, labels, medoids,
                                                               fragment_tol, min_fraction)
    return indptr.cpu().numpy(), mz.cpu().numpy(), intensity.cpu().numpy(), status.cpu().numpy()


def _member_scores_dev(ctx, dataset, labels, medoids, fragment_tol, consensus):
    """the device tensors of `member_scores` for a SpectrumDataset"""
    if consensus is None:
        rep_indptr, rep_mz, rep_intensity, rep_row = dataset.indptr, dataset.mz, dataset.intensity, medoids
    else:
        rep_indptr, rep_mz, rep_intensity = consensus
        rep_row = np.arange(len(medoids), dtype=np.int32)
        if len(rep_indptr) != len(medoids) + 1:
            raise ValueError(f"consensus holds {len(rep_indptr) - 1} spectra for {len(medoids)} clusters")
    return ctx.member_scores(dataset.mz, dataset.intensity, dataset.indptr, labels, rep_mz, rep_intensity, rep_indptr, rep_row,
                             fragment_tol)


def _as_dataset(dataset):
    if isinstance(dataset, SpectrumDataset):
        return dataset
    return SpectrumDataset.from_table(
        dataset.to_table(columns=["precursor_mz", "precursor_charge", "retention_time", "mz", "intensity"])
        if hasattr(dataset, "to_table") else dataset)


def member_scores(dataset, labels, medoids, fragment_tol: float, consensus=None, pipeline: Optional[ClusterPipeline] = None):
    """Every spectrum of `dataset` scored against the representative of its cluster, for the clusters `generate_clusters`
    returned (`fal_member_scores`; DESIGN.md "Member scores and cluster summary"): the matched-peak cosine of the snapshot's
    `cosine_fast(member, representative, fragment_tol)`, clipped to [0, 1].  The representative is the medoid's spectrum, or
    with `consensus` (the (indptr, mz, intensity) triple `consensus_spectra` returns) the cluster's consensus peaks.
    `min_matched_peaks` is not applied: both numbers are reported.

    Returns (similarity float32[n], matched int32[n]) by dataset row."""
    global _default_pipeline
    dataset = _as_dataset(dataset)
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    sim, matched = _member_scores_dev(pipe.ctx, dataset, labels, medoids, fragment_tol, consensus)
    return sim.cpu().numpy(), matched.cpu().numpy()


def cluster_summary(dataset, labels, medoids, fragment_tol: float, consensus=None, pipeline: Optional[ClusterPipeline] = None):
    """`member_scores` and, per cluster, what they say about it (`fal_cluster_summary`).

    Returns a dict of host arrays: per cluster `size` int32, `sim_min` float32, `worst_row` int32 (the member with `sim_min`,
    the lowest row among equals), `sim_mean` float64, `pmz_min`, `pmz_max`, `rt_min`, `rt_max` float32 (the retention times 0
    for a dataset without them); per spectrum `similarity` float32 and `matched` int32."""
    global _default_pipeline
    dataset = _as_dataset(dataset)
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    sim, matched = _member_scores_dev(pipe.ctx, dataset, labels, medoids, fragment_tol, consensus)
    cols = pipe.ctx.cluster_summary(labels, len(medoids), sim, dataset.precursor_mz, dataset.retention_time)
    out = {k: v.cpu().numpy() for k, v in cols.items()}
    out["similarity"], out["matched"] = sim.cpu().numpy(), matched.cpu().numpy()
    return out


def representative_network(dataset, medoids, fragment_tol: float, max_shift: float = 200.0, min_cosine: float = 0.7,
                           min_matched_peaks: int = 6, top_k: int = 10, consensus=None,
                           pipeline: Optional[ClusterPipeline] = None, on_device: bool = False):
    """Molecular network of the clusters `generate_clusters` returned for `dataset` (`fal_network_edges`; DESIGN.md
    "Representative network"): cluster c is a node with the peaks of its medoid's spectrum -- or, with `consensus` (the (indptr,
    mz, intensity) triple `consensus_spectra` returns), its consensus peaks -- and the medoid's precursor m/z.  Two clusters whose
    precursors differ by at most `max_shift` m/z are linked when their greedy modified cosine (peaks matching at the same m/z or
    shifted by the precursor difference; the GNPS / matchms matching, not the optimal assignment) is at least `min_cosine` with at
    least `min_matched_peaks` matched peaks, and, with `top_k` > 0, the link is among the `top_k` best of both clusters.

    Returns a dict of host arrays in (a, b) order: `a`, `b` int32 (cluster indices, a < b), `similarity` float32, `matched`
    int32, `delta_mz` float32 = float32(precursor_mz[medoid b] - precursor_mz[medoid a]).  `on_device`: the same columns as device
    tensors (what `network_families` takes without another copy)."""
    global _default_pipeline
    dataset = _as_dataset(dataset)
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    ctx = pipe.ctx
    import torch
    m = ctx.to_dev(medoids, torch.int64)
    pmz = ctx.to_dev(dataset.precursor_mz, torch.float32)[m]
    if consensus is None:
        indptr, mz, intensity, rows = dataset.indptr, dataset.mz, dataset.intensity, m.to(torch.int32)
    else:
        indptr, mz, intensity = consensus
        rows = np.arange(len(m), dtype=np.int32)
        if len(indptr) != len(m) + 1:
            raise ValueError(f"consensus holds {len(indptr) - 1} spectra for {len(m)} clusters")
    a, b, sim, matched = ctx.network_edges(mz, intensity, indptr, rows, pmz, fragment_tol, max_shift, min_cosine,
                                           min_matched_peaks, top_k)
    cols = dict(a=a, b=b, similarity=sim, matched=matched, delta_mz=pmz[b.long()] - pmz[a.long()])
    return cols if on_device else {k: v.cpu().numpy() for k, v in cols.items()}


def library_search(dataset, medoids, library, fragment_tol: float, precursor_tol: float, mode: str, analog: bool = False,
                   max_shift: float = 200.0, min_cosine: float = 0.7, min_matched_peaks: int = 6, top_n: int = 1, consensus=None,
                   pipeline: Optional[ClusterPipeline] = None):
    """Library search of the clusters `generate_clusters` returned for `dataset` (`fal_library_search`; DESIGN.md "Library
    search"): cluster c is a query with the peaks of its medoid's spectrum -- or, with `consensus` (the (indptr, mz, intensity)
    triple `consensus_spectra` returns), its consensus peaks -- and the medoid's precursor m/z.  `library` is a SpectrumDataset
    (or a dict with its columns) of reference spectra of the same charge.  Exact search: the library spectra inside
    `precursor_tol` (`mode` "ppm" or "Da") of the query's precursor, scored by the greedy cosine; `analog`: those within
    `max_shift` m/z, scored by the greedy modified cosine (peaks matching at the same m/z or shifted by the precursor
    difference).  A pair is a hit with a score of at least `min_cosine` and at least `min_matched_peaks` matched peaks; a
    cluster keeps its `top_n` best hits (0: all), equal scores in library order.

    Returns a dict of host arrays in (cluster, rank) order: `cluster`, `library` int32 (cluster index, library row),
    `similarity` float32, `matched` int32, `delta_mz` float32 = float32(precursor_mz[medoid] - library precursor_mz)."""
    global _default_pipeline
    dataset, library = _as_dataset(dataset), _as_dataset(library)
    if mode not in ("ppm", "Da"):
        raise ValueError('library_search: mode must be "ppm" or "Da"')
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    ctx = pipe.ctx
    import torch
    m = ctx.to_dev(medoids, torch.int64)
    pmz = ctx.to_dev(dataset.precursor_mz, torch.float32)[m]
    if consensus is None:
        indptr, mz, intensity, rows = dataset.indptr, dataset.mz, dataset.intensity, m.to(torch.int32)
    else:
        indptr, mz, intensity = consensus
        rows = np.arange(len(m), dtype=np.int32)
        if len(indptr) != len(m) + 1:
            raise ValueError(f"consensus holds {len(indptr) - 1} spectra for {len(m)} clusters")
    l_pmz = ctx.to_dev(library.precursor_mz, torch.float32)
    l_rows = np.arange(int(l_pmz.numel()), dtype=np.int32)
    q, l, sim, matched = ctx.library_search(mz, intensity, indptr, rows, pmz, library.mz, library.intensity, library.indptr, l_rows,
                                            l_pmz, fragment_tol, precursor_tol, mode == "Da", analog, max_shift, min_cosine,
                                            min_matched_peaks, top_n)
    cols = dict(cluster=q, library=l, similarity=sim, matched=matched, delta_mz=pmz[q.long()] - l_pmz[l.long()])
    return {k: v.cpu().numpy() for k, v in cols.items()}


def network_families(network, n_clusters: int, max_size: int = 100, delta: float = 0.02,
                     pipeline: Optional[ClusterPipeline] = None):
    """Molecular families of the network `representative_network` returned for `n_clusters` clusters (`fal_network_families`;
    DESIGN.md "Molecular families"): the connected components of its links.  While a component has more than `max_size`
    clusters (0: no cap), a round cuts those of its links whose similarity is within `delta` of its weakest link's.

    Returns the same dict restricted to the surviving links, in their order, as host arrays, plus `family` int32 (per surviving
    link, the family of its two clusters), `node_family` int32 (per cluster; families are numbered by their smallest cluster,
    -1: the cluster has no surviving link), `node_size` int32 (per cluster, the clusters of its family; 1 without one),
    `n_families`, `n_rounds` and `n_cut` (the links cut)."""
    global _default_pipeline
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    ctx = pipe.ctx
    import torch
    types = dict(a=torch.int32, b=torch.int32, similarity=torch.float32, matched=torch.int32, delta_mz=torch.float32)
    cols = {k: ctx.to_dev(network[k], t) for k, t in types.items()}
    family, size, edge_round, n_families, n_rounds = ctx.network_families(cols["a"], cols["b"], cols["similarity"], n_clusters,
                                                                          max_size, delta)
    n_cut = ctx.counter(13)
    keep = edge_round == 0
    out = {k: v[keep].cpu().numpy() for k, v in cols.items()}
    out["family"] = family[cols["a"][keep].long()].cpu().numpy()
    out.update(node_family=family.cpu().numpy(), node_size=size.cpu().numpy(), n_families=n_families, n_rounds=n_rounds,
               n_cut=n_cut)
    return out


def propagate_annotations(families, hits, n_clusters: int, max_hops: int = 3, min_score: float = 0.0,
                          pipeline: Optional[ClusterPipeline] = None):
    """The library's names carried through the molecular families (`fal_network_propagate`; DESIGN.md "Annotation propagation").
    `families` is the dict `network_families` returned for `n_clusters` clusters (its `a`, `b`, `similarity`: the surviving
    links), `hits` the dict `library_search` returned for the same clusters.  A cluster with a hit is annotated by its rank-1
    hit, the first entry of its run in `hits`.  From the annotated clusters the walk goes level by level, at most `max_hops`
    links far: a link offers its unreached end the other end's score times the link's similarity (an annotated cluster scores
    1), offers below `min_score` do not count, a cluster takes the greatest offer, of equal ones the lowest cluster's.

    Returns host arrays over the clusters that are annotated or reached, in ascending cluster order: `cluster` int32, `hops`
    int32 (0: annotated itself), `source` int32 (the annotated cluster the name comes from), `via` int32 (the cluster that
    handed it on, -1 at hops 0), `score` float32 (the product of the similarities along the path), `hit` int32 (the index into
    `hits` of the source's rank-1 entry); and `n_seeds`, `n_reached`, `n_levels`."""
    global _default_pipeline
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    ctx = pipe.ctx
    n = int(n_clusters)
    hit_cluster = np.asarray(hits["cluster"], np.int64)
    if len(hit_cluster) and not (0 <= hit_cluster.min() and hit_cluster.max() < n):
        raise ValueError(f"propagate_annotations: a hit of a cluster outside the {n} clusters")
    first = np.flatnonzero(np.r_[True, hit_cluster[1:] != hit_cluster[:-1]]) if len(hit_cluster) else np.zeros(0, np.int64)
    seed = np.full(n, -1, np.int32)
    seed[hit_cluster[first][::-1]] = first[::-1].astype(np.int32)          # (a cluster with two runs keeps the first)
    source, hops, parent, score, n_reached, n_levels = ctx.network_propagate(families["a"], families["b"], families["similarity"], n,
                                                                             seed, max_hops, min_score)
    source, hops = source.cpu().numpy(), hops.cpu().numpy()
    rows = np.flatnonzero(hops >= 0)
    return dict(cluster=rows.astype(np.int32), hops=hops[rows], source=source[rows], via=parent.cpu().numpy()[rows],
                score=score.cpu().numpy()[rows], hit=seed[source[rows]], n_seeds=int((seed >= 0).sum()), n_reached=n_reached,
                n_levels=n_levels)


def write_representatives(filename: str, dataset: SpectrumDataset, medoids, cluster_ids, identifiers, charge: int = 0,
                          consensus=None, pipeline: Optional[ClusterPipeline] = None) -> str:
    """Write the representatives of `dataset`'s clusters to the MGF file `filename`, formatted on the device
    (`fal_mgf_write_sizes` / `fal_mgf_write`; DESIGN.md "MGF out of the device"): byte for byte the file
    `ms_io.write_spectra` writes for the same entries.  Entry c carries the peaks of row medoids[c] -- or, with `consensus`
    (indptr, mz, intensity as `consensus_spectra` returns them), the consensus peaks of cluster c -- the precursor m/z and
    retention time of row medoids[c], TITLE=identifiers[c] (a str array, one per cluster), CLUSTER=cluster_ids[c] and, unless
    `charge` is 0, CHARGE=`charge`.  -> "device", or "host" where the titles are outside what the device path mirrors
    (`mgf_io.title_blob`) and the host writer wrote the file."""
    global _default_pipeline
    from ..ms_io import ms_io
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    if dataset.retention_time is None:
        raise ValueError("write_representatives: the dataset has no retention times")
    ctx = pipe.ctx
    import torch
    m = ctx.to_dev(medoids, torch.int64)
    n = int(m.shape[0])
    if consensus is None:
        indptr, mz, intensity, rows = dataset.indptr, dataset.mz, dataset.intensity, m.to(torch.int32)
    else:
        indptr, mz, intensity = consensus
        rows = np.arange(n, dtype=np.int32)
    pmz, rt = ctx.to_dev(dataset.precursor_mz, torch.float32)[m], ctx.to_dev(dataset.retention_time, torch.float32)[m]
    return ms_io.write_representatives(filename, ctx, mz, intensity, indptr, rows, pmz, rt, np.full(n, int(charge), np.int32),
                                       cluster_ids, np.asarray(identifiers, dtype=str))


def assign_to_library(queries: SpectrumDataset, library: SpectrumDataset, eps: float, precursor_tol: float, mode: str,
                      rt_tol: Optional[float], fragment_tol: float, min_matched_peaks: int,
                      pipeline: Optional[ClusterPipeline] = None):
    """Nearest representative of every spectrum of `queries` among the spectra of `library` (one precursor charge; both
    preprocessed): `fal_assign_nearest` (DESIGN.md "Assigning to representatives").  A library row is a candidate when it passes
    the neighbour filter's precursor (and RT) test with the new spectrum in the query role; the winner minimises (float32
    matched-peak cosine distance, library precursor m/z, library row).  A spectrum is assigned when it has a candidate and
    float32(best_dist) <= float32(eps) -- the comparison DBSCAN makes.

    Returns (best_row int32[nq] library row or -1, best_dist float32[nq] (1.0 without a candidate), n_cand int32[nq],
    assigned bool[nq])."""
    global _default_pipeline
    pipe = pipeline or _default_pipeline
    if pipe is None:
        pipe = _default_pipeline = ClusterPipeline()
    if mode not in ("ppm", "Da"):
        raise ValueError(f"unknown precursor tolerance mode {mode!r} (ppm or Da)")
    row, dist, cand = pipe.ctx.assign_nearest(queries.mz, queries.intensity, queries.indptr, queries.precursor_mz,
                                              queries.retention_time, library.mz, library.intensity, library.indptr,
                                              library.precursor_mz, library.retention_time, precursor_tol, mode, rt_tol,
                                              fragment_tol, min_matched_peaks)
    row, dist, cand = row.cpu().numpy(), dist.cpu().numpy(), cand.cpu().numpy()
    return row, dist, cand, (row >= 0) & (dist <= np.float32(eps))
