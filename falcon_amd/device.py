"""Thin host wrapper over the C ABI: one `Context` per GPU.

PyTorch is used for plumbing only -- device memory (`torch.empty(..., device=cuda)`),
the stream the library enqueues on, and `torch.distributed` for the multi-GPU
exchange.  Every kernel that touches the data is in libfalcon_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import FalconHipError, check


def _torch():
    import torch
    return torch


def chunk_cuts(offsets, max_bytes) -> list:
    """The cuts [0, ..., n] of the text writers' chunks over n units with the ascending byte offsets `offsets` (n + 1): a chunk
    takes the units that stay within `max_bytes` (at least 1) of its first, and at least one: a larger unit grows its own."""
    n = len(offsets) - 1
    cuts = [0]
    while cuts[-1] < n:
        last = int(np.searchsorted(offsets, offsets[cuts[-1]] + max(int(max_bytes), 1), side="right")) - 1
        cuts.append(min(max(last, cuts[-1] + 1), n))
    return cuts


class Context:
    """Owns a `fal_ctx` bound to `cuda:<device>` and torch's current stream on it."""

    def __init__(self, device: int = 0):
        torch = _torch()
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise FalconHipError("no HIP device visible to torch; falcon_amd has no CPU fallback")
        self.device = int(device)
        self.tdev = torch.device("cuda", self.device)
        torch.cuda.set_device(self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        h = C.c_void_p()
        check(self.lib.fal_ctx_create(self.device, C.c_void_p(stream), 0, C.byref(h)), "fal_ctx_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.fal_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    h2d_bytes = 0            # bytes this context has copied host -> device through `to_dev` (the multi-GPU tests count them)

    def to_dev(self, a, dtype=None):
        torch = _torch()
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                self.h2d_bytes += a.numel() * a.element_size()
            t = a.to(self.tdev, non_blocking=True)
            return t.to(dtype).contiguous() if dtype is not None else t.contiguous()
        t = torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None:
            t = t.to(dtype)
        self.h2d_bytes += t.numel() * t.element_size()
        return t.to(self.tdev)

    def empty(self, shape, dtype):
        return _torch().empty(shape, dtype=dtype, device=self.tdev)

    @staticmethod
    def _p(t):
        return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())

    def sync(self):
        check(self.lib.fal_ctx_sync(self._h), "fal_ctx_sync")

    def plan(self, n: int, low_dim: int = 400, k_ann: int = 128, n_probe: int = 16, batch_size: int = 2 ** 15):
        """`fal_ctx_plan`: load every kernel's code object and size the shape-dependent scratch before the first pass"""
        check(self.lib.fal_ctx_plan(self._h, int(n), int(low_dim), int(k_ann), int(n_probe), int(batch_size)), "fal_ctx_plan")

    def trim(self):
        """`fal_ctx_trim`: give the context's cached device memory back to the driver (drains the stream)"""
        check(self.lib.fal_ctx_trim(self._h), "fal_ctx_trim")

    def enable_timing(self, on: bool = True):
        check(self.lib.fal_ctx_enable_timing(self._h, int(on)))

    def stage_ms(self, stage: str):
        ms, k = C.c_float(), C.c_int64()
        check(self.lib.fal_ctx_stage_ms(self._h, _lib.STAGES[stage], C.byref(ms), C.byref(k)))
        return ms.value, k.value

    def counter(self, which: int) -> int:
        v = C.c_int64()
        check(self.lib.fal_ctx_counter(self._h, int(which), C.byref(v)))
        return int(v.value)

    # ------------------------------------------------------------------ a2 / a3
    def to_vector_indices(self, mz, min_mz: float, bin_size: float):
        torch = _torch()
        mz = self.to_dev(mz, torch.float32)
        out = self.empty((mz.numel(),), torch.int32)
        check(self.lib.fal_to_vector_indices(self._h, self._p(mz), mz.numel(), min_mz, bin_size, self._p(out)),
              "fal_to_vector_indices")
        return out

    def vectorize(self, mz, intensity, indptr, row_order, min_mz: float, bin_size: float, n_bins: int,
                  low_dim: int, seed: int = 0, normalize: bool = True, dtype: str = "f32", width: Optional[int] = None):
        """a2 + a3 (`fal_vectorize_rows`).  `low_dim` = the hash modulus (any integer >= 1, README.md:114-117); `width` =
        columns of an output row (default: low_dim, which then has to be a multiple of 8; `row_width(low_dim)` = the width
        the path uses): the columns behind low_dim are zero and change no similarity."""
        torch = _torch()
        mz = self.to_dev(mz, torch.float32)
        intensity = self.to_dev(intensity, torch.float32)
        indptr = self.to_dev(indptr, torch.int64)
        row_order = None if row_order is None else self.to_dev(row_order, torch.int64)
        # output row i is spectrum row_order[i] of the CSR: a subset / permutation of the dataset is fine
        n = indptr.numel() - 1 if row_order is None else row_order.numel()
        w = int(low_dim if width is None else width)
        out2 = None
        if dtype in ("f32+f16", "f16+image"):
            # one pass over the peaks, two outputs: float32 rows and their float16 rounding ("f16+image": float16 VECTORS --
            # the float32 output is the image of the rounded values)
            out, out2 = self.empty((n, w), torch.float32), self.empty((n, w), torch.float16)
            code = _lib.FAL_OUT_F32_F16 if dtype == "f32+f16" else _lib.FAL_OUT_F16_IMAGE
        elif dtype == "split16":
            out, code = self.empty((n, 2, w), torch.float16), _lib.FAL_DTYPE_SPLIT16
        elif dtype in ("f16", "float16"):
            out, code = self.empty((n, w), torch.float16), _lib.FAL_DTYPE_F16
        else:
            out, code = self.empty((n, w), torch.float32), _lib.FAL_DTYPE_F32
        check(self.lib.fal_vectorize_rows(self._h, self._p(mz), self._p(intensity), self._p(indptr), self._p(row_order),
                                          n, float(min_mz), float(bin_size), int(n_bins), int(low_dim), w, int(seed),
                                          int(normalize), code, self._p(out), self._p(out2)), "fal_vectorize_rows")
        return out if out2 is None else (out, out2)


    # ------------------------------------------------------------------ a6 / a7
    def ivf_build(self, X, bucket_off: np.ndarray, n_list: np.ndarray, kmeans_iters: int = 10,
                  X16=None, Xpre=None, Xkm=None, prefilter_which: int = 1) -> "IvfIndex":
        """X: float32 [n, d] (may be None when every bucket is flat and X16 is given);
        X16: optional float16 [n, d] (plain rows) or [n, 2, d] (hi/lo split) for the f16 flat scan;
        Xpre: optional float16 [n, d] copy of X used only as the prefilter of `search_neighbors` (exact results);
        prefilter_which: where Xpre is used: 1 = flat buckets (fused.hip), 2 = buckets with an index (ivf16.hip), 3 = both;
        Xkm: optional float16 [n, d] copy of X used as the prefilter of the k-means assignment (identical index)."""
        torch = _torch()
        if X is not None:
            assert X.dtype == torch.float32 and X.is_contiguous() and X.device == self.tdev
            n, d = X.shape
        else:
            assert X16 is not None
            n, d = X16.shape[0], X16.shape[-1]
        bo = np.ascontiguousarray(bucket_off, np.int64)
        nl = np.ascontiguousarray(n_list, np.int32)
        h = C.c_void_p()
        if Xkm is not None:
            assert Xkm.dtype == torch.float16 and Xkm.is_contiguous() and Xkm.device == self.tdev and tuple(Xkm.shape) == (n, d)
        check(self.lib.fal_ivf_build_x16(self._h, self._p(X), self._p(Xkm), n, d, bo.ctypes.data_as(C.c_void_p), len(nl),
                                         nl.ctypes.data_as(C.c_void_p), int(kmeans_iters), C.byref(h)), "fal_ivf_build")
        index = IvfIndex(self, h, X, bo, nl, n, d)
        index.Xkm = Xkm
        if X16 is not None:
            assert X16.dtype == torch.float16 and X16.is_contiguous() and X16.device == self.tdev
            planes = 2 if X16.dim() == 3 else 1
            check(self.lib.fal_ivf_attach_f16(h, self._p(X16), planes), "fal_ivf_attach_f16")
            index.X16 = X16
        if Xpre is not None:
            assert Xpre.dtype == torch.float16 and Xpre.is_contiguous() and Xpre.device == self.tdev and Xpre.shape == (n, d)
            check(self.lib.fal_ivf_attach_prefilter_ex(h, self._p(Xpre), int(prefilter_which)), "fal_ivf_attach_prefilter_ex")
            index.Xpre = Xpre
        return index


    # ------------------------------------------------------------------ sort / a5
    def sort_by_precursor(self, precursor_mz):
        """stable sort (reference cluster.py:73-85) -> order i64[n], mz_sorted f32[n]"""
        torch = _torch()
        pmz = self.to_dev(precursor_mz, torch.float32)
        n = pmz.numel()
        order = self.empty((n,), torch.int64)
        mzs = self.empty((n,), torch.float32)
        check(self.lib.fal_sort_by_precursor(self._h, self._p(pmz), n, self._p(order), self._p(mzs)),
              "fal_sort_by_precursor")
        return order, mzs

    def gather_f32(self, src, order):
        torch = _torch()
        src = self.to_dev(src, torch.float32)
        out = self.empty((order.numel(),), torch.float32)
        check(self.lib.fal_gather_f32(self._h, self._p(src), self._p(order), order.numel(), self._p(out)),
              "fal_gather_f32")
        return out

    N_WINDOWS = 1 << 14           # deal units the multi-GPU front end counts: window w = floor(mz / mz_interval) -> slot w mod 16,384

    def window_counts(self, precursor_mzs, mz_interval: float):
        """spectra per precursor window floor(mz / mz_interval) of every partition of a job (`fal_window_counts`: one pair of
        launches, one copy to pinned host memory, one wait) -> int64 counts [n_parts, windows] (host), the all-zero trailing
        windows cut"""
        torch = _torch()
        pmz = [self.to_dev(x, torch.float32) for x in precursor_mzs]
        n_parts = len(pmz)
        if n_parts == 0:
            return np.zeros((0, 0), np.int64)
        counts = self.empty((n_parts, self.N_WINDOWS), torch.int32)
        if getattr(self, "_wc_host", None) is None or self._wc_host.numel() < n_parts * (self.N_WINDOWS + 2):
            self._wc_host = torch.empty(n_parts * (self.N_WINDOWS + 2), dtype=torch.int32, pin_memory=True)
        host = self._wc_host
        ptrs = (C.c_void_p * n_parts)(*[x.data_ptr() if x.numel() else None for x in pmz])
        ns = (C.c_int64 * n_parts)(*[x.numel() for x in pmz])
        check(self.lib.fal_window_counts(self._h, ptrs, ns, n_parts, float(mz_interval), self.N_WINDOWS, self._p(counts),
                                         C.c_void_p(host.data_ptr())), "fal_window_counts")
        self.sync()
        h = host.numpy()
        last = h[n_parts * self.N_WINDOWS: n_parts * (self.N_WINDOWS + 2)].reshape(n_parts, 2)
        last = last[last[:, 0] <= last[:, 1], 1]                                  # (empty partitions: INT32_MAX, 0)
        width = int(last.max()) + 1 if len(last) else 0
        return h[: n_parts * self.N_WINDOWS].reshape(n_parts, self.N_WINDOWS)[:, :width].astype(np.int64)

    def window_select(self, precursor_mz, mz_interval: float, owner: np.ndarray, rank: int):
        """the spectra whose window is dealt to `rank` (`fal_window_select`) -> rows i64[m] (ascending dataset rows), mz f32[m]"""
        torch = _torch()
        pmz = self.to_dev(precursor_mz, torch.float32)
        n = pmz.numel()
        own = np.full(self.N_WINDOWS, -1, np.int32)
        own[:len(owner)] = owner
        if len(owner):
            own[len(owner):] = owner[-1]                  # (slots behind the counted ones hold no spectrum)
        own_d = self.to_dev(own, torch.int32)
        rows = self.empty((max(n, 1),), torch.int64)
        mzs = self.empty((max(n, 1),), torch.float32)
        m = C.c_int64()
        check(self.lib.fal_window_select(self._h, self._p(pmz), n, float(mz_interval), self.N_WINDOWS, self._p(own_d), int(rank),
                                         self._p(rows), self._p(mzs), C.byref(m)), "fal_window_select")
        return rows[: m.value], mzs[: m.value]

    def precursor_splits(self, mz_sorted, tol: float, mode: str, batch_size: int, mz_interval: float = 1.0,
                         chunk_last: bool = True) -> np.ndarray:
        """reference cluster.py:159-209 (+ the build's two extra rules) -> int64 boundaries (host)"""
        torch = _torch()
        mzs = self.to_dev(mz_sorted, torch.float32)
        n = mzs.numel()
        cap = n + 2
        out = np.empty(cap, np.int64)
        k = C.c_int64()
        check(self.lib.fal_precursor_splits(self._h, self._p(mzs), n, float(tol), int(mode == "Da"), int(batch_size),
                                            float(mz_interval or 0.0), int(chunk_last),
                                            out.ctypes.data_as(C.c_void_p), cap, C.byref(k)), "fal_precursor_splits")
        return out[:k.value].copy()

    # ------------------------------------------------------------------ a8 .. a12
    def filter_neighbors(self, sim, idx, mz_sorted, rt_sorted, tol: float, mode: str, rt_tol, n_neighbors: int):
        torch = _torch()
        n, k_ann = idx.shape
        nb_idx = self.empty((n, n_neighbors), torch.int32)
        nb_dist = self.empty((n, n_neighbors), torch.float32)
        check(self.lib.fal_filter_neighbors(self._h, self._p(sim), self._p(idx), n, k_ann, self._p(mz_sorted),
                                            self._p(rt_sorted), float(tol), int(mode == "Da"),
                                            -1.0 if rt_tol is None else float(rt_tol), int(n_neighbors),
                                            self._p(nb_idx), self._p(nb_dist)), "fal_filter_neighbors")
        return nb_idx, nb_dist

    SCALING = {None: 0, "off": 0, "root": 1, "log": 2, "rank": 3}

    def process_spectra(self, mz, intensity, indptr, precursor_mz, precursor_charge, min_peaks: int,
                        min_mz_range: float, mz_min=None, mz_max=None, remove_precursor_tolerance=None,
                        min_intensity=None, max_peaks_used=None, scaling=None):
        """f1 (`fal_process_spectra`): batch `process_spectrum` (reference spectrum.py:73-169) over raw CSR peaks
        (mz float64 sorted per spectrum, intensity float32, charge 0 = unknown).
        -> valid bool[n], out_indptr i64[n+1], out_mz f32[nnz_out], out_intensity f32[nnz_out] (device tensors)."""
        torch = _torch()
        mz = self.to_dev(mz, torch.float64)
        intensity = self.to_dev(intensity, torch.float32)
        indptr = self.to_dev(indptr, torch.int64)
        pmz = self.to_dev(precursor_mz, torch.float64)
        charge = self.to_dev(precursor_charge, torch.int32)
        n, nnz = indptr.numel() - 1, mz.numel()
        if scaling not in self.SCALING:
            raise ValueError(f"unknown scaling {scaling!r}")
        valid = self.empty((n,), torch.int32)
        out_indptr = self.empty((n + 1,), torch.int64)
        out_mz = self.empty((max(nnz, 1),), torch.float32)
        out_it = self.empty((max(nnz, 1),), torch.float32)
        nan = float("nan")
        check(self.lib.fal_process_spectra(
            self._h, self._p(mz), self._p(intensity), self._p(indptr), n, nnz, self._p(pmz), self._p(charge),
            int(min_peaks), float(min_mz_range), nan if mz_min is None else float(mz_min),
            nan if mz_max is None else float(mz_max),
            -1.0 if remove_precursor_tolerance is None else float(remove_precursor_tolerance),
            -1.0 if min_intensity is None else float(min_intensity), 0 if max_peaks_used is None else int(max_peaks_used),
            self.SCALING[scaling], self._p(valid), self._p(out_indptr), self._p(out_mz), self._p(out_it)),
            "fal_process_spectra")
        nnz_out = int(out_indptr[-1].item())
        return valid.bool(), out_indptr, out_mz[:nnz_out], out_it[:nnz_out]

    def decode_peaks(self, payload, arrays, spectra):
        """`fal_decode_peaks`: the binary arrays of mzML / mzXML spectra -> the raw CSR `process_spectra` takes, on the device.
        payload u8[] (base64 text, arrays at 8-byte aligned offsets), arrays i64[n_arrays, 4] (offset, base64 length, declared
        count, `_lib.PEAK_*` flags: float width, zlib, byte order, pairs, or an MS-Numpress codec), spectra i64[n, 2] (m/z array,
        intensity array).
        -> indptr i64[n+1], mz f64[nnz], intensity f32[nnz] (sorted by m/z per spectrum, as falcon._raw_csr), status i32[n]
        (0 = decoded; else `_lib.PEAK_STATUS` bits, and that spectrum's peaks are zeros).  Device tensors; no sync."""
        torch = _torch()
        arrays = np.ascontiguousarray(arrays, np.int64).reshape(-1, 4)
        spectra = np.ascontiguousarray(spectra, np.int64).reshape(-1, 2)
        payload = np.frombuffer(payload, np.uint8) if isinstance(payload, (bytes, bytearray, memoryview)) else payload
        n = len(spectra)
        # sizes from the host copy of the tables (the kernels check every slot against them)
        flags, counts = arrays[:, 3], arrays[:, 2]
        # inflate_bytes (falcon_hip.h): per array, 8-byte rounded, the inflated capacity of a zlib array -- the declared size,
        # or the longest MS-Numpress stream of the count -- plus count x 8 for the float64 values of a numpress array
        cnt = np.maximum(counts, 0)
        codec = flags & _lib.PEAK_NUMPRESS_MASK
        nbytes = cnt * np.where(flags & _lib.PEAK_F64, 8, 4) * np.where(flags & _lib.PEAK_PAIRS, 2, 1)
        linear = np.where(cnt == 0, 8, np.where(cnt == 1, 12, 16 + (9 * (cnt - 2) + 1) // 2))
        nbytes = np.select([codec == _lib.PEAK_NUMPRESS_LINEAR, codec == _lib.PEAK_NUMPRESS_PIC,
                            codec == _lib.PEAK_NUMPRESS_SLOF], [linear, (9 * cnt + 1) // 2, 8 + 2 * cnt], nbytes)
        inflate_bytes = int(((nbytes + 7) // 8 * 8)[(flags & _lib.PEAK_ZLIB) != 0].sum() + (cnt * 8)[codec != 0].sum())
        ma = spectra[:, 0]
        ok = (ma >= 0) & (ma < len(arrays))
        nnz = int(np.maximum(counts[ma[ok]], 0).sum()) if len(arrays) else 0
        indptr = self.empty((n + 1,), torch.int64)
        mz = self.empty((max(nnz, 1),), torch.float64)
        it = self.empty((max(nnz, 1),), torch.float32)
        status = self.empty((max(n, 1),), torch.int32)
        d_payload = self.to_dev(payload, torch.uint8) if len(payload) else None
        d_arrays = self.to_dev(arrays) if len(arrays) else None
        d_spectra = self.to_dev(spectra) if n else None
        check(self.lib.fal_decode_peaks(self._h, self._p(d_payload), len(payload), self._p(d_arrays), len(arrays),
                                        self._p(d_spectra), n, inflate_bytes, nnz, self._p(indptr), self._p(mz), self._p(it),
                                        self._p(status)), "fal_decode_peaks")
        return indptr, mz[:nnz], it[:nnz], status[:n]

    def _text_to_dev(self, text):
        """bytes, bytearray, memoryview, uint8 array or uint8 tensor -> uint8 device tensor"""
        torch = _torch()
        if isinstance(text, torch.Tensor):
            return self.to_dev(text, torch.uint8)
        raw = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.asarray(text, np.uint8)
        if not raw.flags.writeable:
            raw = raw.copy()                     # (immutable bytes: torch takes writable arrays only)
        return self.to_dev(raw) if len(raw) else self.empty((0,), torch.uint8)

    def _text_index(self, name, d_text):
        """`fal_mgf_index` / `fal_mzml_index` (`name`) of a uint8 device tensor -> its four counts"""
        counts = (C.c_int64 * 4)()
        check(getattr(self.lib, name)(self._h, self._p(d_text) if d_text.numel() else None, d_text.numel(), counts), name)
        return tuple(int(c) for c in counts)

    def mgf_index(self, d_text):
        """`fal_mgf_index` of MGF text on the device (uint8 tensor) -> (spectra, peaks, `_lib.MGF_FLAG_*` bits, lines).
        Synchronises once.  The tables stay in the context for the `mgf_parse` of the same tensor."""
        return self._text_index("fal_mgf_index", d_text)

    def mgf_parse(self, d_text, n: int, nnz: int, optional_keys: int = 0):
        """`fal_mgf_parse` (`fal_mgf_parse_ex` with `optional_keys`, `_lib.MGF_OPT_*` bits) behind `mgf_index` of the same tensor
        -> device tensors indptr i64[n+1], mz f64[nnz], intensity f32[nnz], precursor_mz f64[n], charge i32[n], has_charge
        i32[n], retention_time f64[n], title i64[n, 2], span i64[n, 2], status i32[n].  No sync."""
        torch = _torch()
        m = max(n, 1)
        indptr, mz, it = self.empty((n + 1,), torch.int64), self.empty((max(nnz, 1),), torch.float64), self.empty((max(nnz, 1),), torch.float32)
        pmz, rt = self.empty((m,), torch.float64), self.empty((m,), torch.float64)
        charge, has_charge, status = (self.empty((m,), torch.int32) for _ in range(3))
        title, span = self.empty((m, 2), torch.int64), self.empty((m, 2), torch.int64)
        args = (self._h, self._p(d_text) if d_text.numel() else None, d_text.numel(), n, nnz, self._p(indptr), self._p(mz), self._p(it),
                self._p(pmz), self._p(charge), self._p(has_charge), self._p(rt), self._p(title), self._p(span), self._p(status))
        if optional_keys:
            check(self.lib.fal_mgf_parse_ex(*args, optional_keys), "fal_mgf_parse_ex")
        else:
            check(self.lib.fal_mgf_parse(*args), "fal_mgf_parse")
        return indptr, mz[:nnz], it[:nnz], pmz[:n], charge[:n], has_charge[:n], rt[:n], title[:n], span[:n], status[:n]

    def mgf_headers(self, d_text, n: int, keys):
        """`fal_mgf_headers` behind `mgf_index` of the same tensor.  `keys`: lower-case header keys (at most `_lib.MGF_MAX_KEYS`),
        a sequence of names (byte ranges only) or a dict name -> `_lib.MGF_KEY_SPAN` / `_lib.MGF_KEY_INT`
        -> device tensors span i64[n, k, 2] (the stripped value of the spectrum's last line of that key), value i64[n, k] (the
        integer of a decided INT key), state i32[n, k] (`_lib.MGF_KEY_ABSENT` / `PRESENT` / `HOST`).  No sync."""
        return self._text_headers("fal_mgf_headers", d_text, n, keys)

    def _text_headers(self, name, d_text, n: int, keys):
        """`fal_mgf_headers` / `fal_msp_headers` (`name`): the key table packed, the outputs allocated"""
        torch = _torch()
        kinds = np.array([keys[k] for k in keys] if isinstance(keys, dict) else [0] * len(keys), np.int32)
        raw = [str(k).encode("utf-8") for k in keys]
        ptr = np.zeros(len(raw) + 1, np.int64)
        np.cumsum([len(r) for r in raw], out=ptr[1:])
        blob = np.frombuffer(b"".join(raw) + b"\0", np.uint8)
        k, m = len(raw), max(n, 1)
        span, value = self.empty((m, max(k, 1), 2), torch.int64), self.empty((m, max(k, 1)), torch.int64)
        state = self.empty((m, max(k, 1)), torch.int32)
        as_p = lambda a: a.ctypes.data_as(C.c_void_p)                             # noqa: E731
        check(getattr(self.lib, name)(self._h, self._p(d_text) if d_text.numel() else None, d_text.numel(), n, as_p(blob), as_p(ptr),
                                      as_p(kinds) if k else None, k, self._p(span), self._p(value), self._p(state)), name)
        return span[:n], value[:n], state[:n]

    def text_rows(self, d_text, span, column: int = 0, width: int = 256):
        """`fal_text_rows`: the byte ranges span[:, column] (i64 device tensor [n, 2] or [n, k, 2]) of the text as rows of `width`
        bytes, zero-padded -> device tensors rows u8[n, width], long i32[n] (1: the range is longer than the row).  Synchronises
        once; a range outside the text raises."""
        torch = _torch()
        span = self.to_dev(span, torch.int64)
        n = int(span.shape[0])
        stride = int(span.shape[1]) if span.dim() == 3 else 1
        rows, long = self.empty((max(n, 1), width), torch.uint8), self.empty((max(n, 1),), torch.int32)
        check(self.lib.fal_text_rows(self._h, self._p(d_text) if d_text.numel() else None, d_text.numel(), self._p(span), stride, column,
                                     n, width, self._p(rows), self._p(long)), "fal_text_rows")
        return rows[:n], long[:n]

    def parse_mgf(self, text, optional_title: bool = False, keys=None):
        """MGF text (bytes, uint8 array or uint8 device tensor) -> dict: `flags` (`_lib.MGF_FLAG_*`; non-zero: the text is the
        host reader's and nothing else is set), else the raw CSR on the device -- `indptr` i64[n+1], `mz` f64, `intensity` f32,
        sorted by m/z inside every spectrum as falcon._raw_csr -- and the per-spectrum host columns `precursor_mz` f64,
        `charge` i32, `has_charge` bool, `retention_time` f64 (-1 when absent), `title` / `span` i64[n, 2] (byte ranges of the
        title value and of the spectrum), `status` i32 (0, or `_lib.MGF_ST_HOST`: the host reader decides that spectrum; its
        slot has the right size and placeholder values).  `optional_title`: a spectrum without TITLE is not HOST on that
        account (its title range is (0, 0)).  `keys` (see `mgf_headers`) adds `key_span` (device, i64[n, k, 2]) and the host
        columns `key_value` i64[n, k], `key_state` i32[n, k], and `text`, the device tensor the ranges refer to (for
        `text_rows`).  DESIGN.md "MGF on the device" states the grammar."""
        from ._lib import MGF_OPT_TITLE
        d_text = self._text_to_dev(text)
        n, nnz, flags, lines = self.mgf_index(d_text)
        if flags:
            return dict(flags=flags, lines=lines)
        indptr, mz, it, *cols = self.mgf_parse(d_text, n, nnz, MGF_OPT_TITLE if optional_title else 0)
        extra = {}
        if keys is not None:
            key_span, value, state = self.mgf_headers(d_text, n, keys)
            extra = dict(key_span=key_span, key_value=value.cpu().numpy(), key_state=state.cpu().numpy(), text=d_text)
        pmz, charge, has_charge, rt, title, span, status = (c.cpu().numpy() for c in cols)
        return dict(flags=0, lines=lines, indptr=indptr, mz=mz, intensity=it, precursor_mz=pmz, charge=charge,
                    has_charge=has_charge.astype(bool), retention_time=rt, title=title, span=span, status=status, **extra)

    def msp_index(self, d_text):
        """`fal_msp_index` of MSP text on the device (uint8 tensor) -> (entries, peaks, `_lib.MGF_FLAG_*` bits, lines).
        Synchronises once.  The tables stay in the context -- beside an MGF index's -- for the `msp_parse` of the same tensor."""
        return self._text_index("fal_msp_index", d_text)

    def msp_parse(self, d_text, n: int, nnz: int):
        """`fal_msp_parse` behind `msp_index` of the same tensor -> device tensors indptr i64[n+1], mz f64[nnz], intensity
        f32[nnz], precursor_mz f64[n], charge i32[n], has_charge i32[n], span i64[n, 2], status i32[n].  No sync."""
        torch = _torch()
        m = max(n, 1)
        indptr, mz, it = self.empty((n + 1,), torch.int64), self.empty((max(nnz, 1),), torch.float64), self.empty((max(nnz, 1),), torch.float32)
        pmz, span = self.empty((m,), torch.float64), self.empty((m, 2), torch.int64)
        charge, has_charge, status = (self.empty((m,), torch.int32) for _ in range(3))
        check(self.lib.fal_msp_parse(self._h, self._p(d_text) if d_text.numel() else None, d_text.numel(), n, nnz, self._p(indptr),
                                     self._p(mz), self._p(it), self._p(pmz), self._p(charge), self._p(has_charge), self._p(span),
                                     self._p(status)), "fal_msp_parse")
        return indptr, mz[:nnz], it[:nnz], pmz[:n], charge[:n], has_charge[:n], span[:n], status[:n]

    def msp_headers(self, d_text, n: int, keys):
        """`fal_msp_headers` behind `msp_index` of the same tensor: `mgf_headers` with ':' between key and value, over the lines
        from an entry's Name: line to its first Num Peaks line; a key may hold a space or '#' ("num peaks", "db#")."""
        return self._text_headers("fal_msp_headers", d_text, n, keys)

    def parse_msp(self, text, keys=None):
        """MSP library text (bytes, uint8 array or uint8 device tensor) -> dict: `flags` (`_lib.MGF_FLAG_*`; non-zero: the text
        is the host reader's and nothing else is set), else the raw CSR on the device -- `indptr` i64[n+1], `mz` f64,
        `intensity` f32, sorted by m/z inside every entry -- and the per-entry host columns `precursor_mz` f64, `charge` i32,
        `has_charge` bool, `span` i64[n, 2] (the entry's bytes), `status` i32 (0, or `_lib.MSP_ST_HOST`: the host reader decides
        that entry; its slot has the right size and placeholder values).  `keys` (see `msp_headers`) adds `key_span` (device,
        i64[n, k, 2]), the host columns `key_value` i64[n, k], `key_state` i32[n, k], and `text`, the device tensor the ranges
        refer to (for `text_rows`).  DESIGN.md "MSP on the device" states the grammar."""
        d_text = self._text_to_dev(text)
        n, nnz, flags, lines = self.msp_index(d_text)
        if flags:
            return dict(flags=flags, lines=lines)
        indptr, mz, it, *cols = self.msp_parse(d_text, n, nnz)
        extra = {}
        if keys is not None:
            key_span, value, state = self.msp_headers(d_text, n, keys)
            extra = dict(key_span=key_span, key_value=value.cpu().numpy(), key_state=state.cpu().numpy(), text=d_text)
        pmz, charge, has_charge, span, status = (c.cpu().numpy() for c in cols)
        return dict(flags=0, lines=lines, indptr=indptr, mz=mz, intensity=it, precursor_mz=pmz, charge=charge,
                    has_charge=has_charge.astype(bool), span=span, status=status, **extra)

    def _write_sizes(self, entry: str, args, n: int):
        """a text writer's sizing call `entry` over the packed columns `args`, n units -> (sizes i64[n], offsets i64[n + 1] on the
        device, total bytes)"""
        torch = _torch()
        sizes, offsets = self.empty((max(n, 1),), torch.int64), self.empty((n + 1,), torch.int64)
        total = C.c_int64(0)
        check(getattr(self.lib, entry)(self._h, *args, self._p(sizes), self._p(offsets), C.byref(total)), entry)
        return sizes[:n], offsets, int(total.value)

    def _write_range(self, entry: str, args, offsets, first: int, last: int, out, host_out):
        """a text writer's write call `entry` over the packed columns `args`: units [first, last) into `out`, copied to `host_out`"""
        if host_out is not None and (not host_out.is_pinned() or host_out.numel() != out.numel()):
            raise ValueError(f"{entry[4:]}: host_out must be pinned and of out's size")
        check(getattr(self.lib, entry)(self._h, *args, self._p(offsets), int(first), int(last), self._p(out) if out.numel() else None,
                                       out.numel(), self._p(host_out) if host_out is not None and out.numel() else None), entry)

    def _write_chunks(self, n: int, offsets, max_bytes, copy: bool, write):
        """units [0, n) cut at `chunk_cuts`, every chunk through `write(first, last, d_view, h_view)` -> its host array"""
        torch = _torch()
        if max_bytes is None:
            from .ms_io.mgf_io import DEFAULT_CHUNK_BYTES as max_bytes
        off = offsets.cpu().numpy()
        cuts = chunk_cuts(off[:n + 1], max_bytes)
        cap = int(max(off[b] - off[a] for a, b in zip(cuts[:-1], cuts[1:])))
        d_out = self.empty((max(cap, 1),), torch.uint8)
        h_out = torch.empty((max(cap, 1),), dtype=torch.uint8, pin_memory=True)
        for a, b in zip(cuts[:-1], cuts[1:]):
            need = int(off[b] - off[a])
            write(a, b, d_out[:need], h_out[:need])
            chunk = h_out[:need].numpy()
            yield chunk.copy() if copy else chunk

    def _mgf_entries(self, mz, intensity, indptr, rows, precursor_mz, retention_time, charge, cluster, title, title_ptr):
        """the writer's columns as device tensors of the entry points' types, checked against each other"""
        torch = _torch()
        cols = dict(mz=self.to_dev(mz, torch.float32), intensity=self.to_dev(intensity, torch.float32),
                    indptr=self.to_dev(indptr, torch.int64), rows=self.to_dev(rows, torch.int32),
                    precursor_mz=self.to_dev(precursor_mz, torch.float32), retention_time=self.to_dev(retention_time, torch.float32),
                    charge=self.to_dev(charge, torch.int32), cluster=self.to_dev(cluster, torch.int64),
                    title=self._text_to_dev(title), title_ptr=self.to_dev(title_ptr, torch.int64))
        n = int(cols["rows"].shape[0])
        for name in ("precursor_mz", "retention_time", "charge", "cluster"):
            if cols[name].shape[0] != n:
                raise ValueError(f"format_mgf: {name} has {cols[name].shape[0]} entries for {n} rows")
        if cols["title_ptr"].shape[0] != n + 1 or cols["indptr"].shape[0] < 1 or cols["mz"].shape != cols["intensity"].shape:
            raise ValueError("format_mgf: title_ptr needs one entry more than rows, indptr at least one, mz and intensity the same size")
        return cols

    def _mgf_entry_args(self, c, with_title: bool):
        head = [self._p(c["mz"]), self._p(c["intensity"]), self._p(c["indptr"]), c["indptr"].shape[0] - 1, c["mz"].shape[0],
                self._p(c["rows"]), c["rows"].shape[0], self._p(c["precursor_mz"]), self._p(c["retention_time"]), self._p(c["charge"]),
                self._p(c["cluster"])]
        return head + ([self._p(c["title"])] if with_title else []) + [self._p(c["title_ptr"]), c["title"].numel()]

    def mgf_write_sizes(self, cols):
        """`fal_mgf_write_sizes` of `_mgf_entries` columns -> (sizes i64[n], offsets i64[n + 1] on the device, total bytes).
        Synchronises once."""
        return self._write_sizes("fal_mgf_write_sizes", self._mgf_entry_args(cols, False), int(cols["rows"].shape[0]))

    def mgf_write(self, cols, offsets, first: int, last: int, out, host_out=None):
        """`fal_mgf_write`: the text of entries [first, last) into the uint8 device tensor (or view) `out`; `host_out`: a pinned
        uint8 host tensor of the same size that receives a copy.  Synchronises once.  FalconHipError (code `_lib.FAL_EINVAL`,
        nothing written) when `out` is too small."""
        self._write_range("fal_mgf_write", self._mgf_entry_args(cols, True), offsets, first, last, out, host_out)

    def format_mgf(self, mz, intensity, indptr, rows, precursor_mz, retention_time, charge, cluster, title, title_ptr,
                   max_bytes: Optional[int] = None, copy: bool = True):
        """The MGF text of n entries, byte for byte what `mgf_io.write_spectra` writes for them (DESIGN.md "MGF out of the
        device"), as a generator of uint8 host arrays that together are the file.  Peaks CSR mz / intensity f32, indptr i64;
        rows i32[n]: the CSR row of entry k (any order, repeats allowed); precursor_mz / retention_time f32[n], charge i32[n]
        (0: no CHARGE line), cluster i64[n]; title: the entries' encoded title bytes, title_ptr i64[n + 1] their offsets.
        Arrays or device tensors.  Chunks are cut on entry boundaries at about `max_bytes` (default
        `mgf_io.DEFAULT_CHUNK_BYTES`); one larger entry grows its chunk.  Every chunk is formatted into one device buffer and
        copied through one pinned host buffer, with one stream synchronisation; `copy=False` yields views of that pinned
        buffer, valid until the next chunk is asked for."""
        cols = self._mgf_entries(mz, intensity, indptr, rows, precursor_mz, retention_time, charge, cluster, title, title_ptr)
        n = int(cols["rows"].shape[0])
        if n == 0:
            return
        sizes, offsets, _ = self.mgf_write_sizes(cols)            # (sizes: alive until the last chunk, as the buffers are)
        yield from self._write_chunks(n, offsets, max_bytes, copy, lambda a, b, d, h: self.mgf_write(cols, offsets, a, b, d, h))

    def csv_order(self, file_rank, ident, id_ptr):
        """`fal_csv_order`: the rows of the cluster CSV sorted by (file_rank, natural order of the ASCII id, row) -> (order i32[n]
        on the device, the longest digit run in an id).  file_rank i32[n]; ident: the ids' bytes, id_ptr i64[n + 1] their offsets.
        Synchronises once.  FalconHipError (code `_lib.FAL_EINVAL`) when id_ptr does not ascend inside the blob."""
        torch = _torch()
        rank, ident, id_ptr = self.to_dev(file_rank, torch.int32), self._text_to_dev(ident), self.to_dev(id_ptr, torch.int64)
        n = int(rank.shape[0])
        if id_ptr.shape[0] != n + 1:
            raise ValueError("csv_order: id_ptr needs one entry more than file_rank")
        order = self.empty((max(n, 1),), torch.int32)
        longest = C.c_int64(0)
        check(self.lib.fal_csv_order(self._h, self._p(rank), self._p(ident) if ident.numel() else None, self._p(id_ptr), ident.numel(), n,
                                     self._p(order), C.byref(longest)), "fal_csv_order")
        return order[:n], int(longest.value)

    def _csv_columns(self, file_id, file_names, file_name_ptr, ident, id_ptr, charge, precursor_mz, retention_time, cluster, order=None,
                     quote_cr: Optional[bool] = None):
        """the CSV writer's columns as device tensors of the entry points' types, checked against each other"""
        torch = _torch()
        if quote_cr is None:
            from .ms_io.csv_io import host_quotes_cr
            quote_cr = host_quotes_cr()
        cols = dict(file_id=self.to_dev(file_id, torch.int32), fn=self._text_to_dev(file_names), fn_ptr=self.to_dev(file_name_ptr, torch.int64),
                    id=self._text_to_dev(ident), id_ptr=self.to_dev(id_ptr, torch.int64), charge=self.to_dev(charge, torch.int32),
                    precursor_mz=self.to_dev(precursor_mz, torch.float32), retention_time=self.to_dev(retention_time, torch.float32),
                    cluster=self.to_dev(cluster, torch.int64), order=None if order is None else self.to_dev(order, torch.int32),
                    quote_cr=int(bool(quote_cr)))
        n = int(cols["file_id"].shape[0])
        for name in ("charge", "precursor_mz", "retention_time", "cluster"):
            if cols[name].shape[0] != n:
                raise ValueError(f"format_csv: {name} has {cols[name].shape[0]} entries for {n} rows")
        if cols["id_ptr"].shape[0] != n + 1 or cols["fn_ptr"].shape[0] < 1:
            raise ValueError("format_csv: id_ptr needs one entry more than the rows, file_name_ptr at least one")
        cols["rows"] = n if order is None else int(cols["order"].shape[0])
        return cols

    def _csv_column_args(self, c):
        ptr = lambda t: self._p(t) if t is not None and t.numel() else None
        return [ptr(c["order"]), c["rows"], ptr(c["file_id"]), ptr(c["fn"]), self._p(c["fn_ptr"]), c["fn_ptr"].shape[0] - 1, c["fn"].numel(),
                ptr(c["id"]), self._p(c["id_ptr"]), c["id"].numel(), ptr(c["charge"]), ptr(c["precursor_mz"]), ptr(c["retention_time"]),
                ptr(c["cluster"]), c["file_id"].shape[0], c["quote_cr"]]

    def csv_write_sizes(self, cols):
        """`fal_csv_write_sizes` of `_csv_columns` columns -> (sizes i64[rows], offsets i64[rows + 1] on the device, total bytes).
        Synchronises once."""
        return self._write_sizes("fal_csv_write_sizes", self._csv_column_args(cols), cols["rows"])

    def csv_write(self, cols, offsets, first: int, last: int, out, host_out=None):
        """`fal_csv_write`: the text of rows [first, last) into the uint8 device tensor (or view) `out`; `host_out`: a pinned uint8
        host tensor of the same size that receives a copy.  Synchronises once.  FalconHipError (code `_lib.FAL_EINVAL`, nothing
        written) when `out` is too small."""
        self._write_range("fal_csv_write", self._csv_column_args(cols), offsets, first, last, out, host_out)

    def format_csv(self, file_id, file_names, file_name_ptr, ident, id_ptr, charge, precursor_mz, retention_time, cluster, order=None,
                   max_bytes: Optional[int] = None, copy: bool = True, quote_cr: Optional[bool] = None):
        """The rows of the cluster CSV, byte for byte what `falcon._write_cluster_info` writes below its header (DESIGN.md "Cluster
        CSV out of the device"), as a generator of uint8 host arrays that together are the rows.  file_id i32[n] into the names
        `file_names` (their encoded bytes) / `file_name_ptr` i64[files + 1]; ident / id_ptr i64[n + 1]: the spectrum ids; charge
        i32[n] (0: None), precursor_mz / retention_time f32[n], cluster i64[n]; order i32: text row k is input row order[k] (what
        `csv_order` gives; None: the rows as they are).  Arrays or device tensors.  Chunks are cut on row boundaries at about
        `max_bytes` (default `mgf_io.DEFAULT_CHUNK_BYTES`); one larger row grows its chunk.  Every chunk is formatted into one
        device buffer and copied through one pinned host buffer, with one stream synchronisation; `copy=False` yields views of
        that pinned buffer, valid until the next chunk is asked for."""
        cols = self._csv_columns(file_id, file_names, file_name_ptr, ident, id_ptr, charge, precursor_mz, retention_time, cluster, order,
                                 quote_cr)
        if cols["rows"] == 0:
            return
        sizes, offsets, _ = self.csv_write_sizes(cols)            # (sizes: alive until the last chunk, as the buffers are)
        yield from self._write_chunks(cols["rows"], offsets, max_bytes, copy, lambda a, b, d, h: self.csv_write(cols, offsets, a, b, d, h))

    def _records_table(self, table):
        """a record table -- dict(n, head, tail, fields) with head / tail bytes and per field dict(kind "i32" / "i64" / "f32" /
        "text", column, ptr (text: i64[rows + 1]), index (i32[n] or None), prefix, suffix (bytes)) -- as the entry points' arguments:
        the columns as device tensors of the kinds' types, the literals as ranges of one blob (equal literals share their bytes)
        and the `fal_rec_field` array.  The dict keeps every tensor alive."""
        torch = _torch()
        dtypes = {"i32": torch.int32, "i64": torch.int64, "f32": torch.float32}
        n, fields = int(table["n"]), list(table["fields"])
        blob, where = bytearray(), {}

        def literal(b: bytes):
            if b not in where:
                where[b] = (len(blob), len(blob) + len(b))
                blob.extend(b)
            return where[b]

        head, tail = literal(bytes(table["head"])), literal(bytes(table["tail"]))
        recs, keep = (_lib.RecField * max(len(fields), 1))(), []
        for rec, f in zip(recs, fields):
            text = f["kind"] == "text"
            col = self._text_to_dev(f["column"]) if text else self.to_dev(f["column"], dtypes[f["kind"]])
            ptr = self.to_dev(f["ptr"], torch.int64) if text else None
            index = None if f.get("index") is None else self.to_dev(f["index"], torch.int32)
            rows = int(ptr.shape[0]) - 1 if text else int(col.shape[0])
            if (text and rows < 0) or (index is None and rows < n) or (index is not None and int(index.shape[0]) != n):
                raise ValueError(f"format_records: a field of {rows} rows{'' if index is None else ' and its index'} for {n} units")
            keep += [col, ptr, index]
            rec.column = col.data_ptr() if col.numel() else None
            rec.ptr = ptr.data_ptr() if text else None
            rec.index = index.data_ptr() if index is not None and n else None
            rec.rows, rec.blob_bytes, rec.kind = rows, col.numel() if text else 0, _lib.REC_KINDS[f["kind"]]
            rec.prefix[:], rec.suffix[:] = literal(bytes(f["prefix"])), literal(bytes(f["suffix"]))
        return dict(n=n, fields=recs, n_fields=len(fields), literals=self._text_to_dev(bytes(blob)), head=head, tail=tail, keep=keep)

    def _records_args(self, c):
        lit = c["literals"]
        return [c["n"], C.cast(c["fields"], C.c_void_p), c["n_fields"], self._p(lit) if lit.numel() else None, lit.numel(), *c["head"],
                *c["tail"]]

    def records_write_sizes(self, cols):
        """`fal_records_write_sizes` of a `_records_table` -> (sizes i64[n], offsets i64[n + 1] on the device, total bytes).
        Synchronises once."""
        return self._write_sizes("fal_records_write_sizes", self._records_args(cols), cols["n"])

    def records_write(self, cols, offsets, first: int, last: int, out, host_out=None):
        """`fal_records_write`: the text of units [first, last) into the uint8 device tensor (or view) `out`; `host_out`: a pinned
        uint8 host tensor of the same size that receives a copy.  Synchronises once.  FalconHipError (code `_lib.FAL_EINVAL`,
        nothing written) when `out` is too small."""
        self._write_range("fal_records_write", self._records_args(cols), offsets, first, last, out, host_out)

    def format_records(self, table, max_bytes: Optional[int] = None, copy: bool = True):
        """The text of the n units of a record table (`_records_table` states its form; DESIGN.md "Records of fields out of the
        device" the field model) as a generator of uint8 host arrays that together are the text: per unit the head, every present
        field as prefix, value, suffix, and the tail.  Arrays or device tensors.  Chunks are cut on unit boundaries at about
        `max_bytes` (default `mgf_io.DEFAULT_CHUNK_BYTES`); one larger unit grows its chunk.  Every chunk is formatted into one
        device buffer and copied through one pinned host buffer, with one stream synchronisation; `copy=False` yields views of
        that pinned buffer, valid until the next chunk is asked for."""
        cols = self._records_table(table)
        if cols["n"] == 0:
            return
        sizes, offsets, _ = self.records_write_sizes(cols)        # (sizes: alive until the last chunk, as the buffers are)
        yield from self._write_chunks(cols["n"], offsets, max_bytes, copy, lambda a, b, d, h: self.records_write(cols, offsets, a, b, d, h))

    def mzml_index(self, d_text):
        """`fal_mzml_index` of mzML text on the device (uint8 tensor) -> (spectra, tags inside spectra, `_lib.MZML_FLAG_*` bits,
        tags).  Synchronises once.  The tables stay in the context for the `mzml_parse` of the same tensor."""
        return self._text_index("fal_mzml_index", d_text)

    def mzml_parse(self, d_text, n: int):
        """`fal_mzml_parse` behind `mzml_index` of the same tensor -> device tensors payload u8[n_bytes + 16 n], status i32[n],
        id i64[n, 2], span i64[n, 2], precursor_mz f64[n], charge i32[n], retention_time f64[n], arrays i64[2 n, 4].  No sync."""
        torch = _torch()
        m = max(n, 1)
        payload = self.empty((d_text.numel() + 16 * n,), torch.uint8)
        status, charge = self.empty((m,), torch.int32), self.empty((m,), torch.int32)
        ident, span = self.empty((m, 2), torch.int64), self.empty((m, 2), torch.int64)
        pmz, rt = self.empty((m,), torch.float64), self.empty((m,), torch.float64)
        arrays = self.empty((2 * m, 4), torch.int64)
        check(self.lib.fal_mzml_parse(self._h, self._p(d_text) if d_text.numel() else None, d_text.numel(), n,
                                      self._p(payload) if payload.numel() else None, payload.numel(), self._p(status), self._p(ident),
                                      self._p(span), self._p(pmz), self._p(charge), self._p(rt), self._p(arrays)), "fal_mzml_parse")
        return payload, status[:n], ident[:n], span[:n], pmz[:n], charge[:n], rt[:n], arrays[:2 * n]

    def scan_mzml(self, text):
        """mzML text from a <spectrum ...> on (bytes, uint8 array or uint8 device tensor) -> dict: `flags` (`_lib.MZML_FLAG_*`;
        non-zero: the text is the host reader's and only `tags` is set besides), else `payload` u8[] on the device and the host
        arrays `status` i32[n] (`_lib.MZML_ST_*`), `id` / `span` i64[n, 2] (byte ranges of the id value and of the spectrum),
        `precursor_mz` f64, `charge` i32 (0: none), `retention_time` f64 (-1 when absent), `arrays` i64[2 n, 4] (rows 2 s and
        2 s + 1: the m/z and the intensity array of spectrum s for `decode_peaks`; zeros unless the status is OK), and `tags`,
        `inside` (tags, and tags inside spectra).  DESIGN.md "mzML on the device" states the grammar."""
        d_text = self._text_to_dev(text)
        n, inside, flags, tags = self.mzml_index(d_text)
        if flags:
            return dict(flags=flags, tags=tags)
        payload, *cols = self.mzml_parse(d_text, n)
        status, ident, span, pmz, charge, rt, arrays = (c.cpu().numpy() for c in cols)
        return dict(flags=0, tags=tags, inside=inside, payload=payload, status=status, id=ident, span=span, precursor_mz=pmz,
                    charge=charge, retention_time=rt, arrays=arrays)

    def consensus_spectra(self, mz, intensity, indptr, labels, medoids, fragment_tol: float, min_fraction: float = 0.25,
                          nnz_cap: Optional[int] = None):
        """`fal_consensus_spectra`: every cluster's members merged peak by peak (DESIGN.md "Consensus representatives").
        mz / intensity f32, indptr i64[n+1]: the preprocessed peaks by dataset row; labels i32[n] in [0, n_clusters); medoids
        i32[n_clusters].  nnz_cap: room for the output peaks (default: the dataset's peak count, which always suffices).
        -> indptr i64[n_clusters+1], mz f32, intensity f32, status i32[n_clusters] of `_lib.CONS_*` bits.  Device tensors;
        synchronises.  Raises FalconHipError when nnz_cap is too small for the output (indptr would point behind the peaks
        returned); the C entry point itself reports that per cluster with `_lib.CONS_CAPACITY`."""
        torch = _torch()
        mz = self.to_dev(mz, torch.float32)
        intensity = self.to_dev(intensity, torch.float32)
        indptr = self.to_dev(indptr, torch.int64)
        labels = self.to_dev(labels, torch.int32)
        medoids = self.to_dev(medoids, torch.int32)
        n, nc = int(labels.shape[0]), int(medoids.shape[0])
        if indptr.shape[0] != n + 1:
            raise ValueError(f"consensus_spectra: indptr has {indptr.shape[0]} entries for {n} labels")
        cap = int(mz.shape[0]) if nnz_cap is None else int(nnz_cap)
        out_indptr = self.empty((nc + 1,), torch.int64)
        out_mz = self.empty((max(cap, 1),), torch.float32)
        out_it = self.empty((max(cap, 1),), torch.float32)
        status = self.empty((max(nc, 1),), torch.int32)
        check(self.lib.fal_consensus_spectra(self._h, self._p(mz), self._p(intensity), self._p(indptr), n, self._p(labels),
                                             self._p(medoids), nc, float(fragment_tol), float(min_fraction), cap,
                                             self._p(out_indptr), self._p(out_mz), self._p(out_it), self._p(status)),
              "fal_consensus_spectra")
        used = int(out_indptr[-1].item())
        if used > cap:
            raise FalconHipError(f"consensus_spectra: the consensus holds {used} peaks, nnz_cap = {cap} is too small")
        return out_indptr, out_mz[:used], out_it[:used], status[:nc]

    def rescore_neighbors(self, nb_idx, nb_dist, mz, intensity, indptr, order, fragment_tol: float, min_matches: int):
        """f4 (`fal_rescore_neighbors`): nb_dist <- 1 - matched-peak cosine (reference similarity.py:17-80), in place."""
        torch = _torch()
        n, k = nb_idx.shape
        mz = self.to_dev(mz, torch.float32)
        intensity = self.to_dev(intensity, torch.float32)
        indptr = self.to_dev(indptr, torch.int64)
        order = self.to_dev(order, torch.int64)
        check(self.lib.fal_rescore_neighbors(self._h, self._p(nb_idx), self._p(nb_dist), n, k, self._p(mz), self._p(intensity),
                                             self._p(indptr), self._p(order), float(fragment_tol), int(min_matches)),
              "fal_rescore_neighbors")
        return nb_dist

    def neighbors_to_csr(self, nb_idx, nb_dist, id_offset: int = 0, out=None, row0: int = 0, nb_count=None, id_map=None):
        """ELL neighbour lists -> CSR (indptr i64[rows+1], idx i32[cap], dist f32[cap]); entries beyond
        indptr[-1] are unspecified.  `out` = (indptr, idx, dist) buffers to fill; with `row0` > 0 the call
        appends a further segment (rows row0.. of `out`, ids shifted by its own id_offset).  `id_map` (i64):
        stored id -> id_map[id] + id_offset (a bucket shard's positions -> dataset rows).  No sync."""
        torch = _torch()
        n, k = nb_idx.shape
        if out is None:
            out = (self.empty((row0 + n + 1,), torch.int64), self.empty((max((row0 + n) * k, 1),), torch.int32),
                   self.empty((max((row0 + n) * k, 1),), torch.float32))
        indptr, idx, dist = out
        if indptr.numel() < row0 + n + 1:
            raise FalconHipError("neighbors_to_csr: indptr buffer too small")
        check(self.lib.fal_neighbors_to_csr_mapped(self._h, self._p(nb_idx), self._p(nb_dist), self._p(nb_count), n, k,
                                                   self._p(id_map), int(id_offset), int(row0),
                                                   self._p(indptr), self._p(idx), self._p(dist)), "fal_neighbors_to_csr")
        return indptr, idx, dist

    def dbscan(self, nb_idx, nb_dist, eps: float):
        torch = _torch()
        n, k = nb_idx.shape
        labels = self.empty((n,), torch.int32)
        nc = C.c_int64()
        check(self.lib.fal_dbscan(self._h, self._p(nb_idx), self._p(nb_dist), n, k, float(eps), self._p(labels),
                                  C.byref(nc)), "fal_dbscan")
        return labels, int(nc.value)

    def refine_clusters(self, labels, n_clusters: int, mz_sorted, rt_sorted, tol: float, mode: str, rt_tol):
        nc = C.c_int64(int(n_clusters))
        check(self.lib.fal_refine_clusters(self._h, self._p(labels), labels.numel(), self._p(mz_sorted),
                                           self._p(rt_sorted), float(tol), int(mode == "Da"),
                                           -1.0 if rt_tol is None else float(rt_tol), C.byref(nc)),
              "fal_refine_clusters")
        return labels, int(nc.value)

    def finalize(self, labels_sorted, n_clusters: int, order, nb_idx, nb_dist):
        torch = _torch()
        n, k = nb_idx.shape
        labels = self.empty((n,), torch.int32)
        medoids = self.empty((n,), torch.int32)
        nl = C.c_int64()
        check(self.lib.fal_finalize(self._h, self._p(labels_sorted), n, int(n_clusters), self._p(order),
                                    self._p(nb_idx), self._p(nb_dist), k, self._p(labels), self._p(medoids),
                                    C.byref(nl)), "fal_finalize")
        return labels, medoids[:int(nl.value)]


    LINKAGE = {"single": 0, "complete": 1, "average": 2}

    def graph_tile_limits(self):
        """-> (rows that close a tile, most rows of one bucket `fal_cluster_graph_tiled` takes per tile)"""
        t, m = C.c_int(), C.c_int()
        self.lib.fal_graph_tile_limits(C.byref(t), C.byref(m))
        return t.value, m.value

    def graph_tile_capacity(self, max_rows: int, rows: int):
        """-> (dynamic LDS bytes of the DBSCAN tile kernel in a call whose largest tile has `max_rows` rows, eps-edges the
        list of a tile of `rows` rows holds in that call); `counter(11)` counts the tiles of a call that had more"""
        b, c = C.c_int64(), C.c_int64()
        self.lib.fal_graph_tile_capacity(int(max_rows), int(rows), C.byref(b), C.byref(c))
        return b.value, c.value

    def cluster_graph(self, nb_idx, nb_dist, eps: float, mz_sorted, rt_sorted, tol: float, mode: str, rt_tol, order,
                      linkage: Optional[str] = None, nb_count=None, splits=None):
        """a9..a12 fused: -> labels i32[n] (dataset rows), medoids i32[n_labels], labels_sorted, n_clusters.
        `linkage` = None: DBSCAN(eps); "single" / "complete" / "average": hierarchical clustering cut at `eps` (f4).
        `nb_count` (the search's per-row neighbour counts, rows front-packed): the graph passes read the stored slots only.
        `splits` (host, the bucket table the search ran on; DBSCAN with `nb_count` only): `fal_cluster_graph_tiled`, the same
        results computed per tile of whole buckets (`counter(10)` tells whether the tiles or the per-row path ran)."""
        torch = _torch()
        n, k = nb_idx.shape
        lab_sorted = self.empty((n,), torch.int32)
        labels = self.empty((n,), torch.int32)
        medoids = self.empty((n,), torch.int32)
        nc, nl = C.c_int64(), C.c_int64()
        tail = (self._p(mz_sorted), self._p(rt_sorted), float(tol), int(mode == "Da"),
                -1.0 if rt_tol is None else float(rt_tol), self._p(order), self._p(lab_sorted), self._p(labels),
                self._p(medoids), C.byref(nc), C.byref(nl))
        if linkage is None and nb_count is not None and splits is not None:
            sp = np.ascontiguousarray(splits, dtype=np.int64)
            check(self.lib.fal_cluster_graph_tiled(self._h, self._p(nb_idx), self._p(nb_dist), self._p(nb_count), n, k,
                                                   float(eps), sp.ctypes.data_as(C.c_void_p), len(sp) - 1, *tail),
                  "fal_cluster_graph_tiled")
        elif linkage is None and nb_count is not None:
            check(self.lib.fal_cluster_graph_counted(self._h, self._p(nb_idx), self._p(nb_dist), self._p(nb_count), n, k,
                                                     float(eps), *tail), "fal_cluster_graph_counted")
        elif linkage is None:
            check(self.lib.fal_cluster_graph(self._h, self._p(nb_idx), self._p(nb_dist), n, k, float(eps), *tail),
                  "fal_cluster_graph")
        else:
            check(self.lib.fal_cluster_graph_linkage(self._h, self._p(nb_idx), self._p(nb_dist), n, k, float(eps),
                                                     self.LINKAGE[linkage], *tail), "fal_cluster_graph_linkage")
        return labels, medoids[:int(nl.value)], lab_sorted, int(nc.value)

    def linkage_cluster(self, nb_idx, nb_dist, threshold: float, linkage: str):
        """f4 staged (`fal_linkage_cluster`): -> labels i32[n] (clusters by lowest row, -1 = groups of one), n_clusters"""
        torch = _torch()
        n, k = nb_idx.shape
        labels = self.empty((n,), torch.int32)
        nc = C.c_int64()
        check(self.lib.fal_linkage_cluster(self._h, self._p(nb_idx), self._p(nb_dist), n, k, float(threshold),
                                           self.LINKAGE[linkage], self._p(labels), C.byref(nc)), "fal_linkage_cluster")
        return labels, int(nc.value)

    # ------------------------------------------------------------------ f5 exact mode
    def _peaks(self, mz, intensity, indptr, order):
        torch = _torch()
        mz, intensity = self.to_dev(mz, torch.float32), self.to_dev(intensity, torch.float32)
        if mz.numel() == 0:                  # spectra without a single peak: an empty tensor has no address, the library takes no NULL
            mz, intensity = self.empty((1,), torch.float32), self.empty((1,), torch.float32)
        return mz, intensity, self.to_dev(indptr, torch.int64), self.to_dev(order, torch.int64)

    @staticmethod
    def _check_order(order, indptr, n_out: int, what: str):
        """exact mode reads the peaks of row order[i] and writes labels_out[order[i]]: every entry must be a row of the CSR
        and fit the n_out-row outputs.  One min / max on the host before any launch (a subset whose `order` holds
        dataset rows has to run as a compact CSR, order = arange).  The min / max costs one device-to-host wait per call,
        single-GPU passes included; accepted: both callers wait for the library anyway (`fal_cluster_exact` synchronises
        to read its counts, `fal_exact_edges` to read the edge count), and an out-of-range order would write past a
        device buffer."""
        if order.numel() == 0:
            return
        lo, hi = (int(x) for x in _torch().aminmax(order))
        if lo < 0 or hi >= min(int(n_out), int(indptr.numel()) - 1):
            raise ValueError(f"{what}: row_order holds rows in [{lo}, {hi}], outside the {n_out} output rows / "
                             f"{int(indptr.numel()) - 1} CSR rows (run a subset as a compact CSR with order = arange)")

    def exact_edges(self, mz, intensity, indptr, order, splits, fragment_tol: float, min_matches: int, threshold: float,
                    max_edges: Optional[int] = None):
        """f5 staged (`fal_exact_edges`): every pair of every bucket of `splits` scored with the matched-peak cosine
        -> symmetric CSR of the pairs with d <= threshold in sorted-row space: (indptr i64[n+1], idx i32[m], dist f64[m]).
        `max_edges` (directed entries) defaults to every pair of the buckets."""
        torch = _torch()
        mz, intensity, indptr, order = self._peaks(mz, intensity, indptr, order)
        n = order.numel()
        self._check_order(order, indptr, int(indptr.numel()) - 1, "exact_edges")
        sp = np.ascontiguousarray(splits, dtype=np.int64)
        if max_edges is None:
            nb = np.diff(sp)
            max_edges = int((nb * (nb - 1)).sum())
        ptr = self.empty((n + 1,), torch.int64)
        idx = self.empty((max(max_edges, 1),), torch.int32)
        dist = self.empty((max(max_edges, 1),), torch.float64)
        m = C.c_int64()
        check(self.lib.fal_exact_edges(self._h, self._p(mz), self._p(intensity), self._p(indptr), self._p(order), n,
                                       sp.ctypes.data_as(C.c_void_p), len(sp), float(fragment_tol), int(min_matches),
                                       float(threshold), self._p(ptr), self._p(idx), self._p(dist), int(max_edges), C.byref(m)),
              "fal_exact_edges")
        return ptr, idx[:m.value], dist[:m.value]

    def linkage_cluster_csr(self, indptr_csr, idx, dist, threshold: float, linkage: str, mz=None, intensity=None, indptr=None,
                            order=None, fragment_tol: float = 0.0, min_matches: int = 0):
        """f5 staged (`fal_linkage_cluster_csr`): `linkage_cluster` on exact mode's CSR; average linkage needs the peaks
        (every member pair of a connected group is scored again).  -> labels i32[n], n_clusters"""
        torch = _torch()
        n = indptr_csr.numel() - 1
        peaks = (None,) * 4 if mz is None else self._peaks(mz, intensity, indptr, order)
        labels = self.empty((max(n, 1),), torch.int32)
        nc = C.c_int64()
        check(self.lib.fal_linkage_cluster_csr(self._h, self._p(indptr_csr), self._p(idx), self._p(dist), n, float(threshold),
                                               self.LINKAGE[linkage], *(self._p(t) for t in peaks), float(fragment_tol),
                                               int(min_matches), self._p(labels), C.byref(nc)), "fal_linkage_cluster_csr")
        return labels[:n], int(nc.value)

    def cluster_exact(self, mz, intensity, indptr, order, splits, fragment_tol: float, min_matches: int, threshold: float,
                      linkage: str, mz_sorted, rt_sorted, tol: float, mode: str, rt_tol):
        """f5 fused (`fal_cluster_exact`): all-pairs edges -> linkage -> refinement -> exact medoids -> labels.
        -> labels i32[n] (dataset rows), medoids i32[n_labels], labels_sorted, n_clusters (as `cluster_graph`)"""
        torch = _torch()
        mz, intensity, indptr, order = self._peaks(mz, intensity, indptr, order)
        n = order.numel()
        self._check_order(order, indptr, n, "cluster_exact")
        sp = np.ascontiguousarray(splits, dtype=np.int64)
        lab_sorted = self.empty((n,), torch.int32)
        labels = self.empty((n,), torch.int32)
        medoids = self.empty((n,), torch.int32)
        nc, nl = C.c_int64(), C.c_int64()
        check(self.lib.fal_cluster_exact(self._h, self._p(mz), self._p(intensity), self._p(indptr), self._p(order), n,
                                         sp.ctypes.data_as(C.c_void_p), len(sp), float(fragment_tol), int(min_matches),
                                         float(threshold), self.LINKAGE[linkage], self._p(mz_sorted), self._p(rt_sorted),
                                         float(tol), int(mode == "Da"), -1.0 if rt_tol is None else float(rt_tol),
                                         self._p(lab_sorted), self._p(labels), self._p(medoids), C.byref(nc), C.byref(nl)),
              "fal_cluster_exact")
        return labels, medoids[:int(nl.value)], lab_sorted, int(nc.value)


    # ------------------------------------------------------------------ nearest representative
    def assign_nearest(self, q_mz, q_intensity, q_indptr, q_precursor_mz, q_rt, l_mz, l_intensity, l_indptr, l_precursor_mz, l_rt,
                       tol: float, mode: str, rt_tol, fragment_tol: float, min_matches: int):
        """`fal_assign_nearest`: for every query spectrum the nearest library spectrum (matched-peak cosine, the query first)
        among the library rows inside its precursor (and RT) tolerance.  Peaks f32 CSR per side, precursor m/z f32, RT f32 or
        None (needed on both sides when `rt_tol` is given).
        -> best_row i32[nq] (library row, -1 = no candidate), best_dist f32[nq] (1.0 then), n_cand i32[nq].  Device tensors;
        synchronises once."""
        torch = _torch()
        q_pmz, l_pmz = self.to_dev(q_precursor_mz, torch.float32), self.to_dev(l_precursor_mz, torch.float32)
        nq, nl = int(q_pmz.numel()), int(l_pmz.numel())
        if rt_tol is not None and nq and nl and (q_rt is None or l_rt is None):
            raise ValueError("assign_nearest: rt_tol needs the retention times of both sides")
        q_mz, q_intensity, q_indptr, _ = self._peaks(q_mz, q_intensity, q_indptr, np.zeros(0, np.int64))
        l_mz, l_intensity, l_indptr, _ = self._peaks(l_mz, l_intensity, l_indptr, np.zeros(0, np.int64))
        if q_indptr.numel() != nq + 1 or l_indptr.numel() != nl + 1:
            raise ValueError(f"assign_nearest: indptr has {q_indptr.numel()} / {l_indptr.numel()} entries for {nq} / {nl} spectra")
        q_rt = None if q_rt is None or rt_tol is None else self.to_dev(q_rt, torch.float32)
        l_rt = None if l_rt is None or rt_tol is None else self.to_dev(l_rt, torch.float32)
        best_row = self.empty((nq,), torch.int32)
        best_dist = self.empty((nq,), torch.float32)
        n_cand = self.empty((nq,), torch.int32)
        ptr = lambda t: self._p(t if t is not None and t.numel() else None)
        check(self.lib.fal_assign_nearest(self._h, ptr(q_mz), ptr(q_intensity), ptr(q_indptr), ptr(q_pmz), ptr(q_rt), nq, ptr(l_mz),
                                          ptr(l_intensity), ptr(l_indptr), ptr(l_pmz), ptr(l_rt), nl, float(tol), int(mode == "Da"),
                                          -1.0 if rt_tol is None else float(rt_tol), float(fragment_tol), int(min_matches),
                                          ptr(best_row), ptr(best_dist), ptr(n_cand)), "fal_assign_nearest")
        return best_row, best_dist, n_cand

    # ------------------------------------------------------------------ member scores and cluster summary
    def member_scores(self, mz, intensity, indptr, labels, rep_mz, rep_intensity, rep_indptr, rep_row, fragment_tol: float):
        """`fal_member_scores`: every spectrum of a clustered partition scored against its cluster's representative (DESIGN.md
        "Member scores and cluster summary").  mz / intensity f32, indptr i64[n+1]: the partition's peaks; labels i32[n] in
        [0, n_clusters); the representatives are rows of the CSR rep_mz / rep_intensity / rep_indptr, cluster c's is row
        rep_row[c] (i32[n_clusters]): the partition's own CSR with the medoids, or the consensus CSR with arange.  Host or
        device arrays.  -> similarity f32[n], matched i32[n].  Device tensors; synchronises once."""
        torch = _torch()
        labels = self.to_dev(labels, torch.int32)
        rep_row = self.to_dev(rep_row, torch.int32)
        n, nc = int(labels.numel()), int(rep_row.numel())
        mz, intensity, indptr, _ = self._peaks(mz, intensity, indptr, np.zeros(0, np.int64))
        rep_mz, rep_intensity, rep_indptr, _ = self._peaks(rep_mz, rep_intensity, rep_indptr, np.zeros(0, np.int64))
        if indptr.numel() != n + 1:
            raise ValueError(f"member_scores: indptr has {indptr.numel()} entries for {n} labels")
        n_rep = int(rep_indptr.numel()) - 1
        if n_rep < 0:
            raise ValueError("member_scores: the representatives' indptr is empty")
        similarity = self.empty((n,), torch.float32)
        matched = self.empty((n,), torch.int32)
        ptr = lambda t: self._p(t if t is not None and t.numel() else None)
        check(self.lib.fal_member_scores(self._h, ptr(mz), ptr(intensity), ptr(indptr), n, ptr(labels), nc, ptr(rep_mz),
                                         ptr(rep_intensity), ptr(rep_indptr), n_rep, ptr(rep_row), float(fragment_tol),
                                         ptr(similarity), ptr(matched)), "fal_member_scores")
        return similarity, matched

    SUMMARY_COLUMNS = ("size", "sim_min", "worst_row", "sim_mean", "pmz_min", "pmz_max", "rt_min", "rt_max")

    def cluster_summary(self, labels, n_clusters: int, similarity, precursor_mz, retention_time=None):
        """`fal_cluster_summary`: the per-cluster columns over a partition's member scores.  labels i32[n], similarity and
        precursor_mz f32[n], retention_time f32[n] or None (rt_min / rt_max are 0 then).  Host or device arrays.
        -> dict of device tensors [n_clusters]: size i32, sim_min f32, worst_row i32, sim_mean f64, pmz_min, pmz_max, rt_min,
        rt_max f32.  Does not synchronise."""
        torch = _torch()
        labels = self.to_dev(labels, torch.int32)
        similarity = self.to_dev(similarity, torch.float32)
        pmz = self.to_dev(precursor_mz, torch.float32)
        rt = None if retention_time is None else self.to_dev(retention_time, torch.float32)
        n, nc = int(labels.numel()), int(n_clusters)
        if similarity.numel() != n or pmz.numel() != n or (rt is not None and rt.numel() != n):
            raise ValueError(f"cluster_summary: the columns do not all have {n} rows")
        types = dict(size=torch.int32, worst_row=torch.int32, sim_mean=torch.float64)
        out = {c: self.empty((nc,), types.get(c, torch.float32)) for c in self.SUMMARY_COLUMNS}
        ptr = lambda t: self._p(t if t is not None and t.numel() else None)
        check(self.lib.fal_cluster_summary(self._h, ptr(labels), n, nc, ptr(similarity), ptr(pmz), ptr(rt),
                                           *(ptr(out[c]) for c in self.SUMMARY_COLUMNS)), "fal_cluster_summary")
        return out

    # ------------------------------------------------------------------ representative network
    def network_edges(self, mz, intensity, indptr, rows, precursor_mz, fragment_tol: float, max_shift: float = 200.0,
                      min_cosine: float = 0.7, min_matched: int = 6, top_k: int = 10, max_edges: Optional[int] = None):
        """`fal_network_edges`: the pairs of nodes whose greedy modified cosine is high (DESIGN.md "Representative network").
        mz / intensity f32, indptr i64: a peak CSR; node v is its row rows[v] (i32[n]) with precursor m/z precursor_mz[v]
        (f32[n]).  Host or device arrays.  `max_edges`: the room of the first call (default 16 edges a node); a result that
        does not fit is fetched by a second call with the room the first one reported.
        -> u i32[m] < v i32[m] (node indices), similarity f32[m], matched i32[m] in (u, v) order.  Device tensors; the call
        synchronises up to five times."""
        torch = _torch()
        rows = self.to_dev(rows, torch.int32)
        pmz = self.to_dev(precursor_mz, torch.float32)
        n = int(rows.numel())
        if pmz.numel() != n:
            raise ValueError(f"network_edges: {pmz.numel()} precursors for {n} nodes")
        mz, intensity, indptr, _ = self._peaks(mz, intensity, indptr, np.zeros(0, np.int64))
        n_csr = int(indptr.numel()) - 1
        if n_csr < 0:
            raise ValueError("network_edges: indptr is empty")
        room =int(16 * n if max_edges is None else max_edges)
        m = C.c_int64()
        ptr = lambda t: self._p(t if t is not None and t.numel() else None)
        for _ in range(2):
            u, v = self.empty((room,), torch.int32), self.empty((room,), torch.int32)
            sim, matched = self.empty((room,), torch.float32), self.empty((room,), torch.int32)
            rc = self.lib.fal_network_edges(self._h, ptr(mz), ptr(intensity), ptr(indptr), n_csr, ptr(rows), ptr(pmz), n,
                                            float(fragment_tol), float(max_shift), float(min_cosine), int(min_matched), int(top_k),
                                            ptr(u), ptr(v), ptr(sim), ptr(matched), room, C.byref(m))
            if rc == _lib.FAL_EINVAL and m.value > room:
                room = int(m.value)              # the edges did not fit: once more with room for them
                continue
            break
        check(rc, "fal_network_edges")
        k = int(m.value)
        return u[:k], v[:k], sim[:k], matched[:k]

    def network_families(self, u, v, sim, n: int, max_size: int = 100, delta: float = 0.02):
        """`fal_network_families`: the connected components of `n` nodes under the edges (u, v i32[m], sim f32[m]; host or
        device arrays, `network_edges`' output as it comes), cut until none has more than `max_size` nodes (0: no cap; DESIGN.md
        "Molecular families").
        -> family i32[n] (-1: no surviving edge), size i32[n], edge_round i32[m] (0: the edge survives) as device tensors,
        n_families, n_rounds.  The call synchronises n_rounds + 2 times."""
        torch = _torch()
        u, v, sim = self.to_dev(u, torch.int32), self.to_dev(v, torch.int32), self.to_dev(sim, torch.float32)
        m, n = int(u.numel()), int(n)
        if v.numel() != m or sim.numel() != m:
            raise ValueError(f"network_families: the edge columns do not all have {m} rows")
        if n < 0:
            raise ValueError(f"network_families: {n} nodes")
        family, size = self.empty((n,), torch.int32), self.empty((n,), torch.int32)
        edge_round = self.empty((m,), torch.int32)
        nf, nr = C.c_int64(), C.c_int64()
        ptr = lambda t: self._p(t if t.numel() else None)
        check(self.lib.fal_network_families(self._h, ptr(u), ptr(v), ptr(sim), m, n, int(max_size), float(delta), ptr(family),
                                            ptr(size), ptr(edge_round), C.byref(nf), C.byref(nr)), "fal_network_families")
        return family, size, edge_round, int(nf.value), int(nr.value)

    def network_propagate(self, u, v, sim, n: int, seed, max_hops: int = 3, min_score: float = 0.0):
        """`fal_network_propagate`: the annotations of the seeded nodes carried along the links (u, v i32[m], sim f32[m]; host or
        device arrays, the surviving links of `network_families` as they come), level by level, at most `max_hops` links far
        (DESIGN.md "Annotation propagation").  `seed` i32[n]: >= 0 marks an annotated node, -1 one that is not.  A link offers
        its unreached end the score of the other end times its sim; offers below `min_score` do not count; the greatest wins,
        of equal ones the lowest parent.
        -> source, hops, parent i32[n] (-1: not reached), score f32[n] as device tensors, n_reached, n_levels.  The call
        synchronises once."""
        torch = _torch()
        u, v, sim = self.to_dev(u, torch.int32), self.to_dev(v, torch.int32), self.to_dev(sim, torch.float32)
        seed = self.to_dev(seed, torch.int32)
        m, n = int(u.numel()), int(n)
        if v.numel() != m or sim.numel() != m:
            raise ValueError(f"network_propagate: the link columns do not all have {m} rows")
        if n < 0 or seed.numel() != n:
            raise ValueError(f"network_propagate: {seed.numel()} seeds for {n} nodes")
        source, hops, parent = (self.empty((n,), torch.int32) for _ in range(3))
        score = self.empty((n,), torch.float32)
        reached, levels = C.c_int64(), C.c_int64()
        ptr = lambda t: self._p(t if t.numel() else None)
        check(self.lib.fal_network_propagate(self._h, ptr(u), ptr(v), ptr(sim), m, n, ptr(seed), int(max_hops), float(min_score),
                                             ptr(source), ptr(hops), ptr(parent), ptr(score), C.byref(reached), C.byref(levels)),
              "fal_network_propagate")
        return source, hops, parent, score, int(reached.value), int(levels.value)

    # ------------------------------------------------------------------ library search
    def library_search(self, q_mz, q_intensity, q_indptr, q_rows, q_precursor_mz, l_mz, l_intensity, l_indptr, l_rows,
                       l_precursor_mz, fragment_tol: float, precursor_tol: float, tol_is_da: bool, analog: bool = False,
                       max_shift: float = 200.0, min_cosine: float = 0.7, min_matched: int = 6, top_n: int = 1,
                       max_hits: Optional[int] = None):
        """`fal_library_search`: for every query its best hits in a library by greedy (modified) cosine (DESIGN.md "Library
        search").  Each side is a peak CSR (mz / intensity f32, indptr i64) of its own: query v is row q_rows[v] (i32[nq]) with
        precursor m/z q_precursor_mz[v] (f32[nq]), library entry w is row l_rows[w] of the second CSR.  Host or device arrays.
        `max_hits`: the room of the first call (default max(top_n, 4) hits a query); a result that does not fit is fetched by a
        second call with the room the first one reported.
        -> query i32[m], library i32[m] (indices), similarity f32[m], matched i32[m] in (query, rank) order.  Device tensors; the
        call synchronises up to five times."""
        torch = _torch()
        q_rows, l_rows = self.to_dev(q_rows, torch.int32), self.to_dev(l_rows, torch.int32)
        q_pmz, l_pmz = self.to_dev(q_precursor_mz, torch.float32), self.to_dev(l_precursor_mz, torch.float32)
        nq, nl = int(q_rows.numel()), int(l_rows.numel())
        if q_pmz.numel() != nq or l_pmz.numel() != nl:
            raise ValueError(f"library_search: {q_pmz.numel()} / {l_pmz.numel()} precursors for {nq} queries / {nl} library spectra")
        q_mz, q_intensity, q_indptr, _ = self._peaks(q_mz, q_intensity, q_indptr, np.zeros(0, np.int64))
        l_mz, l_intensity, l_indptr, _ = self._peaks(l_mz, l_intensity, l_indptr, np.zeros(0, np.int64))
        q_csr, l_csr = int(q_indptr.numel()) - 1, int(l_indptr.numel()) - 1
        if q_csr < 0 or l_csr < 0:
            raise ValueError("library_search: indptr is empty")
        room = int(max(int(top_n), 4) * nq if max_hits is None else max_hits)
        m = C.c_int64()
        ptr = lambda t: self._p(t if t is not None and t.numel() else None)
        for _ in range(2):
            query, library = self.empty((room,), torch.int32), self.empty((room,), torch.int32)
            sim, matched = self.empty((room,), torch.float32), self.empty((room,), torch.int32)
            rc = self.lib.fal_library_search(self._h, ptr(q_mz), ptr(q_intensity), ptr(q_indptr), q_csr, ptr(q_rows), ptr(q_pmz), nq,
                                             ptr(l_mz), ptr(l_intensity), ptr(l_indptr), l_csr, ptr(l_rows), ptr(l_pmz), nl,
                                             float(fragment_tol), float(precursor_tol), int(bool(tol_is_da)), int(bool(analog)),
                                             float(max_shift), float(min_cosine), int(min_matched), int(top_n), ptr(query),
                                             ptr(library), ptr(sim), ptr(matched), room, C.byref(m))
            if rc == _lib.FAL_EINVAL and m.value > room:
                room = int(m.value)              # the hits did not fit: once more with room for them
                continue
            break
        check(rc, "fal_library_search")
        k = int(m.value)
        return query[:k], library[:k], sim[:k], matched[:k]


class IvfIndex:
    """Opaque `fal_ivf` handle (keeps the vectors alive: the index borrows them)."""

    def __init__(self, ctx: Context, handle, X, bucket_off, n_list, n, d):
        self.ctx, self._h, self.X, self.X16, self.Xpre = ctx, handle, X, None, None
        self.bucket_off, self.n_list = bucket_off, n_list
        self.n, self.d = n, d
        t = C.c_int64()
        check(ctx.lib.fal_ivf_total_lists(self._h, C.byref(t)))
        self.total_lists = int(t.value)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):            # (the context owns the pool the index's arrays return to)
                self.ctx.lib.fal_ivf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def export(self):
        """-> centroids [total_lists, d], assign [n], perm [n], list_off [total_lists+1] (device)."""
        torch = _torch()
        c = self.ctx
        cent = c.empty((self.total_lists, self.d), torch.float32)
        asg = c.empty((self.n,), torch.int32)
        perm = c.empty((self.n,), torch.int32)
        off = c.empty((self.total_lists + 1,), torch.int64)
        check(c.lib.fal_ivf_export(c._h, self._h, c._p(cent), c._p(asg), c._p(perm), c._p(off)), "fal_ivf_export")
        return cent, asg, perm, off

    def search(self, n_probe: int, k_ann: int):
        """-> sim f32[n, k_ann] (pad -inf), idx i32[n, k_ann] (pad -1), rows = sorted rows."""
        torch = _torch()
        c = self.ctx
        sim = c.empty((self.n, k_ann), torch.float32)
        idx = c.empty((self.n, k_ann), torch.int32)
        check(c.lib.fal_ivf_search_topk(c._h, self._h, int(n_probe), int(k_ann), c._p(sim), c._p(idx)),
              "fal_ivf_search_topk")
        return sim, idx

    def search_neighbors(self, n_probe: int, k_ann: int, mz_sorted, rt_sorted, tol: float, mode: str, rt_tol,
                         n_neighbors: int):
        """a7 + a8 fused (`fal_ivf_search_neighbors`): -> nb_idx i32[n, n_neighbors] (pad -1), nb_dist f32 (pad +inf);
        identical to `search` followed by `Context.filter_neighbors`."""
        torch = _torch()
        c = self.ctx
        nb_idx = c.empty((self.n, n_neighbors), torch.int32)
        nb_dist = c.empty((self.n, n_neighbors), torch.float32)
        self.nb_count = c.empty((self.n,), torch.int32)         # stored neighbours per row (rows are front-packed)
        check(c.lib.fal_ivf_search_neighbors(c._h, self._h, int(n_probe), int(k_ann), c._p(mz_sorted), c._p(rt_sorted),
                                             float(tol), int(mode == "Da"), -1.0 if rt_tol is None else float(rt_tol),
                                             int(n_neighbors), c._p(nb_idx), c._p(nb_dist), c._p(self.nb_count)),
              "fal_ivf_search_neighbors")
        return nb_idx, nb_dist


def get_dim(min_mz: float, max_mz: float, bin_size: float):
    """Reference spectrum.py:172-199 (float32 arithmetic), host side of the C ABI."""
    lib = _lib.load()
    dim, s, e = C.c_uint32(), C.c_float(), C.c_float()
    check(lib.fal_get_dim(min_mz, max_mz, bin_size, C.byref(dim), C.byref(s), C.byref(e)), "fal_get_dim")
    return int(dim.value), float(s.value), float(e.value)


def row_width(low_dim: int) -> int:
    """`fal_row_width`: columns of the rows the path stores `low_dim`-dimensional vectors in (64 / 128 / 256 / 400 / 800: the
    widths the cosine kernels are instantiated for; zero columns behind low_dim).  Raises beyond 800."""
    lib = _lib.load()
    w = C.c_uint32()
    if int(low_dim) < 1:
        raise FalconHipError(f"low_dim must be a positive integer (got {low_dim})")
    check(lib.fal_row_width(int(low_dim), C.byref(w)), "fal_row_width")
    return int(w.value)


def hash_lookup(n_bins: int, low_dim: int, seed: int = 0) -> np.ndarray:
    lib = _lib.load()
    out = np.empty(n_bins, np.uint32)
    check(lib.fal_hash_lookup(n_bins, low_dim, seed, out.ctypes.data_as(C.c_void_p)), "fal_hash_lookup")
    return out
