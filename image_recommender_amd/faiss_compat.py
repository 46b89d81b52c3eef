"""faiss-compatible index objects backed by the MI355X k-NN kernels (libimgrec.so).

This module is the drop-in boundary of SURVEY.md §8b: it provides exactly the faiss Python
surface that the reference's hot path touches, so ``import faiss`` in the reference can be
replaced by ``from image_recommender_amd import faiss_compat as faiss``:

================================  =================================================================
reference call                    where
================================  =================================================================
``faiss.IndexHNSWFlat(d, M)``     main/create_index.py:219, 230 (+ ``.hnsw.efConstruction/
                                  efSearch`` sets at :220-221, 231-232)
``faiss.IndexIVFPQ(q,d,nl,m,nb)`` main/create_index.py:226
``index.is_trained / train``      main/create_index.py:296-298
``index.add(arr)``                main/create_index.py:311
``index.ntotal``                  main/create_index.py:321, main/search_from_image.py:340
``faiss.write_index``             main/create_index.py:320
``faiss.read_index``              main/search_from_image.py:339
``faiss.normalize_L2``            main/search_from_image.py:322
``index.search(q, k)``            main/search_from_image.py:247, Analytics/rt_Search.py:63
``faiss.Kmeans(d, k, niter=..,    vector_scripts/create_sift_vector.py:221 (``.train(x)`` at :226,
gpu=True)``                       ``.centroids`` at :227): kmeans_train (csrc/knn_kmeans.hip)
================================  =================================================================

Beyond the reference's own calls, ``index.range_search(x, thresh) -> (lims, D, I)`` (every faiss
flat index has it: all rows within a radius, the near-duplicate query) is served by every class
here, multi-device indexes included; ``sharded.ShardedIndex`` and ``ivfpq`` do not have it.

``index.search(x, k, params=SearchParameters(sel=selector))`` is faiss's filtered search: the k
nearest rows among the ids the selector keeps (``IDSelectorRange`` / ``Batch`` / ``Array`` /
``Bitmap`` / ``All`` / ``Not`` / ``And`` / ``Or`` / ``XOr``).  A selector is lowered on the host to
one bitmap over the stored rows and the search walks only the selected rows
(include/imgrec_knn.h knn_search_filtered).  ``range_search`` does not take a selector.

``index.remove_ids(sel_or_ids) -> nremoved`` (faiss ``IndexFlatCodes::remove_ids``) deletes rows in
place: survivors keep their order and are renumbered densely, and the stored rows and every derived
copy are compacted on the device without re-adding anything (include/imgrec_knn.h knn_remove_ids).

================================  =================================================================
beyond the reference's calls      served by
================================  =================================================================
``index.range_search(x, thresh)`` knn_range_search (csrc/knn_range.hip)
``index.search(x, k, params=..)`` knn_search_filtered (csrc/knn_filter.hip)
``index.remove_ids(sel_or_ids)``  knn_remove_ids (csrc/knn_remove.hip)
================================  =================================================================

Semantics: every index class here is an EXACT flat index (the north_star parity target is
``IndexFlatL2``).  ``IndexHNSWFlat`` and ``IndexIVFPQ`` keep their constructor signatures and
attributes (``hnsw.efSearch``, ``nprobe``, ``nlist``, ...) so the reference code runs unchanged,
but they search exactly; their results are therefore the ones the reference's approximate index
approximates.  Results follow faiss conventions: ``D`` float32 (n, k), ``I`` int64 (n, k), rows
sorted best-first, missing neighbours as label -1 with distance FLT_MAX (L2) / -FLT_MAX (IP).
Exact ties are broken by the smaller label.

All arithmetic runs in the HIP kernels; there is no CPU fallback (``NativeLibraryError`` when the
library is missing, ``KnnError`` with the C-ABI message on any failure).

Several GPUs from one process: ``devices=[0, 1, ...]`` on any index class (or on ``read_index``), or
the environment variable ``IMGREC_DEVICES=0,1,...`` for code that cannot pass it — the reference's
own CLI (main/search_from_image.py:430-441) then searches row shards on every listed GPU
(include/imgrec_knn.h knn_create_multi); results are the same as on one device.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

from . import _lib
from ._lib import KNN_MAX_K, KnnError

METRIC_INNER_PRODUCT = 0
METRIC_L2 = 1
METRIC_COSINE = 2   # extension: rows and queries L2-normalised on entry, then inner product

_METRIC_TO_KNN = {METRIC_L2: _lib.KNN_METRIC_L2, METRIC_INNER_PRODUCT: _lib.KNN_METRIC_IP,
                  METRIC_COSINE: _lib.KNN_METRIC_COSINE}
_KNN_TO_METRIC = {v: k for k, v in _METRIC_TO_KNN.items()}


def _as_matrix(x, d: int, what: str) -> np.ndarray:
    """faiss's swig replacement_* wrappers: ``n, d = x.shape; x = ascontiguousarray(x, float32)``."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"{what}: expected a 2-D array, got shape {x.shape}")
    if x.shape[1] != d:
        raise ValueError(f"{what}: array has {x.shape[1]} columns, index dimension is {d}")
    return np.ascontiguousarray(x, dtype=np.float32)


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def _device_list(device: int, devices):
    """The devices an index spans: `devices` if given, else IMGREC_DEVICES when `device` is the
    default (-1), else None (one device)."""
    if devices is None and device == -1 and os.environ.get("IMGREC_DEVICES"):
        devices = [int(v) for v in os.environ["IMGREC_DEVICES"].split(",") if v.strip()]
    if devices is None:
        return None
    devices = [int(v) for v in devices]
    if not devices:
        raise ValueError("devices must list at least one device")
    return devices


# ---- id selectors and search parameters (faiss 1.10 constructors) ---------------------------
class IDSelector:
    """A set of labels.  ``is_member(id)`` tests one; ``to_bitmap(n, offset=0)`` lowers the set to
    faiss IDSelectorBitmap's layout over the labels [offset, offset + n): bit i (byte i >> 3, bit
    i & 7) is ``is_member(offset + i)``, uint8[ceil(n / 8)].  Ids outside that range are silently
    not members."""

    def is_member(self, id: int) -> bool:      # noqa: A002 - faiss's argument name
        raise NotImplementedError

    def _mask(self, n: int, offset: int) -> np.ndarray:
        """bool[n]: membership of the labels offset .. offset + n - 1."""
        raise NotImplementedError

    def to_bitmap(self, n: int, offset: int = 0) -> np.ndarray:
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        return np.packbits(self._mask(n, int(offset)), bitorder="little")


def _id_array(ids, n=None) -> np.ndarray:
    """faiss's (ids) and swig's (n, ids) constructor forms."""
    if n is not None:
        ids, n = n, ids
    a = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
    return a if n is None else a[:int(n)]


class IDSelectorRange(IDSelector):
    """Labels in [imin, imax)."""

    def __init__(self, imin: int, imax: int, assume_sorted: bool = False):
        self.imin, self.imax, self.assume_sorted = int(imin), int(imax), bool(assume_sorted)

    def is_member(self, id: int) -> bool:      # noqa: A002
        return self.imin <= int(id) < self.imax

    def _mask(self, n, offset):
        m = np.zeros(n, dtype=bool)
        lo, hi = max(self.imin - offset, 0), min(self.imax - offset, n)
        if lo < hi:
            m[lo:hi] = True
        return m


class IDSelectorArray(IDSelector):
    """The listed labels (``IDSelectorArray(ids)`` or ``(n, ids)``)."""

    def __init__(self, ids, n=None):
        self.ids = _id_array(ids, n)
        self._set = None

    def is_member(self, id: int) -> bool:      # noqa: A002
        if self._set is None:
            self._set = set(self.ids.tolist())
        return int(id) in self._set

    def _mask(self, n, offset):
        m = np.zeros(n, dtype=bool)
        local = self.ids - offset
        m[local[(local >= 0) & (local < n)]] = True
        return m


class IDSelectorBatch(IDSelectorArray):
    """The listed labels (faiss keeps them in a hash set with a Bloom filter; the set is the same)."""


class IDSelectorBitmap(IDSelector):
    """Label i is a member iff byte i >> 3 exists and its bit i & 7 is set
    (``IDSelectorBitmap(bitmap)`` or ``(nbytes, bitmap)``)."""

    def __init__(self, bitmap, n=None):
        if n is not None:
            bitmap, n = n, bitmap
        b = np.ascontiguousarray(np.asarray(bitmap).reshape(-1), dtype=np.uint8)
        self.bitmap = b if n is None else b[:int(n)]
        self.n = int(self.bitmap.size)

    def is_member(self, id: int) -> bool:      # noqa: A002
        i = int(id)
        return 0 <= (i >> 3) < self.n and bool((int(self.bitmap[i >> 3]) >> (i & 7)) & 1)

    def _mask(self, n, offset):
        m = np.zeros(n, dtype=bool)
        bits = np.unpackbits(self.bitmap, bitorder="little").astype(bool)
        lo, hi = max(offset, 0), min(offset + n, bits.size)
        if lo < hi:
            m[lo - offset:hi - offset] = bits[lo:hi]
        return m


class IDSelectorAll(IDSelector):
    def is_member(self, id: int) -> bool:      # noqa: A002
        return True

    def _mask(self, n, offset):
        return np.ones(n, dtype=bool)


class IDSelectorNot(IDSelector):
    def __init__(self, sel: IDSelector):
        self.sel = sel

    def is_member(self, id: int) -> bool:      # noqa: A002
        return not self.sel.is_member(id)

    def _mask(self, n, offset):
        return ~self.sel._mask(n, offset)


class _IDSelectorPair(IDSelector):
    _op = None

    def __init__(self, lhs: IDSelector, rhs: IDSelector):
        self.lhs, self.rhs = lhs, rhs

    def is_member(self, id: int) -> bool:      # noqa: A002
        return bool(type(self)._op(self.lhs.is_member(id), self.rhs.is_member(id)))

    def _mask(self, n, offset):
        return type(self)._op(self.lhs._mask(n, offset), self.rhs._mask(n, offset))


class IDSelectorAnd(_IDSelectorPair):
    _op = staticmethod(lambda a, b: a & b)


class IDSelectorOr(_IDSelectorPair):
    _op = staticmethod(lambda a, b: a | b)


class IDSelectorXOr(_IDSelectorPair):
    _op = staticmethod(lambda a, b: a ^ b)


class SearchParameters:
    """faiss.SearchParameters: ``sel`` restricts a search to the selector's labels."""

    def __init__(self, sel: IDSelector | None = None):
        self.sel = sel


class SearchParametersIVF(SearchParameters):
    """Constructor-compatible; the extra fields are recorded and ignored (these classes search
    exactly)."""

    def __init__(self, sel=None, nprobe: int = 1, max_codes: int = 0, quantizer_params=None,
                 inverted_list_context=None):
        super().__init__(sel)
        self.nprobe, self.max_codes = int(nprobe), int(max_codes)
        self.quantizer_params, self.inverted_list_context = quantizer_params, inverted_list_context


class SearchParametersHNSW(SearchParameters):
    """Constructor-compatible; the extra fields are recorded and ignored (these classes search
    exactly)."""

    def __init__(self, sel=None, efSearch: int = 16, check_relative_distance: bool = True,
                 bounded_queue: bool = True):
        super().__init__(sel)
        self.efSearch = int(efSearch)
        self.check_relative_distance = bool(check_relative_distance)
        self.bounded_queue = bool(bounded_queue)


def _removal_bitmap(sel_or_ids, ntotal: int, id_offset: int = 0) -> np.ndarray:
    """The bitmap ``remove_ids`` hands to the library: uint8[ceil(ntotal / 8)], bit i set iff the
    stored row i (label ``i + id_offset``) is to be removed.  `sel_or_ids` is an ``IDSelector`` or an
    array of labels (faiss's wrapper turns an array into an ``IDSelectorBatch``); duplicates and
    labels outside the index are ignored."""
    sel = sel_or_ids if isinstance(sel_or_ids, IDSelector) else IDSelectorBatch(sel_or_ids)
    return np.ascontiguousarray(sel.to_bitmap(int(ntotal), int(id_offset)), dtype=np.uint8)


class RangeResult:
    """A range search's device-resident result (include/imgrec_knn.h knn_range_result_t): owns the
    handle and frees it when dropped."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        lib = _lib.load()
        self.nq = int(lib.knn_range_nq(handle))
        self.size = int(lib.knn_range_size(handle))

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_lib, "_lib", None) if _lib is not None else None
        if h is not None and lib is not None:
            lib.knn_range_free(h)
            self._h = None

    def device_ptrs(self):
        """(lims, D, I) device addresses: int64[nq + 1], float32[size], int64[size]; valid while
        this object lives."""
        lims, D, I = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(_lib.load().knn_range_device(self._h, C.byref(lims), C.byref(D), C.byref(I)),
                   "knn_range_device")
        return lims.value or 0, D.value or 0, I.value or 0

    def to_host(self):
        """(lims, D, I) as numpy arrays, faiss's range_search return."""
        lims = np.empty(self.nq + 1, dtype=np.int64)
        D = np.empty(self.size, dtype=np.float32)
        I = np.empty(self.size, dtype=np.int64)
        _lib.check(_lib.load().knn_range_copy(self._h, _ptr(lims), _ptr(D), _ptr(I)),
                   "knn_range_copy")
        return lims, D, I


class Index:
    """Exact flat index on one HIP device, or row-sharded over several (faiss.IndexFlat
    semantics either way)."""

    def __init__(self, d: int, metric: int = METRIC_L2, device: int = -1, devices=None):
        if metric not in _METRIC_TO_KNN:
            raise ValueError(f"unsupported metric {metric}")
        self._h = None
        lib = _lib.load()
        h = C.c_void_p()
        devs = _device_list(device, devices)
        if devs is not None and len(devs) > 1:
            arr = (C.c_int * len(devs))(*devs)
            _lib.check(lib.knn_create_multi(int(d), _METRIC_TO_KNN[metric], arr, len(devs),
                                            C.byref(h)), "knn_create_multi")
        else:
            dev = devs[0] if devs else device
            _lib.check(lib.knn_create(int(d), _METRIC_TO_KNN[metric], int(dev), C.byref(h)),
                       "knn_create")
        self._h = h
        self.d = int(d)
        self.metric_type = metric
        self.verbose = False

    @classmethod
    def _wrap(cls, handle: C.c_void_p) -> "Index":
        obj = cls.__new__(cls)
        lib = _lib.load()
        obj._h = handle
        obj.d = lib.knn_dim(handle)
        obj.metric_type = _KNN_TO_METRIC[lib.knn_metric(handle)]
        obj.verbose = False
        return obj

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_lib, "_lib", None) if _lib is not None else None
        if h is not None and lib is not None:
            lib.knn_free(h)
            self._h = None

    # ---- faiss attributes -------------------------------------------------------------------
    @property
    def ntotal(self) -> int:
        return int(_lib.load().knn_ntotal(self._h))

    @property
    def is_trained(self) -> bool:
        return bool(_lib.load().knn_is_trained(self._h))

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    @property
    def num_shards(self) -> int:
        """Row shards (devices) the index spans: 1 unless created with several devices."""
        return int(_lib.load().knn_num_shards(self._h))

    # ---- faiss methods ----------------------------------------------------------------------
    def train(self, x) -> None:
        x = _as_matrix(x, self.d, "train")
        _lib.check(_lib.load().knn_train(self._h, _ptr(x), x.shape[0]), "knn_train")

    def add(self, x) -> None:
        x = _as_matrix(x, self.d, "add")
        if not self.is_trained:
            raise RuntimeError("Error in add: index is not trained (call train first)")
        _lib.check(_lib.load().knn_add(self._h, _ptr(x), x.shape[0]), "knn_add")

    def search(self, x, k: int, *, params=None, D=None, I=None):
        """faiss ``index.search(x, k[, params=SearchParameters(sel=...)])``.  With a selector the
        result is the k nearest among the selected labels (label -1 past their number), from the
        filtered kernels (include/imgrec_knn.h knn_search_filtered); without one nothing changes."""
        x = _as_matrix(x, self.d, "search")
        k = int(k)
        if k <= 0:
            raise ValueError("k must be positive")
        n = x.shape[0]
        D = np.empty((n, k), dtype=np.float32) if D is None else D
        I = np.empty((n, k), dtype=np.int64) if I is None else I
        if D.shape != (n, k) or I.shape != (n, k) or D.dtype != np.float32 or I.dtype != np.int64 \
                or not D.flags.c_contiguous or not I.flags.c_contiguous:
            raise ValueError("D/I must be C-contiguous float32/int64 arrays of shape (n, k)")
        sel = getattr(params, "sel", None)
        if n and sel is not None:
            nbits = self.ntotal
            bitmap = np.ascontiguousarray(sel.to_bitmap(nbits, getattr(self, "_id_offset", 0)),
                                          dtype=np.uint8)
            _lib.check(_lib.load().knn_search_filtered(self._h, _ptr(x), n, k, _ptr(bitmap), nbits,
                                                       _ptr(D), _ptr(I)), "knn_search_filtered")
        elif n:
            _lib.check(_lib.load().knn_search(self._h, _ptr(x), n, k, _ptr(D), _ptr(I)),
                       "knn_search")
        return D, I

    def range_search(self, x, thresh: float, *, params=None):
        """faiss ``index.range_search(x, thresh) -> (lims, D, I)``: every stored row with squared
        L2 distance < thresh (L2) or inner product > thresh (IP / cosine).  Query i's hits are
        ``D[lims[i]:lims[i+1]]`` / ``I[lims[i]:lims[i+1]]``, best first, exact ties by the smaller
        label (faiss leaves the order unspecified), so a k-prefix of a segment is a top-k.
        A selector in ``params`` is not supported here."""
        if getattr(params, "sel", None) is not None:
            raise NotImplementedError("range_search does not take an id selector; the filtered form "
                                      "that exists is search(x, k, params=SearchParameters(sel=...))")
        x = _as_matrix(x, self.d, "range_search")
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.knn_range_search(self._h, _ptr(x), x.shape[0], float(thresh), C.byref(h)),
                   "knn_range_search")
        return RangeResult(h).to_host()

    def range_search_device(self, q_ptr: int, nq: int, thresh: float, stream: int = 0) -> "RangeResult":
        """range_search over nq device-resident queries on `stream`; the result stays on the
        index's device (``RangeResult.device_ptrs()``) until the returned object is dropped."""
        h = C.c_void_p()
        _lib.check(_lib.load().knn_range_search_device(self._h, C.c_void_p(q_ptr), int(nq),
                                                       float(thresh), C.c_void_p(stream or None),
                                                       C.byref(h)), "knn_range_search_device")
        return RangeResult(h)

    def reset(self) -> None:
        _lib.check(_lib.load().knn_reset(self._h), "knn_reset")

    def remove_ids(self, sel) -> int:
        """faiss ``index.remove_ids(sel) -> nremoved``: the rows whose labels an ``IDSelector`` (or
        an array of labels) names leave the index.  Survivors keep their order and their labels
        become dense again (row offset + id offset), as in faiss's flat indexes.  The removal runs
        in place on the device (include/imgrec_knn.h knn_remove_ids), multi-device indexes included.
        Out of scope: ``sharded.ShardedIndex`` and ``ivfpq`` have no ``remove_ids``."""
        nbits = self.ntotal
        bitmap = _removal_bitmap(sel, nbits, getattr(self, "_id_offset", 0))
        removed = C.c_int64()
        _lib.check(_lib.load().knn_remove_ids(self._h, _ptr(bitmap), nbits, C.byref(removed)),
                   "knn_remove_ids")
        return int(removed.value)

    def reconstruct_n(self, i0: int = 0, n: int | None = None) -> np.ndarray:
        n = self.ntotal - i0 if n is None else n
        out = np.empty((n, self.d), dtype=np.float32)
        _lib.check(_lib.load().knn_reconstruct_n(self._h, int(i0), int(n), _ptr(out)),
                   "knn_reconstruct_n")
        return out

    def reconstruct(self, key: int) -> np.ndarray:
        return self.reconstruct_n(int(key), 1)[0]

    # ---- device-resident entry points (multi-GPU shards, bench) ---------------------------------
    def add_device(self, x_ptr: int, n: int, stream: int = 0) -> None:
        _lib.check(_lib.load().knn_add_device(self._h, C.c_void_p(x_ptr), int(n),
                                              C.c_void_p(stream or None)), "knn_add_device")

    def search_device(self, q_ptr: int, nq: int, k: int, d_ptr: int, i_ptr: int,
                      stream: int = 0) -> None:
        _lib.check(_lib.load().knn_search_device(self._h, C.c_void_p(q_ptr), int(nq), int(k),
                                                 C.c_void_p(d_ptr), C.c_void_p(i_ptr),
                                                 C.c_void_p(stream or None)), "knn_search_device")

    def search_filtered_device(self, q_ptr: int, nq: int, k: int, bitmap_ptr: int, nbits: int,
                               d_ptr: int, i_ptr: int, stream: int = 0) -> None:
        """The filtered search over device-resident queries, bitmap (over the stored rows: bit i is
        row i, label i + id offset) and outputs on `stream`; never waits while k <= KNN_MAX_K."""
        _lib.check(_lib.load().knn_search_filtered_device(
            self._h, C.c_void_p(q_ptr), int(nq), int(k), C.c_void_p(bitmap_ptr or None), int(nbits),
            C.c_void_p(d_ptr), C.c_void_p(i_ptr), C.c_void_p(stream or None)),
            "knn_search_filtered_device")

    def set_id_offset(self, off: int) -> None:
        _lib.check(_lib.load().knn_set_id_offset(self._h, int(off)), "knn_set_id_offset")
        self._id_offset = int(off)      # selectors speak labels: lowered with this offset

    def reserve(self, n: int) -> None:
        _lib.check(_lib.load().knn_reserve(self._h, int(n)), "knn_reserve")

    def set_fence_mode(self, lazy: bool) -> None:
        """Cross-stream fence of the *_device calls (include/imgrec_knn.h knn_set_fence_mode):
        lazy=True records no event while every call uses one stream, which must then stay valid
        until the next call on the index."""
        mode = _lib.KNN_FENCE_LAZY if lazy else _lib.KNN_FENCE_EAGER
        _lib.check(_lib.load().knn_set_fence_mode(self._h, mode), "knn_set_fence_mode")

    # -- search arithmetic (extension; include/imgrec_knn.h knn_search_mode) -------------------
    SEARCH_MODES = {"auto": _lib.KNN_SEARCH_AUTO, "exact": _lib.KNN_SEARCH_EXACT,
                    "split": _lib.KNN_SEARCH_SPLIT, "bf16": _lib.KNN_SEARCH_BF16,
                    "i8": _lib.KNN_SEARCH_I8}

    @property
    def search_mode(self) -> str:
        return getattr(self, "_mode", "auto")

    @search_mode.setter
    def search_mode(self, mode: str) -> None:
        if mode not in self.SEARCH_MODES:
            raise ValueError(f"search_mode must be one of {sorted(self.SEARCH_MODES)}")
        _lib.check(_lib.load().knn_set_search_mode(self._h, self.SEARCH_MODES[mode]),
                   "knn_set_search_mode")
        self._mode = mode

    def search_stats(self, with_error: bool = False):
        """(queries of the last search on a candidate path (split / bf16), of which re-run on the
        exact kernel because no certificate held)
        [+ largest observed approximation error / certificate bound, with_error=True]."""
        st = self.certificate_stats()
        return ((st["candidate_queries"], st["exact_reruns"], st["max_err_over_bound"])
                if with_error else (st["candidate_queries"], st["exact_reruns"]))

    def certificate_stats(self) -> dict:
        """The last search's certificate counts: queries on a candidate path, queries the second
        chance (all per-split list entries reranked) certified, queries re-run exactly, and the
        largest observed error / bound.  Waits for that search to finish.

        On the int8 direct route (batches of <= 4 queries, RerankArgs::direct: no merge and no
        first rerank) every query goes straight to the second chance, so there `second_chance +
        exact_reruns` equals the batch size by construction; it does not mean a first-pass
        certificate failed."""
        a, b, c, r = C.c_int64(), C.c_int64(), C.c_int64(), C.c_float()
        _lib.check(_lib.load().knn_search_stats2(self._h, C.byref(a), C.byref(b), C.byref(c),
                                                 C.byref(r)), "knn_search_stats2")
        return {"candidate_queries": a.value, "second_chance": c.value, "exact_reruns": b.value,
                "max_err_over_bound": r.value}


class IndexFlat(Index):
    def __init__(self, d: int, metric: int = METRIC_L2, device: int = -1, devices=None):
        super().__init__(d, metric, device, devices)


class IndexFlatL2(Index):
    def __init__(self, d: int, device: int = -1, devices=None):
        super().__init__(d, METRIC_L2, device, devices)


class IndexFlatIP(Index):
    def __init__(self, d: int, device: int = -1, devices=None):
        super().__init__(d, METRIC_INNER_PRODUCT, device, devices)


class IndexHNSWFlat(IndexFlatL2):
    """Constructor-compatible with ``faiss.IndexHNSWFlat(d, M[, metric])``; searches exactly.

    ``hnsw.efConstruction`` / ``hnsw.efSearch`` / ``hnsw.max_level`` are accepted and recorded
    (main/create_index.py:220-221, 231-232) but have no effect on an exact search.
    """

    def __init__(self, d: int, M: int = 32, metric: int = METRIC_L2, device: int = -1,
                 devices=None):
        Index.__init__(self, d, metric, device, devices)
        self.hnsw = SimpleNamespace(efConstruction=40, efSearch=16, max_level=0, M=int(M))


class IndexIVFPQ(Index):
    """Constructor-compatible with ``faiss.IndexIVFPQ(quantizer, d, nlist, m, nbits)``
    (main/create_index.py:226); searches exactly (nprobe is recorded, not used).

    Like faiss it starts untrained, so the reference's ``if not index.is_trained: train`` runs.
    """

    def __init__(self, quantizer, d: int, nlist: int, m: int, nbits: int = 8,
                 metric: int = METRIC_L2, device: int = -1, devices=None):
        if d % m != 0:
            raise ValueError(f"IndexIVFPQ: d={d} is not a multiple of m={m}")
        Index.__init__(self, d, metric, device, devices)
        self.quantizer = quantizer
        self.nlist, self.pq_m, self.pq_nbits = int(nlist), int(m), int(nbits)
        self.nprobe = 1
        self._trained = False

    @property
    def is_trained(self) -> bool:
        return self._trained

    def train(self, x) -> None:
        super().train(x)
        self._trained = True


class Kmeans:
    """``faiss.Kmeans(d, k, **clustering_parameters)``: Lloyd k-means on the HIP step kernels
    (include/imgrec_kmeans.h, csrc/knn_kmeans.hip).

    The algorithm is faiss's ``Clustering::train``: per run an initialisation, then ``niter``
    times an assignment (exact fp32, ties to the smaller centroid id), the means, faiss's
    empty-cluster split (a donor drawn in proportion to its size, rows scaled by 1 +- 1/1024) and,
    with ``spherical``, a row normalisation; the recorded objective of an iteration is the one of
    its assignment, before the update; of ``nredo`` runs the best final objective is kept.

    The random stream is not faiss's: the initial centroids are a seeded sample of k distinct
    training rows (``std::mt19937_64(seed + run)``), and the subsample of more than
    ``k * max_points_per_centroid`` rows is a seeded numpy permutation.  faiss itself is not a
    dependency of this project, so bit parity with faiss's own runs is not pinned by any test.
    With ``init_centroids`` given and no empty cluster the result depends on no random number, and
    two runs on the same input give the same bytes (the update uses no float atomics).

    ``gpu`` is accepted and ignored (the reference passes ``gpu=True``): everything runs on the
    GPU.  ``int_centroids``, ``frozen_centroids`` and ``train(weights=...)`` are not implemented.

    After ``train``: ``centroids`` (k, d) float32, ``obj`` (niter,) the objective per iteration,
    ``iteration_stats`` (dicts of ``obj``, ``time``, ``time_search``, ``imbalance_factor``,
    ``nsplit``, plus the step's GPU milliseconds ``ms_assign`` / ``ms_sort`` / ``ms_update``) and
    ``index``, an ``IndexFlatL2`` (``IndexFlatIP`` when spherical) holding the centroids.
    """

    def __init__(self, d: int, k: int, niter: int = 25, nredo: int = 1, verbose: bool = False,
                 spherical: bool = False, min_points_per_centroid: int = 39,
                 max_points_per_centroid: int = 256, seed: int = 1234, gpu=False,
                 update_index: bool = False, device: int = -1, int_centroids: bool = False,
                 frozen_centroids: bool = False, decode_block_size: int = 32768):
        if int_centroids:
            raise NotImplementedError("Kmeans: int_centroids=True (centroids rounded to integers) "
                                      "is not implemented.")
        if frozen_centroids:
            raise NotImplementedError("Kmeans: frozen_centroids=True (initial centroids kept fixed) "
                                      "is not implemented.")
        self.d, self.k = int(d), int(k)
        if self.d <= 0 or self.k <= 0:
            raise ValueError(f"Kmeans: d and k must be positive (got d={d}, k={k})")
        self.niter, self.nredo = int(niter), int(nredo)
        if self.niter <= 0 or self.nredo <= 0:
            raise ValueError(f"Kmeans: niter and nredo must be positive (got {niter}, {nredo})")
        self.verbose, self.spherical = bool(verbose), bool(spherical)
        self.min_points_per_centroid = int(min_points_per_centroid)
        self.max_points_per_centroid = int(max_points_per_centroid)
        self.seed, self.gpu, self.update_index = int(seed), gpu, bool(update_index)
        self.device = int(device)
        self.decode_block_size = int(decode_block_size)
        self.centroids = None
        self.obj = None
        self.iteration_stats = None
        self.index = None

    def _params(self) -> "_lib.KmeansParams":
        return _lib.KmeansParams(self.niter, self.nredo, int(self.spherical), int(self.verbose),
                                 self.seed, self.device)

    def _init(self, init_centroids):
        if init_centroids is None:
            return None
        c = np.ascontiguousarray(init_centroids, dtype=np.float32)
        if c.shape != (self.k, self.d):
            raise ValueError(f"init_centroids must have shape ({self.k}, {self.d}), got {c.shape}")
        return c

    def _finish(self, centroids, obj, stats) -> float:
        self.centroids = centroids
        st = stats.reshape(self.niter, _lib.KMEANS_STATS_PER_ITER)
        self.obj = st[:, 0].copy()
        self.iteration_stats = [
            {"obj": float(r[0]), "time": float(r[1]), "time_search": float(r[2]),
             "imbalance_factor": float(r[3]), "nsplit": int(r[4]), "ms_assign": float(r[5]),
             "ms_sort": float(r[6]), "ms_update": float(r[7])} for r in st]
        cls = IndexFlatIP if self.spherical else IndexFlatL2
        self.index = cls(self.d, device=self.device)
        self.index.add(centroids)
        return float(obj)

    def train(self, x, weights=None, init_centroids=None) -> float:
        """Cluster the rows of x; returns the last iteration's objective."""
        if weights is not None:
            raise NotImplementedError("Kmeans.train: per-row weights are not implemented.")
        x = _as_matrix(x, self.d, "Kmeans.train")
        n, k = x.shape[0], self.k
        if n < k:
            raise RuntimeError(f"Number of training points ({n}) should be at least as large as "
                               f"number of clusters ({k})")
        c0 = self._init(init_centroids)
        if n > k * self.max_points_per_centroid:
            keep = k * self.max_points_per_centroid
            if self.verbose:
                print(f"Sampling a subset of {keep} / {n} for training")
            perm = np.random.RandomState(self.seed).permutation(n)[:keep]
            x = np.ascontiguousarray(x[perm])
            n = keep
        elif n < k * self.min_points_per_centroid:
            import warnings
            warnings.warn(f"clustering {n} points to {k} centroids: please provide at least "
                          f"{k * self.min_points_per_centroid} training points", stacklevel=2)
        centroids = np.empty((k, self.d), dtype=np.float32)
        stats = np.zeros(self.niter * _lib.KMEANS_STATS_PER_ITER, dtype=np.float64)
        obj = C.c_double()
        prm = self._params()
        _lib.check(_lib.load().kmeans_train(_ptr(x), n, self.d, k, C.byref(prm),
                                            None if c0 is None else _ptr(c0), _ptr(centroids),
                                            C.byref(obj), _ptr(stats)), "kmeans_train")
        return self._finish(centroids, obj.value, stats)

    def train_device(self, x_ptr: int, n: int, stream: int = 0, init_centroids=None) -> float:
        """``train`` over n device-resident rows (row-major float32, on the current device) on
        `stream`: no subsampling and no copy of the rows; waits for the result."""
        n = int(n)
        if n < self.k:
            raise RuntimeError(f"Number of training points ({n}) should be at least as large as "
                               f"number of clusters ({self.k})")
        c0 = self._init(init_centroids)
        centroids = np.empty((self.k, self.d), dtype=np.float32)
        stats = np.zeros(self.niter * _lib.KMEANS_STATS_PER_ITER, dtype=np.float64)
        obj = C.c_double()
        prm = self._params()
        _lib.check(_lib.load().kmeans_train_device(C.c_void_p(x_ptr), n, self.d, self.k, C.byref(prm),
                                                   None if c0 is None else _ptr(c0), _ptr(centroids),
                                                   C.byref(obj), _ptr(stats),
                                                   C.c_void_p(stream or None)), "kmeans_train_device")
        return self._finish(centroids, obj.value, stats)

    def assign(self, x):
        """(D.ravel(), I.ravel()) of ``index.search(x, 1)``, as in faiss."""
        if self.centroids is None:
            raise RuntimeError("should train before assigning")
        D, I = self.index.search(x, 1)
        return D.ravel(), I.ravel()


def normalize_L2(x: np.ndarray) -> None:
    """In-place row L2 normalisation (faiss.normalize_L2; rows with norm 0 are left unchanged)."""
    if not isinstance(x, np.ndarray) or x.dtype != np.float32 or not x.flags.c_contiguous:
        raise TypeError("normalize_L2 expects a C-contiguous float32 numpy array")
    if x.ndim == 1:
        n, d = 1, x.shape[0]
    elif x.ndim == 2:
        n, d = x.shape
    else:
        raise ValueError("normalize_L2 expects a 1-D or 2-D array")
    if n and d:
        _lib.check(_lib.load().knn_normalize_L2(_ptr(x), n, d), "knn_normalize_L2")


def write_index(index: Index, fname) -> None:
    """Write in faiss's IndexFlat layout (fourcc IxF2 / IxFI), readable by faiss.read_index."""
    _lib.check(_lib.load().knn_write(index.handle, str(fname).encode()), "knn_write")


def read_index(fname, device: int = -1, devices=None) -> Index:
    h = C.c_void_p()
    devs = _device_list(device, devices)
    if devs is not None and len(devs) > 1:
        arr = (C.c_int * len(devs))(*devs)
        rc = _lib.load().knn_read_multi(str(fname).encode(), arr, len(devs), C.byref(h))
    else:
        rc = _lib.load().knn_read(str(fname).encode(), int(devs[0] if devs else device), C.byref(h))
    if rc < 0:
        # faiss raises RuntimeError from read_index; the recommender logs and returns None
        raise KnnError(f"read_index({fname}) failed (code {rc}): {_lib.last_error()}")
    m = _lib.load().knn_metric(h)
    cls = IndexFlatL2 if m == _lib.KNN_METRIC_L2 else (IndexFlatIP if m == _lib.KNN_METRIC_IP
                                                       else IndexFlat)
    return cls._wrap(h)


__all__ = ["IDSelector", "IDSelectorRange", "IDSelectorBatch", "IDSelectorArray", "IDSelectorBitmap",
           "IDSelectorAll", "IDSelectorNot", "IDSelectorAnd", "IDSelectorOr", "IDSelectorXOr",
           "SearchParameters", "SearchParametersIVF", "SearchParametersHNSW",
           "Index", "RangeResult", "IndexFlat", "IndexFlatL2", "IndexFlatIP", "IndexHNSWFlat", "IndexIVFPQ",
           "Kmeans", "normalize_L2", "read_index", "write_index", "METRIC_L2", "METRIC_INNER_PRODUCT",
           "METRIC_COSINE", "KnnError"]
