"""Soft-assignment VLAD of local descriptors (include/imgrec_vlad.h, csrc/vlad.hip).

The reference's SIFT-VLAD extractor (``vector_scripts/create_sift_vector.py``) aggregates every
image's RootSIFT descriptors against a k-means vocabulary: the ``nn`` nearest words of a descriptor,
a weight ``exp(-dist / (2 sigma^2))`` each, the weighted residuals summed per word, then a per-word
L2 normalisation, a signed square root and a global L2 normalisation
(``_compute_sift_vlad_worker``, ``:448-475``).  ``SoftVLAD.encode`` runs that loop for a ragged
batch of images in HIP kernels; the search is exact where the reference's HNSW approximates it.

    km = faiss_compat.Kmeans(128, 256, niter=25); km.train(all_descriptors)
    enc = SoftVLAD.from_kmeans(km)                      # nn=4, sigma=125.0: the reference's values
    vectors = enc.encode([rootsift(d) for d in per_image_descriptors])     # (nimg, 32768) float32

There is no NumPy fallback: without the native library every call raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KnnError, VLAD_MAX_D, VLAD_MAX_NN, VLAD_RAW

__all__ = ["SoftVLAD", "rootsift", "KnnError"]


def rootsift(desc) -> np.ndarray:
    """RootSIFT of ``(n, d)`` descriptors, the reference's three lines: L1-normalise (+1e-7), square
    root, L2-normalise (+1e-7)."""
    desc = np.asarray(desc, dtype=np.float32)
    desc = desc / (np.linalg.norm(desc, ord=1, axis=1, keepdims=True) + 1e-7)
    desc = np.sqrt(desc)
    desc = desc / (np.linalg.norm(desc, axis=1, keepdims=True) + 1e-7)
    return desc.astype(np.float32, copy=False)


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


class SoftVLAD:
    """The encoder of one codebook.  ``nn`` neighbours per descriptor (1 = plain VLAD with a weight),
    ``sigma`` the weight's scale, ``device`` the HIP device of ``encode`` (-1 = current)."""

    def __init__(self, codebook, nn: int = 4, sigma: float = 125.0, device: int = -1):
        codebook = np.asarray(codebook)
        if codebook.ndim != 2 or codebook.shape[0] < 1 or codebook.shape[1] < 1:
            raise ValueError(f"codebook: expected a (k, d) array, got shape {codebook.shape}")
        self.codebook = np.array(codebook, dtype=np.float32, order="C")      # a copy of its own
        self.k, self.d = (int(v) for v in self.codebook.shape)
        if self.d > VLAD_MAX_D:
            raise ValueError(f"codebook: d = {self.d} exceeds {VLAD_MAX_D}")
        self.nn = int(nn)
        if not 1 <= self.nn <= VLAD_MAX_NN:
            raise ValueError(f"nn must be in [1, {VLAD_MAX_NN}] (got {nn})")
        if self.nn > self.k:
            raise ValueError(f"nn = {self.nn} exceeds the codebook's {self.k} rows")
        self.sigma = float(sigma)
        if not (self.sigma > 0.0 and np.isfinite(self.sigma)):
            raise ValueError(f"sigma must be positive and finite (got {sigma})")
        self.device = int(device)
        self._codebook_dev = None       # (device, torch tensor) for encode_device

    @classmethod
    def from_kmeans(cls, km, nn: int = 4, sigma: float = 125.0, device: int = -1) -> "SoftVLAD":
        """From a trained ``faiss_compat.Kmeans`` (its ``centroids``)."""
        if getattr(km, "centroids", None) is None:
            raise ValueError("from_kmeans: train the Kmeans first (centroids is None)")
        return cls(km.centroids, nn=nn, sigma=sigma, device=device)

    @property
    def dim(self) -> int:
        return self.k * self.d

    # ---- host arrays --------------------------------------------------------------------------
    def _ragged(self, descs):
        """(X (N, d) float32, offsets int64[nimg + 1]) from a list of (n_i, d) arrays or an (X, offsets) pair."""
        if isinstance(descs, tuple) and len(descs) == 2 and np.ndim(descs[1]) == 1 and np.ndim(descs[0]) == 2 \
                and np.issubdtype(np.asarray(descs[1]).dtype, np.integer):
            x = np.asarray(descs[0])
            if x.shape[1] != self.d:
                raise ValueError(f"descriptors have {x.shape[1]} columns, the codebook has {self.d}")
            off = np.ascontiguousarray(descs[1], dtype=np.int64)
            if off.size < 1 or off[0] != 0 or off[-1] != x.shape[0] or (np.diff(off) < 0).any():
                raise ValueError("offsets must start at 0, never decrease and end at the number of descriptors")
            return np.ascontiguousarray(x, dtype=np.float32), off
        parts = []
        for i, a in enumerate(descs):
            a = np.asarray(a)
            if a.size == 0:
                a = a.reshape(0, self.d)
            if a.ndim != 2 or a.shape[1] != self.d:
                raise ValueError(f"image {i}: expected an (n, {self.d}) array, got shape {a.shape}")
            parts.append(np.asarray(a, dtype=np.float32))
        off = np.zeros(len(parts) + 1, np.int64)
        if parts:
            np.cumsum([p.shape[0] for p in parts], out=off[1:])
            x = np.ascontiguousarray(np.concatenate(parts, axis=0))
        else:
            x = np.zeros((0, self.d), np.float32)
        return x, off

    def encode(self, descs, raw: bool = False, return_assignment: bool = False):
        """``descs``: a list of ``(n_i, d)`` arrays (empty images allowed) or a pair ``(X, offsets)``.
        Returns ``(nimg, k * d)`` float32; with ``return_assignment`` also ``(nn_idx, nn_dist)``, each
        ``(N, nn)``.  ``raw`` skips the three normalisations."""
        x, off = self._ragged(descs)
        n, nimg = int(x.shape[0]), int(off.size - 1)
        out = np.empty((nimg, self.dim), np.float32)
        idx = np.empty((n, self.nn), np.int32) if return_assignment else None
        dist = np.empty((n, self.nn), np.float32) if return_assignment else None
        _lib.check(_lib.load().vlad_encode(
            _ptr(x), n, _ptr(off), nimg, self.d, _ptr(self.codebook), self.k, self.nn, self.sigma,
            VLAD_RAW if raw else 0, _ptr(out), _ptr(idx) if return_assignment else None,
            _ptr(dist) if return_assignment else None, self.device), "vlad_encode")
        return (out, idx, dist) if return_assignment else out

    # ---- device-resident ----------------------------------------------------------------------
    def codebook_device(self) -> int:
        """The device pointer of a copy of the codebook on the current torch device (made once)."""
        import torch
        dev = torch.cuda.current_device()
        if self._codebook_dev is None or self._codebook_dev[0] != dev:
            self._codebook_dev = (dev, torch.from_numpy(self.codebook).cuda())
        return self._codebook_dev[1].data_ptr()

    def encode_device(self, x_ptr: int, offsets_ptr: int, nimg: int, N: int, out_ptr: int, stream: int = 0,
                      raw: bool = False, nn_idx_ptr: int = 0, nn_dist_ptr: int = 0, codebook_ptr: int = 0) -> None:
        """The encoding over device-resident descriptors (N x d float32), offsets (int64[nimg + 1])
        and output (nimg x k*d float32) on `stream`; never waits.  The codebook is `codebook_ptr`, or
        this encoder's own device copy (uploaded on first use through torch)."""
        _lib.check(_lib.load().vlad_encode_device(
            C.c_void_p(x_ptr or None), int(N), C.c_void_p(offsets_ptr or None), int(nimg), self.d,
            C.c_void_p(codebook_ptr or self.codebook_device()), self.k, self.nn, self.sigma,
            VLAD_RAW if raw else 0, C.c_void_p(out_ptr or None), C.c_void_p(nn_idx_ptr or None),
            C.c_void_p(nn_dist_ptr or None), C.c_void_p(stream or None)), "vlad_encode_device")
