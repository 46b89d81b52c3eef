"""Pillow's 8-bit LANCZOS resize on the MI355X (csrc/resize.hip, include/imgrec_resize.h).

``Image.resize(size, LANCZOS)`` — the first step of every feature the reference extracts
(``load_image(..., img_size=...)``) — for a ragged batch of decoded images, bit for bit: the
weight tables are built on the host in double as Pillow builds them, the two passes run as HIP
kernels.  ``size`` is ``(width, height)``, as in Pillow.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib

FORMATS = {"u8": _lib.RESIZE_U8_HWC, "f32": _lib.RESIZE_F32_CHW}
PACK_ALIGN = 48      # the decode ring's slot alignment: whole RGB pixels and whole 16-byte vectors


def _error(what: str, rc: int) -> _lib.KnnError:
    return _lib.KnnError(f"{what} failed ({rc}): {_lib.load().resize_last_error().decode()}")


def _as_image(im) -> np.ndarray:
    a = np.asarray(im)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)):
        raise ValueError(f"expected HxWx3, HxWx1 or HxW uint8 images, got {a.shape} {a.dtype}")
    return np.ascontiguousarray(a)


def pack_images(images: Sequence[np.ndarray], align: int = PACK_ALIGN):
    """One byte buffer of the images, each at a multiple of ``align``: (buffer, offsets int64,
    shapes int32 (n, 2) of (height, width), channels)."""
    arrs = [_as_image(im) for im in images]
    chans = {1 if a.ndim == 2 else a.shape[2] for a in arrs}
    if len(chans) > 1:
        raise ValueError("the images of one batch must have the same number of channels")
    channels = chans.pop() if chans else 3
    offsets = np.zeros(len(arrs), np.int64)
    pos = 0
    for i, a in enumerate(arrs):
        offsets[i] = pos
        pos += -(-a.nbytes // align) * align
    buf = np.zeros(max(pos, 1), np.uint8)
    for a, o in zip(arrs, offsets):
        buf[o:o + a.nbytes] = a.reshape(-1)
    shapes = np.array([a.shape[:2] for a in arrs], np.int32).reshape(len(arrs), 2)
    return buf, offsets, shapes, channels


def lanczos_resize_device(pixels, offsets, shapes, size, fmt: str = "u8", out=None, stream=None,
                          channels: int = 3):
    """Resize images that already lie in a torch uint8 tensor on a HIP device.

    pixels: 1-D uint8 tensor; offsets: n byte offsets of the HWC images in it (host integers);
    shapes: n (height, width) pairs (host integers).  Returns (n, out_h, out_w, channels) uint8
    for fmt "u8", (n, channels, out_h, out_w) float32 in [0, 1] for "f32"; ``out`` (contiguous,
    of that shape and dtype, on the same device) receives the result when given.  Enqueued on
    ``stream`` (a torch stream; default: the current one), no synchronisation."""
    import torch
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    if pixels.dtype != torch.uint8 or not pixels.is_cuda or not pixels.is_contiguous():
        raise ValueError("pixels must be a contiguous uint8 tensor on a HIP device")
    out_w, out_h = int(size[0]), int(size[1])
    offs = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
    hw = np.ascontiguousarray(np.asarray(shapes, np.int32).reshape(-1, 2))
    n = int(offs.shape[0])
    if hw.shape[0] != n:
        raise ValueError("offsets and shapes differ in length")
    heights, widths = np.ascontiguousarray(hw[:, 0]), np.ascontiguousarray(hw[:, 1])
    if n and (offs.min() < 0 or int((offs + heights.astype(np.int64) * widths * channels).max()) > pixels.numel()):
        raise ValueError("an image lies outside the pixel tensor")
    shape = (n, out_h, out_w, channels) if fmt == "u8" else (n, channels, out_h, out_w)
    dtype = torch.uint8 if fmt == "u8" else torch.float32
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=pixels.device)
    elif (tuple(out.shape) != shape or out.dtype != dtype or out.device != pixels.device
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape} on {pixels.device}")
    st = stream if stream is not None else torch.cuda.current_stream(pixels.device)
    with torch.cuda.device(pixels.device):
        rc = _lib.load().resize_lanczos_device(
            C.c_void_p(pixels.data_ptr()), offs.ctypes.data, heights.ctypes.data, widths.ctypes.data,
            n, int(channels), out_h, out_w, FORMATS[fmt], C.c_void_p(out.data_ptr()),
            C.c_void_p(st.cuda_stream or None))
    if rc != 0:
        raise _error("resize_lanczos_device", rc)
    return out


def lanczos_resize(images: Sequence[np.ndarray], size, fmt: str = "u8", device=None) -> np.ndarray:
    """Resize HxWx3 (or HxW) uint8 arrays of any sizes on the GPU: packs them, uploads once,
    resizes, copies back.  (n, out_h, out_w, 3) uint8 ((n, out_h, out_w) for HxW inputs) for fmt
    "u8"; (n, channels, out_h, out_w) float32 in [0, 1] for "f32"."""
    import torch
    if not torch.cuda.is_available():
        raise _lib.NativeLibraryError("lanczos_resize needs a HIP device; lanczos_resize_host runs on the CPU")
    gray = len(images) > 0 and all(np.asarray(im).ndim == 2 for im in images)
    buf, offsets, shapes, channels = pack_images(images)
    dev = torch.device(device if device is not None else "cuda")
    pixels = torch.from_numpy(buf).to(dev)
    out = lanczos_resize_device(pixels, offsets, shapes, size, fmt, channels=channels).cpu().numpy()
    return out[..., 0] if (gray and fmt == "u8") else out


def lanczos_resize_host(image: np.ndarray, size) -> np.ndarray:
    """One image through the library's CPU statement of the arithmetic (resize_lanczos_host)."""
    a = _as_image(image)
    channels = 1 if a.ndim == 2 else a.shape[2]
    out_w, out_h = int(size[0]), int(size[1])
    if out_w <= 0 or out_h <= 0:
        raise ValueError(f"size must be positive, got {size}")
    out = np.empty((out_h, out_w) if a.ndim == 2 else (out_h, out_w, channels), np.uint8)
    rc = _lib.load().resize_lanczos_host(a.ctypes.data, a.shape[0], a.shape[1], channels, out_h, out_w,
                                         out.ctypes.data)
    if rc != 0:
        raise _error("resize_lanczos_host", rc)
    return out
