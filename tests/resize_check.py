"""A numpy restatement of Pillow's 8-bit LANCZOS resize (Resample.c, box = the whole image),
independent of the library: the checker of tests/test_resize_cpu.py and tests/test_resize_gpu.py.

Per axis: scale = in / out, fs = max(scale, 1), support = 3 fs; for output index xx the window
starts at xmin = max(int(center - support + 0.5), 0) with center = (xx + 0.5) scale and holds
n = min(int(center + support + 0.5), in) - xmin taps w[j] = L((j + xmin - center + 0.5) / fs),
L(x) = sinc(x) sinc(x / 3) on [-3, 3); the weights are normalised by their sum (accumulated in
order) and rounded to 22 fractional bits away from zero at the half.  A byte is
clamp((2^21 + sum px k) >> 22, 0, 255) in int32.  Horizontal first, rounded to uint8, then
vertical; a pass with in == out is skipped.
"""
from __future__ import annotations

import math

import numpy as np

# (h, w) -> (out_w, out_h): the cases of the CPU and the GPU tests
CASES = [
    ((7, 5), (4, 3)),            # smallest general case
    ((1, 1), (8, 8)),            # windows clipped to a single pixel
    ((64, 64), (64, 64)),        # both passes skipped
    ((224, 300), (224, 224)),    # horizontal pass only
    ((300, 224), (224, 224)),    # vertical pass only
    ((100, 90), (224, 224)),     # upscale, 7 taps
    ((513, 257), (224, 224)),    # odd sizes, different scales per axis
    ((3, 2000), (224, 224)),     # 55 taps on 3 rows
    ((33, 1000), (16, 20)),      # 377 taps
]


def content(h: int, w: int, channels: int, seed: int = 0) -> np.ndarray:
    """Random bytes with every 7th column 255 and every (7j + 3)th column 0: both ends of the
    clamp are reached.  HWC for 3 channels, HW for 1."""
    rng = np.random.default_rng([seed, h, w, channels])
    a = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    a[:, 0::7] = 255
    a[:, 3::7] = 0
    return a if channels == 3 else a[:, :, 0]


def _lanczos(x: float) -> float:
    def sinc(t):
        if t == 0.0:
            return 1.0
        t = t * math.pi
        return math.sin(t) / t
    if -3.0 <= x < 3.0:
        return sinc(x) * sinc(x / 3)
    return 0.0


def coefficients(n_in: int, n_out: int):
    """(xmin[out], n[out], k[out][ksize] int32, ksize)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmins = np.zeros(n_out, np.int64)
    ns = np.zeros(n_out, np.int64)
    k = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [_lanczos((j + xmin - center + 0.5) / fs) for j in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for j in range(n):
            v = w[j] / ww if ww != 0.0 else w[j]
            k[xx, j] = int(v * (1 << 22) - 0.5) if v < 0 else int(v * (1 << 22) + 0.5)
        xmins[xx], ns[xx] = xmin, n
    return xmins, ns, k, ksize


def _pass(a: np.ndarray, n_out: int) -> np.ndarray:
    """Resample axis 1 of a (lines, in, C) uint8 array."""
    lines, n_in, ch = a.shape
    xmins, ns, k, _ = coefficients(n_in, n_out)
    out = np.empty((lines, n_out, ch), np.uint8)
    src = a.astype(np.int64)
    for xx in range(n_out):
        x0, n = int(xmins[xx]), int(ns[xx])
        acc = (1 << 21) + np.tensordot(src[:, x0:x0 + n, :], k[xx, :n].astype(np.int64), axes=([1], [0]))
        assert np.all(np.abs(acc) < 2 ** 31)          # the int32 accumulator never wraps
        out[:, xx, :] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def resize_reference(image: np.ndarray, size) -> np.ndarray:
    """image: HxWxC or HxW uint8; size = (width, height) as in Pillow."""
    a = np.asarray(image)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    out_w, out_h = size
    b = a.reshape(a.shape[0], a.shape[1], -1)
    if b.shape[1] != out_w:
        b = _pass(b, out_w)
    if b.shape[0] != out_h:
        b = _pass(b.transpose(1, 0, 2), out_h).transpose(1, 0, 2)
    b = np.ascontiguousarray(b)
    return b if a.ndim == 3 else b[:, :, 0]


def pil_resize(image: np.ndarray, size) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(image).resize(size, Image.Resampling.LANCZOS))


MODES = {"RGB": 3, "L": 1}
_expected = {}


def expected(case, mode):
    """(input, Pillow's result) of a case of CASES in a mode of MODES, computed once and read-only."""
    key = (case, mode)
    if key not in _expected:
        (h, w), size = case
        img = content(h, w, MODES[mode])
        out = pil_resize(img, size)
        img.setflags(write=False)
        out.setflags(write=False)
        _expected[key] = (img, out)
    return _expected[key]


def case_id(case) -> str:
    return f"{case[0][0]}x{case[0][1]}-to-{case[1][0]}x{case[1][1]}"
