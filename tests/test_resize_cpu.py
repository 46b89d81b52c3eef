"""CPU tests of the LANCZOS resize: the numpy checker (tests/resize_check.py) and the library's
host statement (resize_lanczos_host) each equal Pillow byte for byte; argument validation.  No GPU.
"""
import ctypes as C

import numpy as np
import pytest

from image_recommender_amd import _lib
from image_recommender_amd.resize import lanczos_resize_host, pack_images
from tests.resize_check import CASES, MODES, case_id, content, expected, pil_resize, resize_reference


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_checker_and_host_equal_pillow(case, mode):
    img, want = expected(case, mode)
    size = case[1]
    assert want.shape[:2] == (size[1], size[0])
    ref = resize_reference(img, size)
    assert ref.shape == want.shape and np.array_equal(ref, want), int((ref != want).sum())
    got = lanczos_resize_host(img, size)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), int((got != want).sum())


def test_content_reaches_both_ends_of_the_clamp():
    """A downscaling case (scale >= 1 on both axes) whose expected image holds 0 and 255."""
    hit = []
    for case in CASES:
        (h, w), (ow, oh) = case
        if h >= oh and w >= ow:
            for mode in MODES:
                _, want = expected(case, mode)
                hit.append(bool((want == 0).any() and (want == 255).any()))
    assert hit and any(hit)


def test_host_takes_strided_views_and_single_channel_hwc():
    img = content(40, 30, 3)
    a = lanczos_resize_host(img[::2, ::3], (7, 9))
    assert np.array_equal(a, pil_resize(np.ascontiguousarray(img[::2, ::3]), (7, 9)))
    g = content(12, 17, 1)
    b = lanczos_resize_host(g[:, :, None], (5, 6))
    assert b.shape == (6, 5, 1) and np.array_equal(b[:, :, 0], pil_resize(g, (5, 6)))


def test_argument_validation():
    lib = _lib.load()
    px = np.zeros((4, 4, 3), np.uint8)
    out = np.zeros((8, 8, 3), np.uint8)
    p, o = px.ctypes.data, out.ctypes.data

    def host(*a):
        rc = lib.resize_lanczos_host(*a)
        return rc, lib.resize_last_error().decode()

    rc, msg = host(p, 4, 4, 2, 8, 8, o)
    assert rc == _lib.KNN_EINVAL and "channels" in msg
    rc, msg = host(p, 4, 4, 3, 0, 8, o)
    assert rc == _lib.KNN_EINVAL and "positive" in msg
    rc, msg = host(p, 4, 4, 3, 8, -1, o)
    assert rc == _lib.KNN_EINVAL and "positive" in msg
    rc, msg = host(p, 0, 4, 3, 8, 8, o)
    assert rc == _lib.KNN_EINVAL and "positive" in msg
    rc, msg = host(None, 4, 4, 3, 8, 8, o)
    assert rc == _lib.KNN_EINVAL and "NULL" in msg
    rc, msg = host(p, 4, 4, 3, 8, 8, None)
    assert rc == _lib.KNN_EINVAL and "NULL" in msg

    # the device entry validates before it touches a device
    offs = np.zeros(1, np.int64)
    hs = np.full(1, 4, np.int32)
    ws = np.full(1, 4, np.int32)

    def dev(pix, n, ch, oh, ow, fmt, dst, heights=hs):
        rc = lib.resize_lanczos_device(pix, offs.ctypes.data, heights.ctypes.data, ws.ctypes.data, n, ch, oh, ow,
                                       fmt, dst, None)
        return rc, lib.resize_last_error().decode()

    fake = C.c_void_p(4096)        # never dereferenced: every call below fails or does nothing
    rc, msg = dev(fake, 1, 4, 8, 8, _lib.RESIZE_U8_HWC, fake)
    assert rc == _lib.KNN_EINVAL and "channels" in msg
    rc, msg = dev(fake, 1, 3, 8, 0, _lib.RESIZE_U8_HWC, fake)
    assert rc == _lib.KNN_EINVAL and "positive" in msg
    rc, msg = dev(None, 1, 3, 8, 8, _lib.RESIZE_U8_HWC, fake)
    assert rc == _lib.KNN_EINVAL and "NULL" in msg
    rc, msg = dev(fake, 1, 3, 8, 8, _lib.RESIZE_F32_CHW, None)
    assert rc == _lib.KNN_EINVAL and "NULL" in msg
    rc, msg = dev(fake, -1, 3, 8, 8, _lib.RESIZE_U8_HWC, fake)
    assert rc == _lib.KNN_EINVAL and "negative" in msg
    rc, msg = dev(fake, 1, 3, 8, 8, 7, fake)
    assert rc == _lib.KNN_EINVAL and "format" in msg
    # n == 0 is a successful no-op, null pointers included
    assert lib.resize_lanczos_device(None, None, None, None, 0, 3, 8, 8, _lib.RESIZE_U8_HWC, None, None) == 0


def test_wrapper_rejects_bad_input():
    with pytest.raises(ValueError):
        lanczos_resize_host(np.zeros((4, 4, 2), np.uint8), (2, 2))
    with pytest.raises(ValueError):
        lanczos_resize_host(np.zeros((4, 4, 3), np.float32), (2, 2))
    with pytest.raises(ValueError):
        lanczos_resize_host(np.zeros((4, 4, 3), np.uint8), (0, 2))
    with pytest.raises(ValueError):
        pack_images([np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)])


def test_pack_images_layout():
    imgs = [content(3, 5, 3), content(7, 2, 3), content(1, 1, 3)]
    buf, offs, shapes, ch = pack_images(imgs)
    assert ch == 3 and shapes.tolist() == [[3, 5], [7, 2], [1, 1]]
    assert all(o % 48 == 0 for o in offs) and list(offs) == sorted(offs)
    for im, o in zip(imgs, offs):
        assert np.array_equal(buf[o:o + im.size], im.reshape(-1))
