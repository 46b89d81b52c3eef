"""GPU tests of the LANCZOS resize kernels (csrc/resize.hip): every case of tests/resize_check.py
equals Pillow bit for bit in both output formats and both modes; a ragged batch at odd offsets
equals its images alone, in any order; two calls on two streams; a caller's `out` is all that is
written; the DreamSim indexer's device_resize path feeds the model the tensor of its default path.
"""
from pathlib import Path

import numpy as np
import pytest

from tests.resize_check import CASES, MODES, case_id, content, expected

pytestmark = pytest.mark.gpu


def _f32_chw(u8: np.ndarray) -> np.ndarray:
    """What load_image(normalize=True) and the indexer's transpose(2, 0, 1) make of an image."""
    a = u8.astype(np.float32) / 255.0
    return np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1).transpose(2, 0, 1))


def _pack_odd(images, lead=1):
    """The images in one buffer at offsets that are no multiple of 4."""
    offsets, pos = [], lead
    for im in images:
        while pos % 4 == 0:
            pos += 1
        offsets.append(pos)
        pos += im.size + 2
    buf = np.zeros(pos + 3, np.uint8)
    for im, o in zip(images, offsets):
        buf[o:o + im.size] = im.reshape(-1)
    return buf, offsets, [im.shape[:2] for im in images]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_each_case_equals_pillow(gpu, case, mode):
    from image_recommender_amd.resize import lanczos_resize
    img, want = expected(case, mode)
    size = case[1]
    got = lanczos_resize([img], size, "u8")
    assert got.shape == (1,) + want.shape and got.dtype == np.uint8
    assert np.array_equal(got[0], want), int((got[0] != want).sum())
    f = lanczos_resize([img], size, "f32")
    wf = _f32_chw(want)
    assert f.shape == (1,) + wf.shape and f.dtype == np.float32
    assert np.array_equal(f[0].view(np.uint32), wf.view(np.uint32))


@pytest.mark.parametrize("shape,size", [
    ((7, 5000), (50, 5)),        # 8 rows exceed the LDS budget: blocks of 3 rows, the last of 1
    ((9, 16500), (64, 3)),       # one row exceeds it: rows read from global memory, 8 + 1 rows
    ((2, 16500), (64, 2)),       # the same with the vertical pass skipped and a partial block only
    ((2, 50000), (70, 2)),       # ... long enough for mode L to take that path too
], ids=["rows-of-3", "global-rows", "global-rows-h-only", "global-rows-L"])
def test_rows_wider_than_the_lds_budget(gpu, shape, size):
    """The horizontal kernel's paths for long rows (csrc/resize.hip: kHLds), both modes, in one
    ragged call with a small image so the block search sees both kinds."""
    import torch
    from image_recommender_amd.resize import lanczos_resize_device
    from tests.resize_check import pil_resize
    for mode, ch in MODES.items():
        wide, small = content(*shape, ch), content(6, 9, ch)
        buf, offsets, shapes = _pack_odd([small, wide, small])
        got = lanczos_resize_device(torch.from_numpy(buf).cuda(), offsets, shapes, size, "u8", channels=ch)
        got = got.cpu().numpy()
        for slot, img in enumerate((small, wide, small)):
            want = pil_resize(img, size).reshape(size[1], size[0], ch)
            assert np.array_equal(got[slot], want), (mode, slot, int((got[slot] != want).sum()))


def test_ragged_batch_at_odd_offsets_any_order(gpu):
    import torch
    from image_recommender_amd.resize import lanczos_resize_device
    size = (224, 224)
    cases = [c for c in CASES if c[1] == size]
    assert len(cases) >= 5
    pairs = [expected(c, "RGB") for c in cases]
    images = [p[0] for p in pairs]
    for order in (list(range(len(images))), list(reversed(range(len(images))))):
        buf, offsets, shapes = _pack_odd([images[i] for i in order])
        assert all(o % 4 for o in offsets)
        pixels = torch.from_numpy(buf).cuda()
        got = lanczos_resize_device(pixels, offsets, shapes, size, "u8").cpu().numpy()
        gf = lanczos_resize_device(pixels, offsets, shapes, size, "f32").cpu().numpy()
        for slot, i in enumerate(order):
            want = pairs[i][1]          # Pillow = the image's result alone (test_each_case_equals_pillow)
            assert np.array_equal(got[slot], want), (order, i, int((got[slot] != want).sum()))
            assert np.array_equal(gf[slot].view(np.uint32), _f32_chw(want).view(np.uint32)), (order, i)


def test_unaligned_tensor_base_and_gray_batch(gpu):
    """A pixel tensor that itself starts at an odd address (a view), mode L, several images."""
    import torch
    from image_recommender_amd.resize import lanczos_resize_device
    cases = [CASES[0], CASES[6], CASES[8]]
    for c in cases:
        img, want = expected(c, "L")
        buf, offsets, shapes = _pack_odd([img, img], lead=3)
        whole = torch.from_numpy(np.concatenate([np.zeros(5, np.uint8), buf])).cuda()
        got = lanczos_resize_device(whole[5:], offsets, shapes, c[1], "u8", channels=1).cpu().numpy()
        assert got.shape == (2,) + want.shape + (1,)
        assert np.array_equal(got[0, ..., 0], want) and np.array_equal(got[1, ..., 0], want)


def test_two_streams_back_to_back(gpu):
    import torch
    from image_recommender_amd.resize import lanczos_resize_device, pack_images
    a_case, b_case = CASES[6], CASES[7]          # different shapes: the second call rebuilds the tables
    (a_img, a_want), (b_img, b_want) = expected(a_case, "RGB"), expected(b_case, "RGB")
    abuf, aoff, ashape, _ = pack_images([a_img] * 3)
    bbuf, boff, bshape, _ = pack_images([b_img] * 2)
    ap, bp = torch.from_numpy(abuf).cuda(), torch.from_numpy(bbuf).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ra = lanczos_resize_device(ap, aoff, ashape, a_case[1], "u8", stream=s1)
    rb = lanczos_resize_device(bp, boff, bshape, b_case[1], "f32", stream=s2)
    torch.cuda.synchronize()
    ra, rb = ra.cpu().numpy(), rb.cpu().numpy()
    for k in range(3):
        assert np.array_equal(ra[k], a_want)
    for k in range(2):
        assert np.array_equal(rb[k].view(np.uint32), _f32_chw(b_want).view(np.uint32))


@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_out_margins_stay_untouched(gpu, fmt):
    import torch
    from image_recommender_amd.resize import lanczos_resize_device, pack_images
    case = CASES[0]                              # 4 x 3 x 3 = 36 result bytes per image: odd-sized rows
    img, want = expected(case, "RGB")
    other, owant = expected(CASES[5], "RGB")
    for cs, imgs, wants in ((case, [img, img], [want, want]), (CASES[5], [other], [owant])):
        buf, offs, shapes, _ = pack_images(imgs)
        pixels = torch.from_numpy(buf).cuda()
        ow, oh = cs[1]
        n = len(imgs)
        if fmt == "u8":
            shape, dtype, fill, margin = (n, oh, ow, 3), torch.uint8, 0xA5, 64
        else:
            shape, dtype, fill, margin = (n, 3, oh, ow), torch.float32, -7.5, 16
        count = int(np.prod(shape))
        big = torch.full((count + 2 * margin,), fill, dtype=dtype, device="cuda")
        out = big[margin:margin + count].view(shape)
        ret = lanczos_resize_device(pixels, offs, shapes, cs[1], fmt, out=out)
        torch.cuda.synchronize()
        assert ret.data_ptr() == out.data_ptr()
        host = big.cpu().numpy()
        assert (host[:margin] == fill).all() and (host[margin + count:] == fill).all()
        body = host[margin:margin + count].reshape(shape)
        for k, w in enumerate(wants):
            if fmt == "u8":
                assert np.array_equal(body[k], w)
            else:
                assert np.array_equal(body[k].view(np.uint32), _f32_chw(w).view(np.uint32))


def test_empty_batch(gpu):
    import torch
    from image_recommender_amd.resize import lanczos_resize_device
    out = lanczos_resize_device(torch.zeros(1, dtype=torch.uint8, device="cuda"), [], [], (8, 4), "f32")
    assert tuple(out.shape) == (0, 3, 4, 8)


def test_indexer_device_resize_feeds_the_same_tensor(gpu, tmp_path):
    import torch
    from PIL import Image
    from image_recommender_amd.vector_scripts.create_dreamsim_vector import DreamSimVectorIndexer

    names = []
    for k, (w, h) in enumerate([(40, 30), (224, 224), (300, 260)]):
        Image.fromarray(content(h, w, 3, seed=k)).save(tmp_path / f"im{k}.png")
        names.append(f"im{k}.png")
    (tmp_path / "bad.png").write_bytes(b"not an image at all" * 7)
    names.insert(2, "bad.png")

    class Probe(DreamSimVectorIndexer):                  # no DB, no logs, no model: the input is the output
        def __init__(self, device_resize):
            self.device = torch.device("cuda")
            self.base_dir = Path(tmp_path)
            self.dim = 3 * 224 * 224
            self.device_resize = device_resize
            self.warnings = []

        def _log_and_print(self, message, level="info"):
            self.warnings.append((level, message))

        def embed_tensor(self, images):
            assert images.is_cuda and images.dtype == torch.float32 and tuple(images.shape[1:]) == (3, 224, 224)
            return images.reshape(images.shape[0], -1)

    host, dev = Probe(False), Probe(True)
    eh, vh = host._batch_image_to_vector(names)
    ed, vd = dev._batch_image_to_vector(names)
    assert vh == vd == [n for n in names if n != "bad.png"]
    assert host.warnings == dev.warnings and len(dev.warnings) == 1 and dev.warnings[0][0] == "warning"
    assert eh.shape == ed.shape == (3, 3 * 224 * 224)
    assert np.array_equal(eh.numpy().view(np.uint32), ed.numpy().view(np.uint32))
    # nothing readable: the same empty answer
    e0, v0 = dev._batch_image_to_vector(["bad.png"])
    assert v0 == [] and tuple(e0.shape) == (0, dev.dim)
