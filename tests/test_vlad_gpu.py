"""HIP tests of the soft-VLAD encoding (include/imgrec_vlad.h, csrc/vlad.hip,
image_recommender_amd.vlad) against the rules of tests/vlad_check.py.

Every case (vlad_check.CASES: the reference's shape at sigma = 125 and at 0.5, more than one
codebook tile, an odd d, k barely above nn, k = nn, nn = 1, nn = 8, two bitwise-equal codebook rows;
images of 0, 1, 3, 64, 65, 300, 0 and 1000 descriptors) goes through vlad_encode_device with
poisoned outputs, twice, and the two runs must be byte-equal.  The float64 oracle's share of
near-tie descriptors (checked against a margin only) is printed per case and capped at 1 % by the
checker.  Then: batch invariance byte for byte, the optional outputs, the four ways to call, a
cluster-tiled aggregation, from_kmeans, nn = 1 byte for byte against the k-means step, and agreement
with IndexFlatL2.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import vlad_check as vc

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in vc.CASES]


def gpu_encode(x, off, c, nn, sigma, raw=False, lists=True, lds_floats=0):
    """vlad_encode_device on numpy inputs: (vlad, nn_idx, nn_dist) as numpy (the lists None without
    `lists`).  The outputs start poisoned, so an element the call leaves unwritten fails the checks."""
    import torch
    from image_recommender_amd import _lib
    lib = _lib.load()
    n, d = x.shape
    k, nimg = c.shape[0], len(off) - 1
    dev = torch.device("cuda")
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(dev)       # writable copies
    cd = torch.from_numpy(np.array(c, dtype=np.float32)).to(dev)
    od = torch.from_numpy(np.array(off, dtype=np.int64)).to(dev)
    out = torch.full((nimg, k * d), float("nan"), dtype=torch.float32, device=dev)
    idx = torch.full((max(n, 1), nn), -7, dtype=torch.int32, device=dev)
    dist = torch.full((max(n, 1), nn), float("nan"), dtype=torch.float32, device=dev)
    old = os.environ.get("IMGREC_VLAD_LDS_FLOATS")
    if lds_floats:
        os.environ["IMGREC_VLAD_LDS_FLOATS"] = str(lds_floats)        # read when the call starts
    try:
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.vlad_encode_device(
            C.c_void_p(xd.data_ptr()), n, C.c_void_p(od.data_ptr()), nimg, d, C.c_void_p(cd.data_ptr()), k, nn,
            float(sigma), _lib.VLAD_RAW if raw else 0, C.c_void_p(out.data_ptr()),
            C.c_void_p(idx.data_ptr()) if lists else None, C.c_void_p(dist.data_ptr()) if lists else None,
            C.c_void_p(st or None)), "vlad_encode_device")
        torch.cuda.synchronize()
    finally:
        if lds_floats:
            if old is None:
                os.environ.pop("IMGREC_VLAD_LDS_FLOATS", None)
            else:
                os.environ["IMGREC_VLAD_LDS_FLOATS"] = old
    if not lists:
        assert (idx == -7).all() and torch.isnan(dist).all()
        return out.cpu().numpy(), None, None
    return out.cpu().numpy(), idx.cpu().numpy()[:n], dist.cpu().numpy()[:n]


@pytest.fixture(scope="module")
def runs(gpu):
    """(vlad, raw, nn_idx, nn_dist) of every case, computed once on first use."""
    cache = {}

    def get(name):
        if name not in cache:
            cs = vc.CASE[name]
            x, off, c = vc.case_data(name)
            vlad, idx, dist = gpu_encode(x, off, c, cs.nn, cs.sigma)
            raw, idx2, dist2 = gpu_encode(x, off, c, cs.nn, cs.sigma, raw=True)
            assert idx.tobytes() == idx2.tobytes() and dist.tobytes() == dist2.tobytes()
            cache[name] = (vlad, raw, idx, dist)
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_case(gpu, runs, name):
    cs = vc.CASE[name]
    x, off, c = vc.case_data(name)
    out = runs(name)
    share, _ = vc.check_all(x, off, c, cs.nn, cs.sigma, out)
    print(f"{name}: {share:.3%} of the descriptors within the fp32 margin")
    again = gpu_encode(x, off, c, cs.nn, cs.sigma)
    raw_again = gpu_encode(x, off, c, cs.nn, cs.sigma, raw=True)[0]
    for u, v in zip((out[0], out[2], out[3], out[1]), (*again, raw_again)):
        assert u.tobytes() == v.tobytes()


def test_duplicate_rows_list_the_smaller_id_first(gpu, runs):
    idx = runs("dup")[2]
    has5, has9 = (idx == 5).any(1), (idx == 9).any(1)
    assert has5.any() and has9.any()
    assert not (has9 & ~has5).any(), "row 9 listed without its equal row 5"
    p5, p9 = (idx == 5).argmax(1), (idx == 9).argmax(1)
    assert (p5[has9] < p9[has9]).all()
    # 5 without 9 only where 5 took the last slot (bitwise-equal keys are neighbours in the order,
    # unless rows 6..8 tie with them exactly, which this data does not do)
    assert (p5[has5 & ~has9] == 3).all()


def test_batch_invariance(gpu, runs):
    cs = vc.CASE["sift"]
    x, off, c = vc.case_data("sift")
    vlad, raw, idx, dist = runs("sift")
    nimg = len(off) - 1
    for i in range(nimg):
        xi = x[off[i]:off[i + 1]]
        oi = np.array([0, xi.shape[0]], np.int64)
        v1, i1, d1 = gpu_encode(xi, oi, c, cs.nn, cs.sigma)
        assert v1[0].tobytes() == vlad[i].tobytes(), f"image {i} alone differs from its row of the batch"
        assert i1.tobytes() == idx[off[i]:off[i + 1]].tobytes() and d1.tobytes() == dist[off[i]:off[i + 1]].tobytes()
        assert gpu_encode(xi, oi, c, cs.nn, cs.sigma, raw=True)[0][0].tobytes() == raw[i].tobytes()
    parts = [x[off[i]:off[i + 1]] for i in range(nimg)][::-1]
    xr = np.ascontiguousarray(np.concatenate(parts))
    offr = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
    vr = gpu_encode(xr, offr, c, cs.nn, cs.sigma)[0]
    assert vr[::-1].tobytes() == vlad.tobytes()


def test_lists_are_optional(gpu, runs):
    cs = vc.CASE["sift_sharp"]
    x, off, c = vc.case_data("sift_sharp")
    vlad, raw, _, _ = runs("sift_sharp")
    assert gpu_encode(x, off, c, cs.nn, cs.sigma, lists=False)[0].tobytes() == vlad.tobytes()
    assert gpu_encode(x, off, c, cs.nn, cs.sigma, raw=True, lists=False)[0].tobytes() == raw.tobytes()


@pytest.mark.parametrize("name,floats", [("sift", 5000), ("k300", 49), ("odd19", 1)])
def test_cluster_tiles_change_nothing(gpu, runs, name, floats):
    """A smaller accumulator splits the codebook over several workgroups per image (39 rows of 256 per
    tile; one row per tile): the bytes do not change."""
    cs = vc.CASE[name]
    x, off, c = vc.case_data(name)
    vlad, raw, idx, dist = runs(name)
    v, i, d = gpu_encode(x, off, c, cs.nn, cs.sigma, lds_floats=floats)
    assert v.tobytes() == vlad.tobytes() and i.tobytes() == idx.tobytes() and d.tobytes() == dist.tobytes()
    assert gpu_encode(x, off, c, cs.nn, cs.sigma, raw=True, lds_floats=floats)[0].tobytes() == raw.tobytes()


def test_four_ways_to_call(gpu, runs):
    import torch
    from image_recommender_amd import _lib
    from image_recommender_amd.vlad import SoftVLAD
    cs = vc.CASE["sift"]
    x, off, c = vc.case_data("sift")
    vlad, raw, idx, dist = runs("sift")
    enc = SoftVLAD(c, nn=cs.nn, sigma=cs.sigma)
    a = enc.encode([x[off[i]:off[i + 1]] for i in range(len(off) - 1)])
    assert a.dtype == np.float32 and a.shape == (len(off) - 1, enc.dim) and a.tobytes() == vlad.tobytes()
    b, bi, bd = enc.encode((x, off), return_assignment=True)
    assert b.tobytes() == vlad.tobytes() and bi.tobytes() == idx.tobytes() and bd.tobytes() == dist.tobytes()
    assert enc.encode((x, off), raw=True).tobytes() == raw.tobytes()
    xd = torch.from_numpy(np.array(x)).cuda()
    od = torch.from_numpy(np.array(off)).cuda()
    out = torch.full((len(off) - 1, enc.dim), float("nan"), dtype=torch.float32, device="cuda")
    enc.encode_device(xd.data_ptr(), od.data_ptr(), len(off) - 1, x.shape[0], out.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == vlad.tobytes()
    h = np.full_like(vlad, np.nan)
    hi = np.full_like(idx, -7)
    xc, cc = np.ascontiguousarray(x), np.ascontiguousarray(c)
    _lib.check(_lib.load().vlad_encode(xc.ctypes.data, x.shape[0], off.ctypes.data, len(off) - 1, 128, cc.ctypes.data,
                                       256, cs.nn, cs.sigma, 0, h.ctypes.data, hi.ctypes.data, None, -1), "vlad_encode")
    assert h.tobytes() == vlad.tobytes() and hi.tobytes() == idx.tobytes()
    # no images, and images without any descriptor
    assert enc.encode([]).shape == (0, enc.dim)
    z = enc.encode([np.zeros((0, 128), np.float32), []])
    assert z.shape == (2, enc.dim) and not z.any()


def test_from_kmeans(gpu):
    from image_recommender_amd import faiss_compat as faiss
    from image_recommender_amd.vlad import SoftVLAD
    x, off, _ = vc.case_data("sift")
    km = faiss.Kmeans(128, 32, niter=3)
    km.train(x)
    enc = SoftVLAD.from_kmeans(km)
    assert (enc.k, enc.d, enc.nn, enc.sigma) == (32, 128, 4, 125.0)
    vlad, idx, dist = enc.encode((x, off), return_assignment=True)
    raw = enc.encode((x, off), raw=True)
    vc.check_dist(x, km.centroids, idx, dist)
    vc.check_raw(x, off, km.centroids, 125.0, idx, dist, raw)
    vc.check_final(raw, vlad, off, 32, 128)
    np.testing.assert_allclose(np.linalg.norm(vlad[np.diff(off) > 0], axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("n,d,k,tie", [
    (333, 19, 300, (290, 3)),    # ragged last workgroup, scalar loads, padded depth, two codebook tiles
    (130, 40, 7, None),          # one tile barely used, a two-row tail workgroup, a partial last stage
])
def test_one_neighbour_is_the_kmeans_assignment(gpu, n, d, k, tie):
    """vlad_nn_kernel<1> and kmeans_assign_kernel run one stage stream (csrc/rows_tile.h) with one key,
    one (key, id) order and one direct distance: nn = 1 returns, per descriptor, the bytes of
    kmeans_step_device's assign and dist on the same rows and codebook."""
    from tests.test_kmeans_gpu import gpu_step
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, d)).astype(np.float32)
    c = x[rng.choice(n, k, replace=False)] + 0.1 * rng.standard_normal((k, d)).astype(np.float32)
    if tie:
        c[tie[0]] = c[tie[1]]                        # a tie that crosses the two tiles
    assign, dist = gpu_step(x, c)[:2]
    _, idx, nnd = gpu_encode(x, np.array([0, n], np.int64), c, 1, 125.0, raw=True)
    assert idx.shape == nnd.shape == (n, 1) and idx.dtype == assign.dtype and nnd.dtype == dist.dtype
    assert np.isfinite(dist).all()
    assert idx.tobytes() == assign.tobytes()
    assert nnd.tobytes() == dist.tobytes()
    if tie:
        assert (assign == tie[1]).any() and not (assign == tie[0]).any()


@pytest.mark.parametrize("name", ["sift", "k300", "odd19"])
def test_neighbours_agree_with_the_flat_index(gpu, runs, name):
    from image_recommender_amd import faiss_compat as faiss
    cs = vc.CASE[name]
    x, off, c = vc.case_data(name)
    idx = runs(name)[2]
    _, clear = vc.check_neighbours(x, c, cs.nn, idx)
    index = faiss.IndexFlatL2(cs.d)
    index.add(np.ascontiguousarray(c))
    _, I = index.search(np.ascontiguousarray(x), cs.nn)
    np.testing.assert_array_equal(np.sort(I[clear], axis=1), np.sort(idx[clear].astype(np.int64), axis=1))
    # label for label where the order inside the list is clear too (every float64 gap between
    # adjacent ranks above the fp32 margin): two near-equal distances may be ordered differently by
    # two kernels that are both right
    top, _, _, _, D, E = vc.margins(x, c, cs.nn)
    rows = np.arange(x.shape[0])[:, None]
    Dt, Et = D[rows, top], E[rows, top]
    ordered = clear & (np.diff(Dt, axis=1) > Et[:, :-1] + Et[:, 1:]).all(1)
    assert ordered.mean() > 0.5
    np.testing.assert_array_equal(I[ordered], idx[ordered].astype(np.int64))


def test_encode_device_alternating_on_two_streams(gpu):
    """Six encodings alternating between two streams share the per-device workspace (code norms,
    neighbour lists) through its stream hand-off (csrc/dev_workspace.h over csrc/stream_fence.h): each
    equals, byte for byte, the same encoding called alone on one stream.  Every call has descriptors
    of its own, so a call that overtook its predecessor's use of the workspace would show."""
    import torch
    from image_recommender_amd.vlad import SoftVLAD
    from tests.datagen import mixture
    nimg, per, d, k, nn, calls = 4, 50, 128, 16, 4, 6
    data = mixture(k + calls * nimg * per, d, centres=k, seed=41)
    enc = SoftVLAD(data[:k], nn=nn, sigma=1.0)
    xs = [torch.from_numpy(np.ascontiguousarray(data[k + c * nimg * per:k + (c + 1) * nimg * per])).cuda()
          for c in range(calls)]
    off = torch.arange(0, nimg * per + 1, per, dtype=torch.int64).cuda()
    enc.codebook_device()
    one = torch.cuda.Stream()
    torch.cuda.synchronize()

    def run(streams, sync):
        outs = [torch.full((nimg, enc.dim), float("nan"), dtype=torch.float32, device="cuda") for _ in xs]
        torch.cuda.synchronize()
        for c, (x, out) in enumerate(zip(xs, outs)):
            enc.encode_device(x.data_ptr(), off.data_ptr(), nimg, nimg * per, out.data_ptr(),
                              stream=streams[c % len(streams)].cuda_stream)
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]

    alone = run([one], True)
    assert all(np.isfinite(a).all() for a in alone)
    assert len({a.tobytes() for a in alone}) == calls
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for got, want in zip(run([a, b], False), alone):
        assert got.tobytes() == want.tobytes()
