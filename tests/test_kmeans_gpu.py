"""HIP tests of k-means (include/imgrec_kmeans.h, csrc/knn_kmeans.hip, faiss_compat.Kmeans) against
the rules of tests/kmeans_check.py.

Step cases (kmeans_check.CASES; data is tests.datagen.mixture(n, d, centres=20, seed=7), sigma 0.5):
the reference's codebook shape scaled down, the concat width with k = 37 and empty clusters, the
DreamSim width with two centroid tiles, k = 1000 >> tile, long segments cut into parts of 64 members
with n no multiple of the 64-point tile, and an odd d.  Every case runs twice and its five outputs
must be byte-equal.  The float64 oracle's share of near-tie points (checked against a margin only) is
printed per case and capped at 1 % by the checker.

Train tests pin the host loop: to the blobs' labels and means, to the step (byte for byte), to the
split rule, to nredo and to the index the class leaves behind.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import kmeans_check as kc
from tests.datagen import mixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def faiss(gpu):
    from image_recommender_amd import faiss_compat
    return faiss_compat


def gpu_step(x, c, flags=0, part=0):
    """kmeans_step_device on numpy inputs: (assign, dist, new_centroids, counts, obj) as numpy.
    The outputs start poisoned, so an element the step leaves unwritten fails the checks."""
    import torch
    from image_recommender_amd import _lib
    lib = _lib.load()
    n, d = x.shape
    k = c.shape[0]
    dev = torch.device("cuda")
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(dev)       # a writable copy
    cd = torch.from_numpy(np.array(c, dtype=np.float32)).to(dev)
    assign = torch.full((n,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    new = torch.full((k, d), float("nan"), dtype=torch.float32, device=dev)
    counts = torch.full((k,), -7, dtype=torch.int64, device=dev)
    obj = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    old = os.environ.get("IMGREC_KMEANS_PART")
    if part:
        os.environ["IMGREC_KMEANS_PART"] = str(part)         # read when the call starts
    try:
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.kmeans_step_device(C.c_void_p(xd.data_ptr()), n, d, C.c_void_p(cd.data_ptr()), k, flags,
                                          C.c_void_p(assign.data_ptr()), C.c_void_p(dist.data_ptr()),
                                          C.c_void_p(new.data_ptr()), C.c_void_p(counts.data_ptr()),
                                          C.c_void_p(obj.data_ptr()), C.c_void_p(st or None)),
                   "kmeans_step_device")
        torch.cuda.synchronize()
    finally:
        if part:
            if old is None:
                os.environ.pop("IMGREC_KMEANS_PART", None)
            else:
                os.environ["IMGREC_KMEANS_PART"] = old
    return (assign.cpu().numpy(), dist.cpu().numpy(), new.cpu().numpy(), counts.cpu().numpy(),
            float(obj.cpu().numpy()[0]))


def same_bytes(a, b):
    for u, v in zip(a[:4], b[:4]):
        assert u.tobytes() == v.tobytes()
    assert np.float64(a[4]).tobytes() == np.float64(b[4]).tobytes()


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_step_case(gpu, name):
    cs = kc.CASE[name]
    x, c = kc.case_data(name)
    out = gpu_step(x, c, part=cs.part)
    share = kc.check_step(x, c, out)
    print(f"{name}: {share:.3%} of the points within the fp32 margin, {int((out[3] == 0).sum())} empty clusters, "
          f"largest cluster {int(out[3].max())}")
    same_bytes(out, gpu_step(x, c, part=cs.part))
    if cs.part:
        assert out[3].max() > 4 * cs.part             # several parts per segment
        # another part size is another summation tree: it must still meet the same bounds
        kc.check_step(x, c, gpu_step(x, c))


def test_duplicate_centroid_row_loses_every_tie(gpu):
    x, c = kc.case_data("sift128")
    c = c.copy()
    c[9] = c[5]
    out = gpu_step(x, c)
    assert (out[0] == 5).any() and not (out[0] == 9).any()
    assert out[3][9] == 0 and out[2][9].tobytes() == c[9].tobytes()
    kc.check_step(x, c, out)
    # the same rows far apart: different centroid tiles, waves and registers
    x2, c2 = kc.case_data("dreamsim768")
    c2 = c2.copy()
    c2[290] = c2[3]
    out2 = gpu_step(x2, c2)
    assert (out2[0] == 3).any() and not (out2[0] == 290).any()
    kc.check_step(x2, c2, out2)


def test_spherical_step(gpu):
    from image_recommender_amd import _lib
    x, c = kc.case_data("sift128")
    xs = np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))
    cs = np.ascontiguousarray(c / np.linalg.norm(c, axis=1, keepdims=True))
    out = gpu_step(xs, cs, flags=_lib.KMEANS_SPHERICAL)
    share = kc.check_step(xs, cs, out, spherical=True)
    print(f"spherical sift128: {share:.3%} within the margin")
    same_bytes(out, gpu_step(xs, cs, flags=_lib.KMEANS_SPHERICAL))


# ---- train -----------------------------------------------------------------------------------------
def test_train_blobs(gpu, faiss):
    rng = np.random.default_rng(3)
    n, d, k = 4000, 64, 16
    centres = 10.0 * rng.standard_normal((k, d))
    labels = np.arange(n) % k
    x = (centres[labels] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    km = faiss.Kmeans(d, k, niter=5)
    last = km.train(x, init_centroids=x[:k])          # row j belongs to blob j
    assert km.centroids.shape == (k, d) and km.centroids.dtype == np.float32
    assert len(km.obj) == 5 and last == km.obj[-1]
    assert (np.diff(km.obj) <= 0).all(), km.obj
    assert [s["nsplit"] for s in km.iteration_stats] == [0] * 5
    assert all(abs(s["imbalance_factor"] - 1.0) < 1e-12 for s in km.iteration_stats[1:])
    D, I = km.assign(x)
    np.testing.assert_array_equal(I, labels)
    kc.check_centroids(x, km.centroids, labels, km.centroids)
    assert isinstance(km.index, faiss.IndexFlatL2) and km.index.ntotal == k


def test_train_equals_three_steps(gpu, faiss):
    x, c0 = kc.case_data("sift128")
    km = faiss.Kmeans(128, 256, niter=3)
    km.train(x, init_centroids=c0)
    assert [s["nsplit"] for s in km.iteration_stats] == [0] * 3
    c, objs = c0, []
    for _ in range(3):
        out = gpu_step(x, c)
        assert out[3].min() > 0
        c = out[2]
        objs.append(out[4])
    assert km.centroids.tobytes() == c.tobytes()
    assert km.obj.tobytes() == np.array(objs, np.float64).tobytes()
    km2 = faiss.Kmeans(128, 256, niter=3)
    km2.train(x, init_centroids=c0)
    assert km2.centroids.tobytes() == km.centroids.tobytes()


def test_train_splits_empty_clusters(gpu, faiss):
    x, c0 = kc.case_data("sift128")
    c0 = c0.copy()
    c0[9] = c0[5]
    km = faiss.Kmeans(128, 256, niter=1)
    km.train(x, init_centroids=c0)
    assert km.iteration_stats[0]["nsplit"] >= 1
    out = gpu_step(x, c0)                               # the state the split started from
    assert out[3][9] == 0
    pairs = kc.check_split(out[2], out[3], km.centroids)
    assert len(pairs) == km.iteration_stats[0]["nsplit"] and pairs[0][0] == 9
    km4 = faiss.Kmeans(128, 256, niter=4)
    km4.train(x, init_centroids=c0)
    assert gpu_step(x, km4.centroids)[3].min() > 0, "a cluster is still empty after four iterations"


def test_split_device_alone(gpu):
    import torch
    from image_recommender_amd import _lib
    rng = np.random.default_rng(8)
    k, d = 12, 19
    old = rng.standard_normal((k, d)).astype(np.float32)
    cnt = np.array([5, 0, 1, 9, 0, 2, 1, 0, 30, 1, 1, 4], np.int64)
    cd = torch.from_numpy(old).cuda()
    host = cnt.copy()
    ns = C.c_int(-1)
    _lib.check(_lib.load().kmeans_split_device(C.c_void_p(cd.data_ptr()), k, d, host.ctypes.data, C.byref(ns),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream or None)),
               "kmeans_split_device")
    torch.cuda.synchronize()
    assert ns.value == 3 and host.sum() == cnt.sum() and (host > 0).all()
    kc.check_split(old, cnt, cd.cpu().numpy())


def test_nredo_keeps_the_best_run(gpu, faiss):
    x, _ = kc.case_data("sift128")
    one = faiss.Kmeans(128, 32, niter=4, nredo=1, seed=99)
    two = faiss.Kmeans(128, 32, niter=4, nredo=2, seed=99)
    o1, o2 = one.train(x), two.train(x)
    assert o2 <= o1 and len(two.obj) == 4 and two.obj[-1] == o2


def test_assign_is_the_index_search(gpu, faiss):
    x, c0 = kc.case_data("odd19")
    km = faiss.Kmeans(19, 33, niter=2)
    with pytest.warns(UserWarning, match="please provide at least 1287 training points"):
        km.train(x, init_centroids=c0)                  # 1000 rows < 33 * 39
    D, I = km.assign(x[:200])
    D2, I2 = km.index.search(x[:200], 1)
    assert D.shape == (200,) and I.shape == (200,)
    np.testing.assert_array_equal(I, I2.ravel())
    np.testing.assert_array_equal(D, D2.ravel())
    best, exc, _, _ = kc.margins(x[:200], km.centroids)     # and it is the nearest centroid
    np.testing.assert_array_equal(I[~exc], best[~exc])


def test_spherical_train(gpu, faiss):
    x, _ = kc.case_data("sift128")
    xs = np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))
    km = faiss.Kmeans(128, 20, niter=4, spherical=True)
    km.train(xs)
    np.testing.assert_allclose(np.linalg.norm(km.centroids, axis=1), 1.0, atol=1e-6)
    # the summed inner product grows, up to the fp32 rounding of the n unit-norm products it sums
    # ((d + 2) * 2^-24 each, kmeans_check's bound at |x| = |c| = 1 over 4)
    assert (np.diff(km.obj) >= -(128 + 2) * xs.shape[0] * 2.0 ** -24).all(), km.obj
    assert isinstance(km.index, faiss.IndexFlatIP)


def test_train_device_matches_train(gpu, faiss):
    import torch
    x, c0 = kc.case_data("parts")
    a = faiss.Kmeans(16, 7, niter=3, max_points_per_centroid=1000)     # train() must not subsample
    a.train(x, init_centroids=c0)
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    b = faiss.Kmeans(16, 7, niter=3)
    b.train_device(xd.data_ptr(), x.shape[0], torch.cuda.current_stream().cuda_stream, init_centroids=c0)
    assert a.centroids.tobytes() == b.centroids.tobytes() and a.obj.tobytes() == b.obj.tobytes()


def test_the_reference_call(gpu, faiss):
    x = mixture(10000, 128, centres=20, seed=7)
    kmeans = faiss.Kmeans(x.shape[1], 256, niter=25, verbose=True, gpu=True)
    kmeans.train(x)
    assert kmeans.centroids.shape == (256, 128) and np.isfinite(kmeans.centroids).all()
    assert len(kmeans.obj) == 25 and kmeans.obj[-1] <= kmeans.obj[0]
