"""CPU tests of k-means: the checker of tests/kmeans_check.py accepts a correct fp32 step on every
case of the GPU suite and rejects each kind of defect; every case keeps its share of near-tie points
(where only a margin is checked) at or below 1 %; faiss_compat.Kmeans exists and validates its
arguments; the C entry points reject bad arguments before any GPU call.  No GPU is used.
"""
import ctypes as C

import numpy as np
import pytest

from image_recommender_amd import _lib
from tests import kmeans_check as kc

NAMES = [c.name for c in kc.CASES]


@pytest.fixture(scope="module")
def steps():
    """The fp32 numpy step of every case, computed once."""
    return {name: kc.step32(*kc.case_data(name)) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_fp32_step_passes_and_share_is_small(name, steps):
    x, c = kc.case_data(name)
    share = kc.exception_share(x, c)
    print(f"{name}: {share:.3%} of the points within the fp32 margin, "
          f"{int((steps[name][3] == 0).sum())} empty clusters")
    assert share <= kc.MAX_SHARE
    assert kc.check_step(x, c, steps[name]) == share


def test_spherical_fp32_step_passes():
    x, c = kc.case_data("sift128")
    xs = x / np.linalg.norm(x, axis=1, keepdims=True)
    cs = c / np.linalg.norm(c, axis=1, keepdims=True)
    assert kc.check_step(xs, cs, kc.step32(xs, cs, spherical=True), spherical=True) <= kc.MAX_SHARE


def test_cases_cover_what_they_claim(steps):
    assert (steps["concat1968"][3] == 0).any(), "the wide case must have empty clusters"
    assert steps["parts"][3].max() > 4 * kc.CASE["parts"].part, "several parts per segment"
    assert kc.CASE["odd19"].d % 2 == 1 and kc.CASE["parts"].n % 64 != 0
    assert kc.CASE["dreamsim768"].k > 256 and kc.CASE["concat1968"].k % 32 != 0


@pytest.mark.parametrize("name", ["sift128", "parts"])
def test_relabelled_clear_point_is_rejected(name, steps):
    x, c = kc.case_data(name)
    a, dist, new, cnt, obj = steps[name]
    _, exc, _, D = kc.margins(x, c)
    p = int(np.nonzero(~exc)[0][0])
    a2 = a.copy()
    a2[p] = int(np.argsort(D[p])[1])
    with pytest.raises(AssertionError, match="clear points mislabelled"):
        kc.check_assign(x, c, a2)


def test_tie_to_the_larger_id_is_rejected(steps):
    x, c = kc.case_data("sift128")
    c = c.copy()
    c[9] = c[5]
    out = kc.step32(x, c)
    a = out[0].copy()
    assert (a == 5).any() and not (a == 9).any()
    kc.check_assign(x, c, a)
    a[np.nonzero(a == 5)[0][0]] = 9
    with pytest.raises(AssertionError, match="larger id of an exact tie"):
        kc.check_assign(x, c, a)


def test_count_off_by_one_is_rejected(steps):
    a, _, _, cnt, _ = steps["manyk"]
    cnt2 = cnt.copy()
    cnt2[3] += 1
    with pytest.raises(AssertionError):
        kc.check_counts(a, cnt2, kc.CASE["manyk"].k)


@pytest.mark.parametrize("name", ["sift128", "parts"])
def test_centroid_coordinate_off_is_rejected(name, steps):
    x, c = kc.case_data(name)
    a, _, new, cnt, _ = steps[name]
    j = int(np.nonzero(cnt)[0][0])
    new2 = new.copy()
    new2[j, 1] += np.float32(1e-3)
    with pytest.raises(AssertionError, match=f"cluster {j} "):
        kc.check_centroids(x, c, a, new2)
    e = np.nonzero(steps["concat1968"][3] == 0)[0]
    xw, cw = kc.case_data("concat1968")
    neww = steps["concat1968"][2].copy()
    neww[e[0], 0] = np.nextafter(neww[e[0], 0], np.float32(np.inf))
    with pytest.raises(AssertionError, match="not copied through"):
        kc.check_centroids(xw, cw, steps["concat1968"][0], neww)


def test_dist_and_obj_defects_are_rejected(steps):
    x, c = kc.case_data("sift128")
    a, dist, _, _, obj = steps["sift128"]
    d2 = dist.copy()
    d2[7] *= np.float32(1.01)
    with pytest.raises(AssertionError):
        kc.check_dist(x, c, a, d2)
    with pytest.raises(AssertionError):
        kc.check_obj(dist, obj * (1 + 1e-9))


def test_split_rule():
    rng = np.random.default_rng(5)
    old = rng.standard_normal((6, 9)).astype(np.float32)
    cnt = np.array([4, 0, 1, 7, 0, 2])
    new = old.copy()
    new[1], new[3] = kc.split_rows(old[3])
    new[4], new[0] = kc.split_rows(old[0])
    assert kc.check_split(old, cnt, new) == [(1, 3), (4, 0)]
    wrong = new.copy()                       # the sign pattern swapped between the two rows
    wrong[3], wrong[1] = kc.split_rows(old[3])
    with pytest.raises(AssertionError):
        kc.check_split(old, cnt, wrong)
    lone = old.copy()                        # a donor with a single member
    lone[1], lone[2] = kc.split_rows(old[2])
    lone[4], lone[0] = kc.split_rows(old[0])
    with pytest.raises(AssertionError):
        kc.check_split(old, cnt, lone)
    touched = new.copy()
    touched[5, 0] += 1
    with pytest.raises(AssertionError):
        kc.check_split(old, cnt, touched)


# ---- the Python class -------------------------------------------------------------------------------
def test_kmeans_class_validates():
    from image_recommender_amd import faiss_compat as faiss
    assert "Kmeans" in faiss.__all__
    km = faiss.Kmeans(128, 256, niter=25, verbose=True, gpu=True)
    assert (km.d, km.k, km.niter, km.nredo, km.seed) == (128, 256, 25, 1, 1234)
    assert (km.min_points_per_centroid, km.max_points_per_centroid) == (39, 256)
    assert km.centroids is None
    with pytest.raises(NotImplementedError):
        faiss.Kmeans(8, 2, int_centroids=True)
    with pytest.raises(NotImplementedError):
        faiss.Kmeans(8, 2, frozen_centroids=True)
    with pytest.raises(NotImplementedError):
        km.train(np.zeros((300, 128), np.float32), weights=np.ones(300, np.float32))
    with pytest.raises(ValueError):
        faiss.Kmeans(0, 4)
    with pytest.raises(ValueError):
        faiss.Kmeans(8, 4, niter=0)
    with pytest.raises(ValueError):
        km.train(np.zeros((300, 64), np.float32))
    with pytest.raises(RuntimeError, match=r"Number of training points \(100\) should be at least as large "
                                           r"as number of clusters \(256\)"):
        km.train(np.zeros((100, 128), np.float32))
    with pytest.raises(ValueError, match="init_centroids"):
        km.train(np.zeros((300, 128), np.float32), init_centroids=np.zeros((3, 128), np.float32))
    with pytest.raises(RuntimeError, match="train before"):
        km.assign(np.zeros((1, 128), np.float32))


# ---- the C entry points: bad arguments are KNN_EINVAL before any GPU call ----------------------------
def _step(lib, x, n, d, c, k, flags=0, outs=True):
    o = [C.c_void_p(4096 * (i + 1)) for i in range(5)] if outs else [None] * 5     # never dereferenced
    return lib.kmeans_step_device(x, n, d, c, k, flags, *o, None)


def test_step_rejects_bad_arguments():
    lib = _lib.load()
    p = C.c_void_p(16)
    for args, word in [((p, 100, 8, p, 0), "k must be positive"), ((p, 100, 0, p, 4), "d must be positive"),
                       ((p, 100, -3, p, 4), "d must be positive"), ((p, 3, 8, p, 4), "at least as large"),
                       ((None, 100, 8, p, 4), "NULL"), ((p, 100, 8, None, 4), "NULL"),
                       ((p, 1 << 31, 8, p, 4), "2^31")]:
        assert _step(lib, *args) == _lib.KNN_EINVAL
        assert word in _lib.last_error(), (args, _lib.last_error())
    assert _step(lib, p, 100, 8, p, 4, outs=False) == _lib.KNN_EINVAL and "NULL output" in _lib.last_error()
    assert _step(lib, p, 100, 8, p, 4, flags=6) == _lib.KNN_EINVAL and "flags" in _lib.last_error()


def test_train_and_split_reject_bad_arguments():
    lib = _lib.load()
    x = np.zeros((10, 4), np.float32)
    out = np.zeros((3, 4), np.float32)
    obj = C.c_double()
    prm = _lib.KmeansParams(5, 1, 0, 0, 1234, -1)

    def train(xp, n, d, k, pp=C.byref(prm), outp=out.ctypes.data):
        return lib.kmeans_train(xp, n, d, k, pp, None, outp, C.byref(obj), None)

    for args, word in [((x.ctypes.data, 10, 4, 0), "k must be positive"),
                       ((x.ctypes.data, 10, 0, 3), "d must be positive"),
                       ((x.ctypes.data, 2, 4, 3), "at least as large"), ((None, 10, 4, 3), "NULL")]:
        assert train(*args) == _lib.KNN_EINVAL
        assert word in _lib.last_error(), (args, _lib.last_error())
    assert train(x.ctypes.data, 10, 4, 3, pp=None) == _lib.KNN_EINVAL
    assert train(x.ctypes.data, 10, 4, 3, outp=None) == _lib.KNN_EINVAL
    bad = _lib.KmeansParams(0, 1, 0, 0, 1234, -1)
    assert train(x.ctypes.data, 10, 4, 3, pp=C.byref(bad)) == _lib.KNN_EINVAL and "niter" in _lib.last_error()
    assert lib.kmeans_train_device(None, 10, 4, 3, C.byref(prm), None, out.ctypes.data, C.byref(obj), None,
                                   None) == _lib.KNN_EINVAL

    cnt = np.array([0, 1, 1], np.int64)
    ns = C.c_int(-1)
    p = C.c_void_p(16)
    assert lib.kmeans_split_device(p, 3, 4, cnt.ctypes.data, C.byref(ns), None) == _lib.KNN_EINVAL
    assert "no cluster with more than one member" in _lib.last_error()
    assert lib.kmeans_split_device(None, 3, 4, cnt.ctypes.data, C.byref(ns), None) == _lib.KNN_EINVAL
    assert lib.kmeans_split_device(p, 0, 4, cnt.ctypes.data, C.byref(ns), None) == _lib.KNN_EINVAL
    full = np.array([2, 1, 1], np.int64)            # nothing empty: nothing to do, no GPU needed
    assert lib.kmeans_split_device(p, 3, 4, full.ctypes.data, C.byref(ns), None) == 0 and ns.value == 0
