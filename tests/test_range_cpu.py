"""CPU tests of the range search: the C ABI surface, argument validation, the oracle-side
conditions of every case the GPU tests run (tests/range_check.py CASES), and the checker itself
against planted faults.  No GPU compute.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from image_recommender_amd import _lib
from tests.range_check import (CASES, assert_conditions, check_range, make_case, oracle_result,
                               range_conditions)

ROOT = Path(__file__).resolve().parents[1]
RANGE_NAMES = ("knn_range_search", "knn_range_search_device", "knn_range_nq", "knn_range_size",
               "knn_range_copy", "knn_range_device", "knn_range_free")


def test_range_abi_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "imgrec_knn.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in RANGE_NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared in imgrec_knn.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported by the library"
    assert "index.range_search(x, thresh)" in (ROOT / "include" / "imgrec_knn.h").read_text()


def test_range_argument_validation():
    lib = _lib.load()
    out = C.c_void_p(123)
    q = np.zeros((1, 4), np.float32)
    rc = lib.knn_range_search(None, q.ctypes.data, 1, 1.0, C.byref(out))
    assert rc == _lib.KNN_EINVAL and out.value is None
    assert b"NULL" in lib.knn_last_error()
    # NULL out is rejected before the index is looked at (no index exists without a GPU: the
    # handle below is never dereferenced)
    fake = C.c_void_p(0x1000)
    assert lib.knn_range_search(fake, q.ctypes.data, 1, 1.0, None) == _lib.KNN_EINVAL
    assert lib.knn_range_search_device(None, None, 0, 1.0, None, C.byref(out)) == _lib.KNN_EINVAL
    assert lib.knn_range_search_device(fake, None, 0, 1.0, None, None) == _lib.KNN_EINVAL
    assert lib.knn_range_free(None) == _lib.KNN_OK
    assert lib.knn_range_nq(None) < 0 and lib.knn_range_size(None) < 0
    assert lib.knn_range_copy(None, None, None, None) == _lib.KNN_EINVAL
    assert lib.knn_range_device(None, None, None, None) == _lib.KNN_EINVAL


def test_python_surface():
    from image_recommender_amd import faiss_compat as faiss
    for cls in (faiss.Index, faiss.IndexFlat, faiss.IndexFlatL2, faiss.IndexFlatIP,
                faiss.IndexHNSWFlat, faiss.IndexIVFPQ):
        assert callable(getattr(cls, "range_search")) and callable(getattr(cls, "range_search_device"))
    for attr in ("device_ptrs", "to_host"):
        assert callable(getattr(faiss.RangeResult, attr))


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_conditions_hold(name):
    """band <= 2 % of expected and expected >= 5 nq, from the oracle alone, for every table entry."""
    xb, xq, radius, metric, d64, b = make_case(name)
    N, d, nq = CASES[name][:3]
    assert xb.shape == (N, d) and xq.shape == (nq, d)
    band, expected = range_conditions(xb, xq, radius, metric, d64, b)
    print(f"{name}: radius {radius:.6g}, expected {expected} ({expected / nq:.1f} per query), band {band}")
    assert_conditions(band, expected, nq)


@pytest.fixture(scope="module")
def good():
    xb, xq, radius, metric, d64, b = make_case("l2_1000x96_q33")
    lims, D, I = oracle_result(xb, xq, radius, metric, d64)
    return xb, xq, radius, metric, d64, b, lims, D, I


def _busy_query(lims):
    return int(np.argmax(np.diff(lims)))


def test_checker_accepts_the_oracle_result(good):
    xb, xq, radius, metric, d64, b, lims, D, I = good
    band, expected = check_range(lims, D, I, xb, xq, radius, metric, d64, b)
    assert_conditions(band, expected, xq.shape[0])
    xi, qi, ri, mi, d64i, bi = make_case("ip_1000x96_q33")
    check_range(*oracle_result(xi, qi, ri, mi, d64i), xi, qi, ri, mi, d64i, bi)


def test_checker_rejects_a_missing_hit(good):
    xb, xq, radius, metric, d64, b, lims, D, I = good
    q = _busy_query(lims)
    at = lims[q]                                   # the query's best hit: far inside the radius
    lims2 = lims.copy()
    lims2[q + 1:] -= 1
    with pytest.raises(AssertionError, match="missing"):
        check_range(lims2, np.delete(D, at), np.delete(I, at), xb, xq, radius, metric, d64, b)


def test_checker_rejects_an_extra_far_hit(good):
    xb, xq, radius, metric, d64, b, lims, D, I = good
    q = _busy_query(lims)
    far = int(np.argmax(d64[q]))
    at = lims[q + 1]
    lims2 = lims.copy()
    lims2[q + 1:] += 1
    # reported with a distance that passes (b) and keeps the segment sorted: only (c) / (d) see it
    D2 = np.insert(D, at, np.nextafter(np.float32(radius), np.float32(0)))
    I2 = np.insert(I, at, far)
    with pytest.raises(AssertionError):
        check_range(lims2, D2, I2, xb, xq, radius, metric, d64, b)
    # and with its true distance: (b) and (d)
    D3 = np.insert(D, at, np.float32(d64[q, far]))
    with pytest.raises(AssertionError):
        check_range(lims2, D3, I2, xb, xq, radius, metric, d64, b)


def test_checker_rejects_an_unsorted_segment(good):
    xb, xq, radius, metric, d64, b, lims, D, I = good
    q = _busy_query(lims)
    a, z = lims[q], lims[q + 1] - 1
    assert D[a] != D[z]
    D2, I2 = D.copy(), I.copy()
    D2[[a, z]], I2[[a, z]] = D[[z, a]], I[[z, a]]
    with pytest.raises(AssertionError, match="not sorted"):
        check_range(lims, D2, I2, xb, xq, radius, metric, d64, b)


def test_checker_rejects_wrong_lims(good):
    xb, xq, radius, metric, d64, b, lims, D, I = good
    q = _busy_query(lims)
    bad = lims.copy()
    bad[q + 1] -= 1                                # the query's last hit handed to the next query
    with pytest.raises(AssertionError):
        check_range(bad, D, I, xb, xq, radius, metric, d64, b)
    bad = lims.copy()
    bad[-1] += 1
    with pytest.raises(AssertionError):
        check_range(bad, D, I, xb, xq, radius, metric, d64, b)
    bad = lims.copy()
    bad[0] = 1
    with pytest.raises(AssertionError):
        check_range(bad, D, I, xb, xq, radius, metric, d64, b)
