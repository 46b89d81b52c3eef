"""The three public views of a search's route agree (csrc/knn_plan.h choose_route is behind all three).

A search's chunk takes one of four routes, on one kernel, with one launch plan.  The library shows
that decision three ways: knn_plan_kernel names the kernel a search of (nq, k) runs, knn_plan gives
its tile and row-split counts, and knn_last_path says which route the last search actually took.
Each case runs one small search and asserts that

* knn_last_path is the route the kernel's name implies (knn_i8_scan_kernel: 3, knn_b16w_tile_kernel:
  2, knn_tile_topk_kernel<..., MODE, ...>: MODE);
* knn_plan's tile is the one that kernel instance has, and its split and workgroup counts are that
  plan's, restated here from the tile, the batch and the CU count;
* with timing on, the search recorded exactly one timed launch (one chunk).

IMGREC_CUS=8 plans for 8 CUs, so that 4096 rows still split.  What the routes compute is checked
elsewhere (test_i8_gpu, test_split_gpu, test_i8tail_gpu, ...): here only that the views agree.
"""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CUS = 8
K = 10
BIG_MIN_Q = 512          # kB16BigMinQ (csrc/knn_consts.h): batches from here run the 256 x 256 kernel


@pytest.fixture(scope="module")
def faiss(gpu):
    from image_recommender_amd import faiss_compat
    return faiss_compat


_DATA = {}


def _data(d, n):
    """n rows and BIG_MIN_Q queries, unit-norm, in C = n / 16 - 8 tight clusters (sigma 0.1 around
    Gaussian centres), row i in cluster i % C.  A cluster's 17 or so rows sit C rows apart: C / 8 is
    odd, so their 8-row groups go round the four row splits that 8 CUs give the 256 x 256 kernel
    (group g belongs to split g % 4), four or five rows to each.  No list of 10 then drops a row of
    a query's own cluster, and all of the cluster fits K' = 64: the int8 tail's trial search
    certifies every query and the index keeps the copy.  (Rows dealt to clusters at random put 11 or
    more of a cluster into one split for a few percent of the queries; those go to the exact re-run
    and the trial may drop the copy.)"""
    if (d, n) not in _DATA:
        rng = np.random.default_rng(61)
        nc = n // 16 - 8
        c = rng.standard_normal((nc, d))
        x = c[np.arange(n + BIG_MIN_Q) % nc] + 0.1 * rng.standard_normal((n + BIG_MIN_Q, d))
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        _DATA[d, n] = (x[:n], x[n:])
    return _DATA[d, n]


_INDEX = {}


def _index(faiss, d, n, monkeypatch):
    if (d, n) not in _INDEX:
        monkeypatch.setenv("IMGREC_CUS", str(CUS))
        idx = faiss.IndexFlatL2(d)                      # the knob is read here
        monkeypatch.delenv("IMGREC_CUS")
        idx.add(_data(d, n)[0])
        _INDEX[d, n] = idx
    return _INDEX[d, n]


def _views(idx, nq, k):
    """(tile rows, tile queries, splits, workgroups) of knn_plan and knn_plan_kernel's name."""
    from image_recommender_amd import _lib
    lib = _lib.load()
    tr, tq, sp, wg = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.knn_plan(idx.handle, nq, k, C.byref(tr), C.byref(tq), C.byref(sp), C.byref(wg)), "knn_plan")
    name = C.create_string_buffer(128)
    _lib.check(lib.knn_plan_kernel(idx.handle, nq, k, name, 128), "knn_plan_kernel")
    return (tr.value, tq.value, sp.value, wg.value), name.value.decode()


def _plan_of(name, n, d, nq):
    """(route, (tile rows, tile queries, splits, workgroups)) of the kernel instance `name` on n rows
    of d columns for nq queries on CUS CUs: DESIGN.md "Launch plan", restated."""
    m = re.fullmatch(r"knn_i8_scan_kernel<(\d+), (\d+), (\d+)>", name)
    if m:
        assert int(m.group(1)) == (nq if nq <= 2 else 4 if nq <= 4 else 8), name
        nblk = (d + 63) // 64
        assert int(m.group(3)) == (nblk + 15) // 16, name
        wgpcu = 1 if nq == 1 and nblk >= 24 else 2 if nq <= 2 else 3
        splits = max(1, min(CUS * wgpcu, (n + 7) // 8))
        return 3, (8, nq, splits, splits)
    m = re.fullmatch(r"knn_b16w_tile_kernel(_i8t)?<(\d+), [01], (true|false)>", name)
    if m:
        route, rows, queries, per_cu = 2, 256, 256, 1
    else:
        m = re.fullmatch(r"knn_tile_topk_kernel<(\d+), (\d+), \.\.\., ([012]), \.\.\.>", name)
        assert m, name
        route, rows, queries = int(m.group(3)), 128 * int(m.group(1)), 32 * int(m.group(2))
        per_cu = 3 if route == 0 and nq <= 32 else 2
    nqb = -(-nq // queries)
    splits = max(1, min(-(-CUS * per_cu // nqb), -(-n // rows)))
    return route, (rows, queries, splits, nqb * splits)


def _search_and_compare(idx, xq, n, d):
    from image_recommender_amd import _lib
    lib = _lib.load()
    nq = xq.shape[0]
    plan, name = _views(idx, nq, K)
    route, want = _plan_of(name, n, d, nq)
    assert plan == want, (name, plan, want)
    _lib.check(lib.knn_set_timing(idx.handle, 1), "knn_set_timing")
    try:
        idx.search(xq, K)
        ms, launches = C.c_double(), C.c_int()
        _lib.check(lib.knn_kernel_time(idx.handle, C.byref(ms), C.byref(launches)), "knn_kernel_time")
    finally:
        lib.knn_set_timing(idx.handle, 0)
    assert launches.value == 1, (name, launches.value)
    assert lib.knn_last_path(idx.handle) == route, (name, lib.knn_last_path(idx.handle))
    return name


# (search_mode = "split" needs d >= 256)
CASES = [(d, nq, mode) for d in (128, 256) for nq in (1, 8, 9, BIG_MIN_Q)
         for mode in ("auto", "exact", "bf16", "i8") + (("split",) if d >= 256 else ())]


@pytest.mark.parametrize("d,nq,mode", CASES)
def test_views_agree(faiss, monkeypatch, d, nq, mode):
    n = 4096
    idx = _index(faiss, d, n, monkeypatch)
    idx.search_mode = mode
    try:
        _search_and_compare(idx, _data(d, n)[1][:nq], n, d)
    finally:
        idx.search_mode = "auto"


def test_views_agree_across_the_int8_tail_build(faiss, monkeypatch):
    """AUTO, kB16BigMinQ queries on 2048 rows of 1024 columns: the first search builds the int8 tail
    copy, so the kernel's name gains its _i8t suffix exactly while the copy exists; route, plan and
    launch count are the same before and after."""
    from image_recommender_amd import _lib
    d, n = 1024, 2048
    idx = _index(faiss, d, n, monkeypatch)
    xq = _data(d, n)[1]

    def has_copy():
        return _lib.load().knn_debug_i8tail(idx.handle, None, None, 0, 0, None, None, None) == 0

    assert not has_copy()
    before = _search_and_compare(idx, xq, n, d)
    assert before.startswith("knn_b16w_tile_kernel<"), before
    assert has_copy()
    after = _search_and_compare(idx, xq, n, d)
    assert after == before.replace("knn_b16w_tile_kernel<", "knn_b16w_tile_kernel_i8t<"), (before, after)
    assert has_copy()
