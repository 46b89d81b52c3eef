"""The int8 tail of the 256 x 256 candidate kernel on the GPU (csrc/knn_b16w.hip
knn_b16w_tile_kernel_i8t, DESIGN.md "int8 tail"; IMGREC_B16W_I8TAIL, read at index creation).

AUTO sends batches of >= 512 queries with k <= 10 to the sibling kernel once the index has built
its int8 tail copy.  Every candidate route returns the rerank's exact fp32 keys of the certified top
k, so each case compares (D, I) bit for bit with search_mode = "bf16" on the same index; against
search_mode = "exact", whose keys come out of another fp32 arithmetic (the fp32 MFMA tile), the keys
are held to the rounding of one such evaluation and the labels to the float64 oracle of
tests/knn_check.py.  Each case also checks the kernel name, the certificate's error ratio and the
exact re-runs.  20,000 rows: every row split (79 of them
on a 256-CU device) holds one partial 256-row tile, the smallest shape that runs the first-tile
path, the partial-tile path and pad queries.
"""
import ctypes as C

import numpy as np
import pytest

from tests import i8tail_ref as R
from tests.datagen import mixture
from tests.knn_check import check_knn

pytestmark = pytest.mark.gpu

N_ = 20_000


@pytest.fixture(scope="module")
def faiss(gpu):
    from image_recommender_amd import faiss_compat
    return faiss_compat


def _rows(n, d, seed, lead):
    """Unit-norm rows in 640 tight clusters (about 31 rows each, sigma 0.1 around centres sqrt(2)
    apart): a query's neighbours are its cluster's rows, well separated from every other row, so the
    exact reference's top k is far from the rest and K' = 64 holds the int8 band.  (Rows drawn with
    sigma 0.5 around 40 centres concentrate every in-cluster distance within the int8 bound; there
    the certificate sends most queries to the second chance — the data's doing, not the kernel's.)
    lead: 48 leading columns six times larger (they belong in the head)."""
    x = mixture(n, d, centres=640, sigma=0.1, seed=seed, normalize=True)
    if lead:
        x[:, :48] *= np.float32(6.0)
    return x


_DATA = {}


def _data(d, lead):
    if (d, lead) not in _DATA:
        x = _rows(N_ + 600, d, 51, lead)             # queries from the corpus's own clusters
        _DATA[d, lead] = (x[:N_], x[N_:])
    return _DATA[d, lead]


def _new(faiss, d, metric, monkeypatch, on=True):
    if not on:
        monkeypatch.setenv("IMGREC_B16W_I8TAIL", "0")
    idx = faiss.IndexFlatL2(d) if metric == "l2" else faiss.IndexFlatIP(d)     # the knob is read here
    if not on:
        monkeypatch.delenv("IMGREC_B16W_I8TAIL")
    return idx


def _kernel(idx, nq, k):
    from image_recommender_amd import _lib
    name = C.create_string_buffer(128)
    _lib.check(_lib.load().knn_plan_kernel(idx.handle, nq, k, name, 128), "knn_plan_kernel")
    return name.value.decode()


def _tail(idx, i0=0, n=None):
    """(head, dpt, codes, scales, stats) of rows [i0, i0 + n) through knn_debug_i8tail."""
    from image_recommender_amd import _lib
    lib = _lib.load()
    h, t = C.c_int(), C.c_int()
    _lib.check(lib.knn_debug_i8tail(idx.handle, C.byref(h), C.byref(t), 0, 0, None, None, None), "knn_debug_i8tail")
    n = idx.ntotal - i0 if n is None else n
    codes = np.empty((n, t.value), np.int8)
    scales = np.empty(n, np.float32)
    stats = np.empty((n, 4), np.float32)
    _lib.check(lib.knn_debug_i8tail(idx.handle, None, None, i0, n, codes.ctypes.data, scales.ctypes.data,
                                    stats.ctypes.data), "knn_debug_i8tail")
    return h.value, t.value, codes, scales, stats


_XNORM_MAX = [0.0]       # the largest row norm of the index under test (set by _add)


def _add(idx, xb):
    idx.add(xb)
    _XNORM_MAX[0] = float(np.linalg.norm(xb, axis=1).max())


def _three_ways(idx, xq, k, rerun_cap=0, ref=None):
    """AUTO (the int8 tail), then exact and bf16 on the same index; ref = (xb, metric): the labels
    against the float64 oracle as well.  Returns AUTO's (D, I, stats)."""
    idx.search_mode = "auto"
    D, I = idx.search(xq, k)
    st = idx.certificate_stats()
    name = _kernel(idx, xq.shape[0], k)
    assert name.startswith("knn_b16w_tile_kernel_i8t<") and name.endswith("true>"), name
    assert st["candidate_queries"] == xq.shape[0] and 0.0 <= st["max_err_over_bound"] < 1.0, st
    assert st["exact_reruns"] <= rerun_cap, st
    for mode in ("exact", "bf16"):
        idx.search_mode = mode
        if mode == "bf16":
            assert _kernel(idx, xq.shape[0], k).startswith("knn_b16w_tile_kernel<")
        Dm, Im = idx.search(xq, k)
        if mode == "bf16" and st["exact_reruns"] == 0:
            assert np.array_equal(I, Im), (mode, np.argwhere(I != Im)[:5])
            assert np.array_equal(D, Dm), (mode, float(np.abs(D - Dm).max()))
        else:
            # the exact route's keys (and those of queries the certificate re-ran exactly) come out
            # of the fp32 MFMA tile, the candidate routes' out of the rerank's FMA chains: two fp32
            # evaluations of the same key, each within gamma_d of the terms' scale (|q| + |x|)^2, so
            # they agree to 2 d 2^-24 of it, not to the bit (the pure bf16 route differs from the
            # exact one in the same way)
            scale = float((np.linalg.norm(xq, axis=1).max() + _XNORM_MAX[0]) ** 2)
            tol = 2.0 * xq.shape[1] * 2.0 ** -24 * scale
            print(f"i8tail vs exact keys: max |dD| {float(np.abs(D - Dm).max()):.3g}, tolerance {tol:.3g}")
            assert float(np.abs(D - Dm).max()) <= tol, (mode, float(np.abs(D - Dm).max()), tol)
    if ref is not None:        # labels and keys inside the float64 oracle's rigorous windows
        check_knn(D, I, ref[0], xq, k, ref[1], min_exact_frac=0.0)
    idx.search_mode = "auto"
    return D, I, st


def _check_copy(idx, xb, head, dpb):
    h, dpt, codes, scales, stats = _tail(idx)
    assert (h, dpt) == (head, (dpb - head + 127) // 128 * 128)
    rc, rs = R.quantize_tail(xb, head, dpb, dpt)
    assert np.array_equal(codes, rc) and np.array_equal(scales, rs)
    assert (stats.astype(np.float64) >= R.row_stats64(xb, head, dpb, rc, rs)).all()


# d = 704 with 48 large leading columns: H = 64, five tail stages exactly; d = 760: 8 pad columns in
# the bf16 rows, 72 pad codes; d = 768 homogeneous: H = 0, no head stage
CASES = [(704, True, 64, 704), (760, True, 64, 768), (768, False, 0, 768)]


@pytest.mark.parametrize("d,lead,head,dpb", CASES)
@pytest.mark.parametrize("metric,nq,k", [("l2", 512, 10), ("ip", 600, 8), ("l2", 600, 8), ("ip", 512, 10)])
def test_equals_exact_and_bf16(faiss, monkeypatch, d, lead, head, dpb, metric, nq, k):
    xb, xq = _data(d, lead)
    idx = _new(faiss, d, metric, monkeypatch)
    _add(idx, xb)
    _three_ways(idx, xq[:nq], k, ref=(xb, metric))          # clustered rows: no exact re-run allowed
    if metric == "l2" and nq == 512:
        _check_copy(idx, xb, head, dpb)


def test_state_changes(faiss, monkeypatch):
    """Adds after the build, remove_ids, regrowth and reset keep the copy current."""
    d = 704
    xb, xq = _data(d, True)
    xq = xq[:512]
    idx = _new(faiss, d, "l2", monkeypatch)
    _add(idx, xb[:9_000])
    _three_ways(idx, xq, 10)                                # builds the copy (capacity 9216 rows)
    _add(idx, xb[9_000:15_000])                             # regrowth + rows added after the build
    _three_ways(idx, xq, 10)
    _check_copy(idx, xb[:15_000], 64, 704)
    rm = np.arange(3, 15_000, 7)
    assert idx.remove_ids(rm) == rm.size
    keep = np.setdiff1d(np.arange(15_000), rm)
    _three_ways(idx, xq, 10)
    _check_copy(idx, xb[keep], 64, 704)
    idx.reset()                                             # the split column is chosen again
    homog, hq = _data(768, False)
    _add(idx, homog[:12_000, :d].copy())
    _three_ways(idx, np.ascontiguousarray(hq[:512, :d]), 10)
    assert _tail(idx, 0, 1)[0] == 0


def test_ineligible_and_knob(faiss, monkeypatch):
    """A short tail (d = 512 with a 64-column head) and IMGREC_B16W_I8TAIL=0 keep the bf16 kernel."""
    x = _rows(N_ + 512, 512, 53, True)
    xb, xq = x[:N_], x[N_:]
    idx = _new(faiss, 512, "l2", monkeypatch)
    _add(idx, xb)
    D, I = idx.search(xq, 10)
    assert _kernel(idx, 512, 10).startswith("knn_b16w_tile_kernel<")
    idx.search_mode = "bf16"
    Db, Ib = idx.search(xq, 10)
    assert np.array_equal(I, Ib) and np.array_equal(D, Db)
    check_knn(D, I, xb, xq, 10, "l2", min_exact_frac=0.0)
    xb, xq = _data(704, True)
    off = _new(faiss, 704, "l2", monkeypatch, on=False)
    off.add(xb)
    D0, I0 = off.search(xq[:512], 10)
    assert _kernel(off, 512, 10).startswith("knn_b16w_tile_kernel<")
    on = _new(faiss, 704, "l2", monkeypatch)
    _add(on, xb)
    D1, I1, _ = _three_ways(on, xq[:512], 10)
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)


def test_duplicated_rows(faiss, monkeypatch):
    """16 copies of one row, all in 8-row groups of one row split (on a 256-CU device), and the
    row as a query: ties go to the smaller label.  Queries allowed to fall back to the exact
    re-run: that one (its answer is 10 equal keys in one list, which no certificate separates) — a
    cap counted from the rows perturbed here, not measured."""
    d = 704
    xb, xq = _data(d, True)
    xb, xq = xb.copy(), xq[:512].copy()
    rng = np.random.default_rng(9)
    dup = np.array([8 * (5 + 79 * j) + 1 for j in range(16)])
    assert dup.max() < N_
    xb[dup] = rng.choice(np.float32([-0.25, 0.25]), d)       # |q|^2 + |x|^2 - 2 q.x is exactly 0
    xq[2] = xb[dup[0]]
    idx = _new(faiss, d, "l2", monkeypatch)
    _add(idx, xb)
    D, I, st = _three_ways(idx, xq, 10, rerun_cap=1, ref=(xb, "l2"))
    np.testing.assert_array_equal(I[2], dup[:10])
    assert (D[2] == 0.0).all()


def _auto(idx, xq, k):
    idx.search_mode = "auto"
    D, I = idx.search(xq, k)
    return D, I, idx.certificate_stats(), _kernel(idx, xq.shape[0], k)


def test_rows_with_one_huge_tail_element(faiss, monkeypatch):
    """20 rows with one tail element of 30, added after the copy was built (in the corpus from the
    start they move the split column past them and the short tail turns the route off): their
    scale leaves every other code 0, so their tail residual is their whole tail and R_t, a corpus
    maximum, grows to ~1 for EVERY query.  The first search after the add is a trial again: its
    results are exact whatever the certificate needed, and the index keeps the route exactly when
    that search re-ran at most 1/32 of the batch — so no later search pays more than that share."""
    d = 704
    xb, xq = _data(d, True)
    xq = xq[:512].copy()
    idx = _new(faiss, d, "l2", monkeypatch)
    _add(idx, xb)
    _three_ways(idx, xq, 10)
    bad = xb[100:120].copy()
    bad[:, 200] = 30.0
    xq[3] = bad[4]                                           # a query that is such a row
    _add(idx, bad)
    allx = np.concatenate([xb, bad])
    D, I, st, name = _auto(idx, xq, 10)
    print("huge tail elements: trial search", st, name)
    assert st["candidate_queries"] == 512 and 0.0 <= st["max_err_over_bound"] < 1.0, st
    assert I[3, 0] == N_ + 4 and D[3, 0] == 0.0
    check_knn(D, I, allx, xq, 10, "l2", min_exact_frac=0.0)
    kept = st["exact_reruns"] * 32 <= 512
    assert name.startswith("knn_b16w_tile_kernel_i8t<" if kept else "knn_b16w_tile_kernel<"), (name, st)
    D2, I2, st2, _ = _auto(idx, xq, 10)                      # after the trial: never past the share
    assert st2["exact_reruns"] * 32 <= 512, st2
    check_knn(D2, I2, allx, xq, 10, "l2", min_exact_frac=0.0)
    if not kept:                                             # dropped: the bf16 pass's own bits
        idx.search_mode = "bf16"
        Db, Ib = idx.search(xq, 10)
        assert np.array_equal(I2, Ib) and np.array_equal(D2, Db)


def test_trial_drops_a_losing_index(faiss, monkeypatch):
    """768 homogeneous columns (H = 0) and 600 queries far from every cluster of the corpus: all
    rows' keys sit inside the int8 band and the certificate re-runs far more than 1/32 of the batch
    exactly.  That first search is the copy's trial: its results are exact, and from then on the
    index reports and runs the bf16 kernel, with the bf16 route's bits."""
    xb, _ = _data(768, False)
    xq = _rows(600, 768, 52, False)                          # other centres than the corpus's
    idx = _new(faiss, 768, "l2", monkeypatch)
    _add(idx, xb)
    assert _kernel(idx, 600, 10).startswith("knn_b16w_tile_kernel<")        # nothing decided yet
    D, I, st, name = _auto(idx, xq, 10)
    print("losing index: trial search", st, name)
    assert st["exact_reruns"] * 32 > 600, st                 # the premise of this case
    assert name.startswith("knn_b16w_tile_kernel<"), name
    check_knn(D, I, xb, xq, 10, "l2", min_exact_frac=0.0)
    D2, I2, st2, name2 = _auto(idx, xq, 10)
    assert name2.startswith("knn_b16w_tile_kernel<")
    idx.search_mode = "bf16"
    Db, Ib = idx.search(xq, 10)
    assert np.array_equal(I2, Ib) and np.array_equal(D2, Db)
    with pytest.raises(Exception):
        _tail(idx, 0, 1)                                     # the copy is gone
