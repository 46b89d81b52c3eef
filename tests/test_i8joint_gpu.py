"""The joint rows of the int8 tail copy on the GPU (csrc/knn_b16w.hip knn_b16w_tile_kernel_i8t,
DESIGN.md "int8 tail": a row of the copy is its dpt tail codes, then its first H columns as bf16, and
the kernel stages 128 B of that row per stage for both operands).

tests/test_i8tail_gpu.py holds the route at H = 64 and H = 0.  Here the head is more than one stage
and the joint stride is neither the bf16 rows' nor the codes' own:

* d = 832 with 176 large leading columns: H = 192 (three head stages), 640 tail columns (five tail
  stages exactly), joint row 1024 B;
* d = 700 with 100 large leading columns: dpb 704, H = 128, 576 tail columns padded to 640 codes,
  joint row 896 B.

Row counts are no multiple of 8 or 256, chosen so that (on a 256-CU device) the row splits' last,
partial tiles have 1, 2 and 4 live quad rows of 64 rows over the cases; the tile counts are worked out
from knn_plan's row_splits and the last test asserts that the three paths occurred.  Every case
compares AUTO's (D, I) bit for bit with search_mode = "bf16" on the same index (both return the
rerank's exact fp32 keys of the certified top k) and holds the labels to the float64 oracle of
tests/knn_check.py, with no exact re-run (clustered rows, as in tests/test_i8tail_gpu.py).
"""
import ctypes as C

import numpy as np
import pytest

from tests import i8tail_ref as R
from tests.datagen import mixture
from tests.knn_check import check_knn

pytestmark = pytest.mark.gpu

# d -> (large leading columns, H, dpb, dpt, joint row bytes)
SHAPES = {832: (176, 192, 832, 640, 1024), 700: (100, 128, 704, 640, 896)}
# (d, rows, metric, queries, k); the live quad rows of the splits' last tiles on 256 CUs:
# 20,003 rows: 4 (79 splits of 31 or 32 groups); 40,011 x 512 queries: 1 (128 splits of 39 or 40
# groups: 7 or 8 in the second tile); 30,003 and 28,003 x 600 queries: 2, or 1 and 2 (86 splits)
CASES = [(832, 20_003, "l2", 512, 10), (832, 20_003, "ip", 600, 8), (700, 40_011, "ip", 512, 10),
         (700, 40_011, "l2", 600, 8), (832, 30_003, "l2", 600, 10), (700, 28_003, "ip", 600, 8)]
N_MAX = 40_011


@pytest.fixture(scope="module")
def faiss(gpu):
    from image_recommender_amd import faiss_compat
    return faiss_compat


_DATA = {}


def _data(d):
    """Unit-norm rows in 640 tight clusters (tests/test_i8tail_gpu.py _rows) with the shape's leading
    columns six times larger; the queries come from the corpus's own clusters."""
    if d not in _DATA:
        x = mixture(N_MAX + 600, d, centres=640, sigma=0.1, seed=61, normalize=True)
        x[:, :SHAPES[d][0]] *= np.float32(6.0)
        _DATA[d] = (x[:N_MAX], x[N_MAX:])
    return _DATA[d]


def _lib():
    from image_recommender_amd import _lib
    return _lib


def _new(faiss, d, metric):
    return faiss.IndexFlatL2(d) if metric == "l2" else faiss.IndexFlatIP(d)


def _kernel(idx, nq, k):
    name = C.create_string_buffer(128)
    _lib().check(_lib().load().knn_plan_kernel(idx.handle, nq, k, name, 128), "knn_plan_kernel")
    return name.value.decode()


def _codes(idx):
    """(head, dpt, codes) of every row through knn_debug_i8tail."""
    lib = _lib().load()
    h, t = C.c_int(), C.c_int()
    _lib().check(lib.knn_debug_i8tail(idx.handle, C.byref(h), C.byref(t), 0, 0, None, None, None), "knn_debug_i8tail")
    codes = np.empty((idx.ntotal, t.value), np.int8)
    _lib().check(lib.knn_debug_i8tail(idx.handle, None, None, 0, idx.ntotal, codes.ctypes.data, None, None),
                 "knn_debug_i8tail")
    return h.value, t.value, codes


def _joint(idx):
    """(row bytes, raw joint rows) of every row through knn_debug_i8tail_rows."""
    lib = _lib().load()
    rb = C.c_int()
    _lib().check(lib.knn_debug_i8tail_rows(idx.handle, 0, 0, C.byref(rb), None), "knn_debug_i8tail_rows")
    rows = np.empty((idx.ntotal, rb.value), np.uint8)
    _lib().check(lib.knn_debug_i8tail_rows(idx.handle, 0, idx.ntotal, None, rows.ctypes.data), "knn_debug_i8tail_rows")
    return rb.value, rows


def _bf16_bits(x):
    """fp32 -> the bits of the nearest bf16 (ties to even), as uint16."""
    return (R.bf16_rne(x).view(np.uint32) >> 16).astype(np.uint16)


def _check_joint(idx, xb, d):
    """The copy of an index holding exactly the rows xb: H by the rule, the codes against numpy, and
    every joint row = [codes | bf16 of the row's first H columns]."""
    _, head, dpb, dpt, row = SHAPES[d]
    h, t, codes = _codes(idx)
    assert h == R.pick_head(R.block_absmax(xb, dpb)) == head and t == dpt
    rb, rows = _joint(idx)
    assert rb == row == dpt + 2 * head and rows.shape == (xb.shape[0], row)
    assert np.array_equal(codes, R.quantize_tail(xb, head, dpb, dpt)[0])
    assert np.array_equal(rows[:, :dpt].view(np.int8), codes)
    got = np.ascontiguousarray(rows[:, dpt:]).view(np.uint16)
    assert np.array_equal(got, _bf16_bits(xb[:, :head]))


def _live_quads(idx, n, nq, k):
    """The live quad rows (64 tile rows each) of every row split's last tile, from knn_plan's
    row_splits: split s holds the 8-row groups s, s + splits, ...; a tile holds 32 of them."""
    tr, tq, sp, wg = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib().check(_lib().load().knn_plan(idx.handle, nq, k, C.byref(tr), C.byref(tq), C.byref(sp), C.byref(wg)),
                 "knn_plan")
    assert (tr.value, tq.value) == (256, 256)
    groups, live = (n + 7) // 8, set()
    for s in range(sp.value):
        cnt = (groups - s + sp.value - 1) // sp.value if s < groups else 0
        last = cnt - (cnt - 1) // 32 * 32 if cnt else 0          # groups of the last tile
        live.add((last * 8 + 63) // 64)
    return live


_LIVE = {}


def _auto_equals_bf16(idx, xq, k, xb, metric):
    idx.search_mode = "auto"
    D, I = idx.search(xq, k)
    st = idx.certificate_stats()
    name = _kernel(idx, xq.shape[0], k)
    assert name.startswith("knn_b16w_tile_kernel_i8t<") and name.endswith("true>"), name
    assert st["candidate_queries"] == xq.shape[0] and 0.0 <= st["max_err_over_bound"] < 1.0, st
    assert st["exact_reruns"] == 0, st
    idx.search_mode = "bf16"
    assert _kernel(idx, xq.shape[0], k).startswith("knn_b16w_tile_kernel<")
    Db, Ib = idx.search(xq, k)
    assert idx.certificate_stats()["exact_reruns"] == 0      # the reference route re-ran nothing either
    assert np.array_equal(I, Ib), np.argwhere(I != Ib)[:5]
    assert np.array_equal(D, Db), float(np.abs(D - Db).max())
    check_knn(D, I, xb, xq, k, metric, min_exact_frac=0.0)
    idx.search_mode = "auto"


@pytest.mark.parametrize("d,n,metric,nq,k", CASES)
def test_route_on_joint_rows(faiss, d, n, metric, nq, k):
    xb, xq = _data(d)
    xb, xq = xb[:n], xq[:nq]
    assert n % 8 != 0 and n % 256 != 0
    idx = _new(faiss, d, metric)
    idx.add(xb)
    _auto_equals_bf16(idx, xq, k, xb, metric)
    _LIVE[d, n, nq, k] = _live_quads(idx, n, nq, k)
    if nq == 512:
        _check_joint(idx, xb, d)


def test_joint_rows_through_state_changes(faiss):
    """The joint rows after the build, an add into spare capacity, a regrowth (reserve_rows), and a
    remove_ids whose compaction moves rows across 8-row group boundaries."""
    d = 832
    xb, xq = _data(d)
    xq = xq[:512]
    idx = _new(faiss, d, "l2")
    idx.add(xb[:9_003])
    _auto_equals_bf16(idx, xq, 10, xb[:9_003], "l2")        # builds the copy (capacity 9216 rows)
    _check_joint(idx, xb[:9_003], d)
    idx.add(xb[9_003:9_150])                                # fits the capacity: the add path alone
    _check_joint(idx, xb[:9_150], d)
    idx.add(xb[9_150:15_005])                               # regrowth, then rows added after it
    _check_joint(idx, xb[:15_005], d)
    _auto_equals_bf16(idx, xq, 10, xb[:15_005], "l2")
    rm = np.arange(3, 15_005, 7)                            # every survivor past row 3 moves, by 1 .. 2143 rows
    assert idx.remove_ids(rm) == rm.size
    keep = np.setdiff1d(np.arange(15_005), rm)
    _check_joint(idx, xb[keep], d)
    _auto_equals_bf16(idx, xq, 10, xb[keep], "l2")


def test_no_copy_stays_on_bf16(faiss, monkeypatch):
    """An index whose copy cannot be allocated (IMGREC_I8TAIL_ALLOC_FAIL=1, read at creation) and one
    that is ineligible (a 448-column tail behind H = 64) search on the bf16 kernel, with its bits."""
    d = 700
    xb, xq = _data(d)
    xb, xq = xb[:20_003], xq[:512]
    monkeypatch.setenv("IMGREC_I8TAIL_ALLOC_FAIL", "1")
    full = _new(faiss, d, "l2")
    monkeypatch.delenv("IMGREC_I8TAIL_ALLOC_FAIL")
    short = _new(faiss, 512, "l2")
    xs = np.ascontiguousarray(xb[:, :512])                  # H = 128 leaves 384 tail columns < 512
    assert R.pick_head(R.block_absmax(xs, 512)) == -1
    for idx, rows, q in ((full, xb, xq), (short, xs, np.ascontiguousarray(xq[:, :512]))):
        idx.add(rows)
        D, I = idx.search(q, 10)
        assert _kernel(idx, 512, 10).startswith("knn_b16w_tile_kernel<")
        with pytest.raises(Exception):
            _joint(idx)                                      # no copy
        idx.search_mode = "bf16"
        Db, Ib = idx.search(q, 10)
        assert np.array_equal(I, Ib) and np.array_equal(D, Db)
        check_knn(D, I, rows, q, 10, "l2", min_exact_frac=0.0)


def test_every_nlive_path_ran(faiss):
    """Over the cases the row splits' last tiles have 1, 2 and 4 live quad rows (a case that did not
    run in this process is planned here: its index without a search)."""
    for d, n, metric, nq, k in CASES:
        if (d, n, nq, k) not in _LIVE:
            idx = _new(faiss, d, metric)
            idx.add(_data(d)[0][:n])
            _LIVE[d, n, nq, k] = _live_quads(idx, n, nq, k)
    seen = set().union(*_LIVE.values())
    print("live quad rows of the last tiles:", {c: sorted(v) for c, v in _LIVE.items()})
    assert {1, 2, 4} <= seen, _LIVE
