"""HIP tests of remove_ids (faiss Index::remove_ids on the MI355X index): after a removal the index
must be, bit for bit, the index a fresh build from the surviving rows gives — the stored rows, the
norms (through range_search and the filtered search, whose keys depend on the pair alone) and every
derived copy that existed before the removal (through the search mode that reads it).

Shapes: d = 48 (no bf16 / int8 copy), d = 80 (bf16 copy, an int8 row of 2 blocks, padded row stride)
and d = 1968 (split copy allowed, 31 int8 blocks); N is never a multiple of the 256-row tile.  The
bounce chunk is forced to tests.remove_check.CHUNK rows (IMGREC_REMOVE_CHUNK) so that every case
moves its rows in several chunks; one case runs with the default chunk.

Candidate modes (bf16 / i8 / split): the result after a removal is compared byte for byte with the
fresh index's whenever the fresh index searched twice gives equal bytes (printed otherwise); the
certificate checks hold either way.
"""
import ctypes as C
import os
import pickle
import sqlite3
from pathlib import Path

import numpy as np
import pytest

from tests.datagen import mixture
from tests.knn_check import check_knn
from tests.remove_check import CHUNK, PATTERNS, bitmap, keep_of, pattern, survivors

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
SHAPES = {48: 1000, 80: 1000, 1968: 700}
NQ, K = 8, 10
PATH_OF = {"exact": 0, "split": 1, "bf16": 2, "i8": 3}
CASES = [(d, "l2") for d in SHAPES] + [(80, "cosine"), (80, "ip")]


@pytest.fixture(scope="module")
def faiss(gpu):
    from image_recommender_amd import faiss_compat
    old = os.environ.get("IMGREC_REMOVE_CHUNK")
    os.environ["IMGREC_REMOVE_CHUNK"] = str(CHUNK)        # read when an index is created
    yield faiss_compat
    if old is None:
        os.environ.pop("IMGREC_REMOVE_CHUNK", None)
    else:
        os.environ["IMGREC_REMOVE_CHUNK"] = old


def _index(faiss, d, metric, **kw):
    if metric == "l2":
        return faiss.IndexFlatL2(d, **kw)
    if metric == "ip":
        return faiss.IndexFlatIP(d, **kw)
    return faiss.IndexFlat(d, faiss.METRIC_COSINE, **kw)


_data = {}


def _rows(d):
    """(xb, xq, extra rows for later adds) of a shape: one mixture, so queries have neighbours."""
    if d not in _data:
        n = SHAPES[d]
        x = mixture(n + NQ + 87, d, centres=20, seed=100 + d)
        _data[d] = (np.ascontiguousarray(x[:n]), np.ascontiguousarray(x[n:n + NQ]),
                    np.ascontiguousarray(x[n + NQ:]))
    return _data[d]


def _modes(d):
    return ["exact"] + (["bf16", "i8"] if d >= 64 else []) + (["split"] if d >= 256 else [])


def _nq(mode):
    return 4 if mode == "i8" else NQ


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert x.tobytes() == y.tobytes()


def _last_path(idx):
    from image_recommender_amd import _lib
    return _lib.load().knn_last_path(idx.handle)


def _materialise(idx, d, xq):
    """One search per candidate mode, so its copy of the rows exists from here on."""
    for mode in _modes(d):
        idx.search_mode = mode
        idx.search(xq[:_nq(mode)], K)
        assert _last_path(idx) == PATH_OF[mode]
    idx.search_mode = "auto"


_built = {}


def _removed_and_fresh(faiss, d, metric, name):
    """(index after remove_ids with every copy materialised before, fresh index of the survivors,
    the survivors, the return value), built once per case."""
    key = (d, metric, name)
    if key not in _built:
        xb, xq, _ = _rows(d)
        mask = pattern(name, len(xb))
        idx = _index(faiss, d, metric)
        idx.add(xb)
        _materialise(idx, d, xq)
        removed = idx.remove_ids(faiss.IDSelectorBitmap(bitmap(mask)))
        fresh = _index(faiss, d, metric)
        left = survivors(xb, mask)
        if len(left):
            fresh.add(left)
        _built[key] = (idx, fresh, left, removed)
    return _built[key]


def _random_mask(n, seed):
    return np.random.default_rng(seed).random(n) < 0.5


def _assert_rows_and_pair_keys_equal(faiss, idx, fresh, xq, metric):
    """Checks 1 and 2: the stored rows, and the keys that depend on (query, row, norm) alone."""
    assert idx.ntotal == fresh.ntotal
    n = idx.ntotal
    _same([idx.reconstruct_n(0, n)], [fresh.reconstruct_n(0, n)])
    radius = np.inf if metric == "l2" else -np.inf
    _same(idx.range_search(xq, radius), fresh.range_search(xq, radius))
    p = faiss.SearchParameters(sel=faiss.IDSelectorBitmap(bitmap(_random_mask(n, n + 1))))
    _same(idx.search(xq, K, params=p), fresh.search(xq, K, params=p))


# ---- 1, 2: rows and norms -----------------------------------------------------------------------
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("d,metric", CASES)
def test_rows_and_norms_equal_a_fresh_index(faiss, d, metric, name):
    xb, xq, _ = _rows(d)
    mask = pattern(name, len(xb))
    idx, fresh, left, removed = _removed_and_fresh(faiss, d, metric, name)
    assert removed == int(mask.sum()) and idx.ntotal == len(xb) - removed == len(left)
    if metric != "cosine" and len(left):
        _same([idx.reconstruct_n(0, idx.ntotal)], [left])
    _assert_rows_and_pair_keys_equal(faiss, idx, fresh, xq, metric)


# ---- 3: every copy that existed before the removal ----------------------------------------------
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("d,metric", CASES)
def test_every_search_mode_after_removal(faiss, d, metric, name):
    xb, xq, _ = _rows(d)
    idx, fresh, left, _ = _removed_and_fresh(faiss, d, metric, name)
    oracle = None
    for mode in _modes(d):
        q = xq[:_nq(mode)]
        idx.search_mode = mode
        fresh.search_mode = mode
        D, I = idx.search(q, K)
        if len(left) == 0:
            assert (I == -1).all() and (D == (FLT_MAX if metric == "l2" else -FLT_MAX)).all()
            continue
        assert _last_path(idx) == PATH_OF[mode]
        if oracle is None:
            from oracle.flat_knn import search_exact
            oracle = search_exact(left, xq, K + 1, metric)
        check_knn(D, I, left, q, K, metric, oracle=(oracle[0][:len(q)], oracle[1][:len(q)]))
        f1 = fresh.search(q, K)
        if mode == "exact":
            _same((D, I), f1)
            continue
        st = idx.certificate_stats()
        print(f"[remove d={d} {metric} {name} {mode}] {st}")
        assert st["max_err_over_bound"] <= 1.0
        fst = fresh.certificate_stats()
        assert st["candidate_queries"] == fst["candidate_queries"]
        assert st["exact_reruns"] <= fst["exact_reruns"]
        f2 = fresh.search(q, K)
        if all(a.tobytes() == b.tobytes() for a, b in zip(f1, f2)):
            _same((D, I), f1)
        else:
            print(f"[remove d={d} {metric} {name} {mode}] the fresh index searched twice differs: "
                  f"bytes not compared")
    idx.search_mode = "auto"
    fresh.search_mode = "auto"


# ---- 4: regrowth after compaction ---------------------------------------------------------------
@pytest.mark.parametrize("d", sorted(SHAPES))
def test_add_after_removal_and_second_removal(faiss, d):
    xb, xq, extra = _rows(d)
    mask = pattern("random30", len(xb))
    idx = _index(faiss, d, "l2")
    idx.add(xb)
    _materialise(idx, d, xq)
    idx.remove_ids(faiss.IDSelectorBitmap(bitmap(mask)))
    n1 = idx.ntotal
    idx.add(extra[:37])
    assert idx.ntotal == n1 + 37
    rows = np.concatenate([survivors(xb, mask), extra[:37]])
    # labels continue from the new ntotal: the added rows are their own nearest neighbours
    D, I = idx.search(extra[:4], 1)
    assert I[:, 0].tolist() == list(range(n1, n1 + 4))
    fresh = _index(faiss, d, "l2")
    fresh.add(rows)
    _assert_rows_and_pair_keys_equal(faiss, idx, fresh, xq, "l2")
    # a second removal, across old survivors and added rows
    mask2 = pattern("straddle", len(rows)) | (np.arange(len(rows)) >= len(rows) - 9)
    assert idx.remove_ids(np.nonzero(mask2)[0]) == int(mask2.sum())
    fresh2 = _index(faiss, d, "l2")
    fresh2.add(survivors(rows, mask2))
    _assert_rows_and_pair_keys_equal(faiss, idx, fresh2, xq, "l2")
    for mode in _modes(d):
        idx.search_mode = mode
        fresh2.search_mode = mode
        q = xq[:_nq(mode)]
        D, I = idx.search(q, K)
        check_knn(D, I, survivors(rows, mask2), q, K, "l2")
        if mode == "exact":
            _same((D, I), fresh2.search(q, K))
        else:
            assert idx.certificate_stats()["max_err_over_bound"] <= 1.0


def test_default_chunk(faiss, monkeypatch):
    monkeypatch.delenv("IMGREC_REMOVE_CHUNK")
    d = 80
    xb, xq, _ = _rows(d)
    mask = pattern("random30", len(xb))
    idx = _index(faiss, d, "l2")
    idx.add(xb)
    _materialise(idx, d, xq)
    assert idx.remove_ids(np.nonzero(mask)[0]) == int(mask.sum())
    _, fresh, _, _ = _removed_and_fresh(faiss, d, "l2", "random30")
    _assert_rows_and_pair_keys_equal(faiss, idx, fresh, xq, "l2")
    for mode in ("bf16", "i8"):
        idx.search_mode = mode
        idx.search(xq[:4], K)
        assert idx.certificate_stats()["max_err_over_bound"] <= 1.0


# ---- 5: labels, not rows --------------------------------------------------------------------------
def test_id_offset_shifts_the_removed_labels(faiss):
    d = 48
    xb, xq, _ = _rows(d)
    idx = _index(faiss, d, "l2")
    idx.add(xb)
    idx.set_id_offset(1000)
    assert idx.remove_ids(faiss.IDSelectorRange(0, 10)) == 0          # no label below 1000
    assert idx.remove_ids(faiss.IDSelectorRange(1000, 1010)) == 10
    assert idx.ntotal == len(xb) - 10
    _same([idx.reconstruct_n(0, idx.ntotal)], [xb[10:]])
    D, I = idx.search(xb[10:13], 1)
    assert I[:, 0].tolist() == [1000, 1001, 1002]                    # dense again, from the offset


# ---- 6: the file ------------------------------------------------------------------------------------
def test_written_file_equals_a_fresh_index_file(faiss, tmp_path):
    d = 80
    xb, xq, _ = _rows(d)
    idx, fresh, _, _ = _removed_and_fresh(faiss, d, "l2", "random30")
    faiss.write_index(idx, tmp_path / "removed.faiss")
    faiss.write_index(fresh, tmp_path / "fresh.faiss")
    assert (tmp_path / "removed.faiss").read_bytes() == (tmp_path / "fresh.faiss").read_bytes()
    back = faiss.read_index(tmp_path / "removed.faiss")
    _assert_rows_and_pair_keys_equal(faiss, back, fresh, xq, "l2")
    back.search_mode = fresh.search_mode = "exact"
    _same(back.search(xq, K), fresh.search(xq, K))
    fresh.search_mode = "auto"


# ---- 7: contract edges ------------------------------------------------------------------------------
def _raw(idx, bits, nbits):
    from image_recommender_amd import _lib
    n = C.c_int64(-1)
    bp = None if bits is None else C.c_void_p(bits.ctypes.data)
    _lib.check(_lib.load().knn_remove_ids(idx.handle, bp, nbits, C.byref(n)), "knn_remove_ids")
    return n.value


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_contract_edges(faiss, devices):
    from image_recommender_amd._lib import KnnError
    kw = {} if devices is None else {"devices": devices}
    d = 48
    xb, xq, _ = _rows(d)
    empty = _index(faiss, d, "l2", **kw)
    assert empty.remove_ids(faiss.IDSelectorAll()) == 0 and empty.ntotal == 0
    assert _raw(empty, np.full(4, 255, dtype=np.uint8), 32) == 0
    idx = _index(faiss, d, "l2", **kw)
    idx.add(xb[:300])
    assert _raw(idx, None, 0) == 0 and idx.ntotal == 300              # nbits = 0: nothing, NULL allowed
    with pytest.raises(KnnError, match="bitmap is NULL"):
        _raw(idx, None, 8)
    with pytest.raises(KnnError, match="nbits"):
        _raw(idx, np.zeros(1, dtype=np.uint8), -1)
    # nbits < ntotal: rows at and past nbits are kept whatever the bytes hold
    assert _raw(idx, np.full(38, 255, dtype=np.uint8), 101) == 101
    assert idx.ntotal == 199
    _same([idx.reconstruct_n(0, 199)], [xb[101:300]])
    # bits set past ntotal are ignored
    bits = np.concatenate([bitmap(np.arange(199) % 3 == 0), np.full(40, 255, dtype=np.uint8)])
    assert _raw(idx, bits, 8 * len(bits)) == 67
    _same([idx.reconstruct_n(0, idx.ntotal)], [xb[101:300][np.arange(199) % 3 != 0]])
    # removing everything leaves a usable index
    assert idx.remove_ids(faiss.IDSelectorAll()) == 132 and idx.ntotal == 0
    D, I = idx.search(xq, 3)
    assert (I == -1).all() and (D == FLT_MAX).all()
    idx.add(xb[:5])
    D, I = idx.search(xb[:5], 1)
    assert I[:, 0].tolist() == [0, 1, 2, 3, 4]


# ---- multi-device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("force_remote", [False, True])
def test_three_shards_equal_one_device(faiss, tmp_path, monkeypatch, force_remote):
    if force_remote:
        monkeypatch.setenv("IMGREC_MULTI_FORCE_REMOTE", "1")
    d = 80
    xb, xq, extra = _rows(d)
    adds = [xb[:100], xb[100:107], xb[107:357]]
    n = 357
    mask = np.random.default_rng(77).random(n) < 0.3
    mask[100 + 7 * 1 // 3:100 + 7 * 2 // 3] = True        # shard 1's whole piece of the second add
    one = _index(faiss, d, "l2")
    multi = _index(faiss, d, "l2", devices=[0, 0, 0])
    assert multi.num_shards == 3
    for idx in (one, multi):
        for a in adds:
            idx.add(a)
        idx.search_mode = "exact"
        assert idx.remove_ids(faiss.IDSelectorBitmap(bitmap(mask))) == int(mask.sum())

    def compare(tag):
        assert one.ntotal == multi.ntotal
        m = one.ntotal
        _same(multi.search(xq, K), one.search(xq, K))
        _same(multi.range_search(xq, np.inf), one.range_search(xq, np.inf))
        p = faiss.SearchParameters(sel=faiss.IDSelectorBitmap(bitmap(_random_mask(m, m))))
        _same(multi.search(xq, K, params=p), one.search(xq, K, params=p))
        _same([multi.reconstruct_n(0, m)], [one.reconstruct_n(0, m)])
        faiss.write_index(one, tmp_path / f"one_{tag}.faiss")
        faiss.write_index(multi, tmp_path / f"multi_{tag}.faiss")
        assert (tmp_path / f"one_{tag}.faiss").read_bytes() == (tmp_path / f"multi_{tag}.faiss").read_bytes()

    compare("removed")
    _same([one.reconstruct_n(0, one.ntotal)], [survivors(xb[:n], mask)])
    for idx in (one, multi):
        idx.add(extra[:50])
    compare("regrown")
    D, I = multi.search(extra[:3], 1)
    assert I[:, 0].tolist() == [one.ntotal - 50, one.ntotal - 49, one.ntotal - 48]


# ---- the drop-in CLI ----------------------------------------------------------------------------------
TYPES = ["color", "sift"]


def _edit_db(db):
    """Three images lose a vector, five new images arrive (ids above every indexed id)."""
    rng = np.random.default_rng(99)
    con = sqlite3.connect(db)
    con.execute("DELETE FROM color_vectors WHERE image_id IN (2, 17)")
    con.execute("DELETE FROM sift_vectors WHERE image_id = 30")
    for i in range(5):
        cur = con.execute("INSERT INTO images (path) VALUES (?)", (f"image_data/new/{i:04d}.png",))
        for t, dim in (("color", 48), ("sift", 128)):
            v = rng.standard_normal(dim)
            v = (np.abs(v) if t == "color" else v)
            v = (v / np.linalg.norm(v)).astype(np.float32)
            con.execute(f"INSERT INTO {t}_vectors (image_id, {t}_vector_blob) VALUES (?, ?)",
                        (cur.lastrowid, sqlite3.Binary(pickle.dumps(v, protocol=pickle.HIGHEST_PROTOCOL))))
    con.commit()
    con.close()


def _builder(tmp, db, index_file):
    from image_recommender_amd.main.create_index import FAISSIndexBuilderDB
    return FAISSIndexBuilderDB(db_path=str(db), vector_types=TYPES, batch_size=3, index_file=str(index_file),
                               log_dir=str(tmp / "logs"))


def _offsets(db):
    con = sqlite3.connect(db)
    rows = con.execute("SELECT image_id, offset FROM faiss_index_offsets_color_sift ORDER BY offset").fetchall()
    con.close()
    return rows


def test_sync_index_equals_a_full_rebuild(gpu, faiss, tmp_path, monkeypatch):
    from tests.golden.make_golden import build_db
    from image_recommender_amd.main.search_from_image import ImageRecommender
    monkeypatch.chdir(tmp_path)
    name = "index_hnsw_color_sift.faiss"
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    db_a, db_b = tmp_path / "a" / "images.db", tmp_path / "b" / "images.db"
    build_db(db_a)
    build_db(db_b)
    assert _builder(tmp_path, db_a, tmp_path / "a" / name).build_index() is not None
    before = _offsets(db_a)
    assert len(before) == 37                      # 40 images, 3 without a colour or SIFT vector
    _edit_db(db_a)
    _edit_db(db_b)
    synced = _builder(tmp_path, db_a, tmp_path / "a" / name).sync_index()
    assert synced is not None and synced.ntotal == 37 - 3 + 5
    assert _builder(tmp_path, db_b, tmp_path / "b" / name).build_index() is not None
    assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    assert _offsets(db_a) == _offsets(db_b) and len(_offsets(db_a)) == 39
    assert {i for i, _ in _offsets(db_a)}.isdisjoint({2, 17, 30})
    results = []
    for side, db in (("a", db_a), ("b", db_b)):
        rec = ImageRecommender(images_root=".", db_path=str(db), top_k=5, index_dir=str(tmp_path / side))
        rec._plot_results = lambda *a, **k: None
        results.append([rec.search_similar_images([str(tmp_path / q)], "color,sift")
                        for q in ("image_data/set0/0000.png", "image_data/new/0003.png")])
    assert results[0] == results[1] and all(r and len(r) == 5 for r in results[0])
    # a second sync has nothing to do and leaves the same bytes
    assert _builder(tmp_path, db_a, tmp_path / "a" / name).sync_index() is not None
    assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    # the CLI flag runs the same sync
    from image_recommender_amd.main import create_index
    create_index.main(["--db-path", str(db_a), "--vector-types", "color", "sift", "--output",
                       str(tmp_path / "a" / name), "--sync"])
    assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    # a table that does not describe the file: refused, nothing written
    con = sqlite3.connect(db_a)
    con.execute("UPDATE faiss_index_offsets_color_sift SET offset = offset + 1 WHERE offset = 38")
    con.commit()
    con.close()
    tampered = _offsets(db_a)
    assert _builder(tmp_path, db_a, tmp_path / "a" / name).sync_index() is None
    assert _offsets(db_a) == tampered
    assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    # other vector types than the file was built for: refused as well
    from image_recommender_amd.main.create_index import FAISSIndexBuilderDB
    other = FAISSIndexBuilderDB(db_path=str(db_b), vector_types=["color"], index_file=str(tmp_path / "b" / name),
                                log_dir=str(tmp_path / "logs"))
    assert other.sync_index() is None
