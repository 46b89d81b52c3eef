"""HIP tests of the filtered search (faiss SearchParameters.sel on the MI355X kernels): parity with
float64 at the shapes where the gathered tile kernel can go wrong, bitwise agreement with
range_search (the same contraction), the bitwise invariances the fixed arithmetic promises, the
seam between the register-list route and the sort route, the edge cases of the contract
(include/imgrec_knn.h) and the recommender's two options.

Every result checked by tests/filter_check.check_filtered belongs to a table case whose 0.6
label-checked condition tests/test_filter_cpu.py proves on the CPU.
"""
import ctypes as C
import json
import sqlite3
from pathlib import Path

import numpy as np
import pytest

from tests.filter_check import CASES, check_filtered, make_case

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
GOLDEN = json.loads((Path(__file__).parent / "golden" / "plumbing.json").read_text())


@pytest.fixture(scope="module")
def faiss(gpu):
    from image_recommender_amd import faiss_compat
    return faiss_compat


def _index(faiss, d, metric, **kw):
    if metric == "l2":
        return faiss.IndexFlatL2(d, **kw)
    if metric == "ip":
        return faiss.IndexFlatIP(d, **kw)
    return faiss.IndexFlat(d, faiss.METRIC_COSINE, **kw)


def _bitmap(mask):
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little")


def _params(faiss, mask):
    return faiss.SearchParameters(sel=faiss.IDSelectorBitmap(_bitmap(mask)))


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert x.tobytes() == y.tobytes()


_built = {}


def _case(faiss, name):
    """(index, (D, I)) of a table case through the public surface, computed once per module."""
    if name not in _built:
        xb, xq, mask, k, metric = make_case(name)
        idx = _index(faiss, xb.shape[1], metric)
        idx.add(xb)
        _built[name] = (idx, idx.search(xq, k, params=_params(faiss, mask)))
    return _built[name]


def _prefix_of_range(idx, xq, k, metric):
    """The first k of every range_search(all rows) segment, padded as a search pads."""
    lims, D, I = idx.range_search(xq, np.inf if metric == "l2" else -np.inf)
    nq = xq.shape[0]
    Dk = np.full((nq, k), FLT_MAX if metric == "l2" else -FLT_MAX, dtype=np.float32)
    Ik = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        n = min(k, int(lims[q + 1] - lims[q]))
        Dk[q, :n] = D[lims[q]:lims[q] + n]
        Ik[q, :n] = I[lims[q]:lims[q] + n]
    return Dk, Ik


def _expect_from_sub(faiss, xb, xq, mask, k, metric):
    """What the filtered search must return, bit for bit: the k-prefix of range_search(all rows) on
    an index built from xb[mask], labels mapped back to rows of xb."""
    sel = np.nonzero(mask)[0]
    if len(sel) == 0:
        nq = xq.shape[0]
        return (np.full((nq, k), FLT_MAX if metric == "l2" else -FLT_MAX, dtype=np.float32),
                np.full((nq, k), -1, dtype=np.int64))
    sub = _index(faiss, xb.shape[1], metric)
    sub.add(np.ascontiguousarray(xb[mask]))
    Dk, Ik = _prefix_of_range(sub, xq, k, metric)
    return Dk, np.where(Ik >= 0, sel[np.maximum(Ik, 0)], -1).astype(np.int64)


def _raw(idx, xq, k, bitmap, nbits):
    """knn_search_filtered itself (its own nbits and bitmap pointer)."""
    from image_recommender_amd import _lib
    n = xq.shape[0]
    D = np.empty((n, k), dtype=np.float32)
    I = np.empty((n, k), dtype=np.int64)
    bp = None if bitmap is None else C.c_void_p(bitmap.ctypes.data)
    _lib.check(_lib.load().knn_search_filtered(idx.handle, C.c_void_p(xq.ctypes.data), n, k, bp, nbits,
                                               C.c_void_p(D.ctypes.data), C.c_void_p(I.ctypes.data)),
               "knn_search_filtered")
    return D, I


# ---- parity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_float64(faiss, name):
    xb, xq, mask, k, metric = make_case(name)
    idx, (D, I) = _case(faiss, name)
    assert D.shape == (xq.shape[0], k) and D.dtype == np.float32 and I.dtype == np.int64
    checked, total = check_filtered(D, I, xb, xq, mask, k, metric)
    print(f"[filter {name}] {checked} of {total} ranks label-checked")
    from image_recommender_amd import _lib
    assert _lib.load().knn_last_path(idx.handle) == 0


# ---- bitwise against what exists ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "f", "d"])
def test_full_mask_equals_range_prefix(faiss, name):
    xb, xq, _, k, metric = make_case(name)
    idx, _ = _case(faiss, name)
    got = idx.search(xq, k, params=_params(faiss, np.ones(len(xb), dtype=bool)))
    _same(got, _prefix_of_range(idx, xq, k, metric))
    _same(got, idx.search(xq, k, params=faiss.SearchParameters(sel=faiss.IDSelectorAll())))


@pytest.mark.parametrize("name", ["a", "f", "d"])
def test_masked_equals_sub_index_range_prefix(faiss, name):
    xb, xq, mask, k, metric = make_case(name)
    _, got = _case(faiss, name)
    _same(got, _expect_from_sub(faiss, xb, xq, mask, k, metric))


# ---- invariances, all bitwise ----------------------------------------------------------------------
def test_second_call_is_identical(faiss):
    xb, xq, mask, k, _ = make_case("a")
    idx, first = _case(faiss, "a")
    _same(first, idx.search(xq, k, params=_params(faiss, mask)))


def test_query_by_query_equals_batch(faiss):
    xb, xq, mask, k, _ = make_case("a")
    idx, (D, I) = _case(faiss, "a")
    p = _params(faiss, mask)
    for q in range(xq.shape[0]):
        _same(idx.search(xq[q:q + 1], k, params=p), (D[q:q + 1], I[q:q + 1]))


def test_two_adds_equal_one(faiss):
    xb, xq, mask, k, metric = make_case("a")
    _, want = _case(faiss, "a")
    idx = _index(faiss, xb.shape[1], metric)
    idx.add(xb[:301])
    idx.add(xb[301:])
    _same(idx.search(xq, k, params=_params(faiss, mask)), want)


@pytest.mark.parametrize("name", ["a", "d"])
def test_three_shards_equal_one_device(faiss, name):
    xb, xq, mask, k, metric = make_case(name)
    _, want = _case(faiss, name)
    idx = _index(faiss, xb.shape[1], metric, devices=[0, 0, 0])
    assert idx.num_shards == 3
    idx.add(xb[:301])
    idx.add(xb[301:])
    _same(idx.search(xq, k, params=_params(faiss, mask)), want)


def test_sort_route_on_shards_equals_one_device(faiss):
    xb, xq, mask, k, metric = make_case("g")
    _, want = _case(faiss, "g")
    idx = _index(faiss, xb.shape[1], metric, devices=[0, 0])
    idx.add(xb)
    _same(idx.search(xq, k, params=_params(faiss, mask)), want)


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_device_form_equals_host_form(faiss, devices):
    import torch
    xb, xq, mask, k, metric = make_case("a")
    _, want = _case(faiss, "a")
    idx = _index(faiss, xb.shape[1], metric, **({} if devices is None else {"devices": devices}))
    idx.add(xb)
    q = torch.from_numpy(xq.copy()).cuda()
    bm = torch.from_numpy(_bitmap(mask)).cuda()
    D = torch.empty((xq.shape[0], k), dtype=torch.float32, device="cuda")
    I = torch.empty((xq.shape[0], k), dtype=torch.int64, device="cuda")
    idx.search_filtered_device(q.data_ptr(), xq.shape[0], k, bm.data_ptr(), len(xb), D.data_ptr(),
                               I.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same((D.cpu().numpy(), I.cpu().numpy()), want)


def test_id_offset_shifts_labels_and_selectors(faiss):
    xb, xq, mask, k, metric = make_case("a")
    _, (D0, I0) = _case(faiss, "a")
    off = 10 ** 6
    idx = _index(faiss, xb.shape[1], metric)
    idx.add(xb)
    idx.set_id_offset(off)
    labels = np.nonzero(mask)[0] + off
    D, I = idx.search(xq, k, params=faiss.SearchParameters(sel=faiss.IDSelectorBatch(labels)))
    _same((D, I), (D0, I0 + off))
    # a selector of the unshifted labels selects nothing now
    D, I = idx.search(xq, k, params=faiss.SearchParameters(sel=faiss.IDSelectorBatch(labels - off)))
    assert (I == -1).all() and (D == FLT_MAX).all()


def test_every_selector_class_equals_its_bitmap(faiss):
    xb, xq, _, k, _ = make_case("a")
    idx, _ = _case(faiss, "a")
    N = len(xb)
    rng = np.random.default_rng(9)
    ids = np.sort(rng.choice(N, 300, replace=False))
    rngsel = faiss.IDSelectorRange(100, 700)
    sels = [rngsel, faiss.IDSelectorBatch(ids), faiss.IDSelectorArray(ids),
            faiss.IDSelectorBitmap(_bitmap(rng.random(N) < 0.3)), faiss.IDSelectorAll(),
            faiss.IDSelectorNot(rngsel), faiss.IDSelectorAnd(rngsel, faiss.IDSelectorBatch(ids)),
            faiss.IDSelectorOr(rngsel, faiss.IDSelectorBatch(ids)),
            faiss.IDSelectorXOr(rngsel, faiss.IDSelectorBatch(ids))]
    for s in sels:
        member = np.array([s.is_member(i) for i in range(N)])
        got = idx.search(xq, k, params=faiss.SearchParameters(sel=s))
        _same(got, idx.search(xq, k, params=_params(faiss, member)))
        assert member[got[1][got[1] >= 0]].all()
    # the IVF / HNSW parameter classes carry the selector the same way
    want = idx.search(xq, k, params=faiss.SearchParameters(sel=rngsel))
    _same(idx.search(xq, k, params=faiss.SearchParametersIVF(sel=rngsel, nprobe=4)), want)
    _same(idx.search(xq, k, params=faiss.SearchParametersHNSW(sel=rngsel, efSearch=64)), want)
    with pytest.raises(NotImplementedError):
        idx.range_search(xq, 1.0, params=faiss.SearchParameters(sel=rngsel))


# ---- route seam ------------------------------------------------------------------------------------
def test_sort_route_agrees_with_list_route(faiss):
    xb, xq, mask, _, _ = make_case("g")
    idx, _ = _case(faiss, "g")
    p = _params(faiss, mask)
    D33, I33 = idx.search(xq, 33, params=p)
    D32, I32 = idx.search(xq, 32, params=p)
    _same((np.ascontiguousarray(D33[:, :32]), np.ascontiguousarray(I33[:, :32])), (D32, I32))


# ---- edges ---------------------------------------------------------------------------------------
def _edge_mask(N, rows):
    m = np.zeros(N, dtype=bool)
    m[rows] = True
    return m


@pytest.mark.parametrize("nsel", [256, 512, 1, 7, 0])
def test_selected_counts_at_tile_edges(faiss, nsel):
    """Whole tiles exactly, one row, fewer than k (padded tail), none."""
    xb, xq, _, k, metric = make_case("a")
    idx, _ = _case(faiss, "a")
    rows = np.sort(np.random.default_rng(nsel + 1).choice(len(xb), nsel, replace=False))
    mask = _edge_mask(len(xb), rows)
    D, I = idx.search(xq, k, params=_params(faiss, mask))
    _same((D, I), _expect_from_sub(faiss, xb, xq, mask, k, metric))
    n = min(nsel, k)
    assert (I[:, :n] >= 0).all() and (I[:, n:] == -1).all() and (D[:, n:] == FLT_MAX).all()
    # one query (the 256 x 32 geometry) and the sort route see the same edge
    _same(idx.search(xq[:1], k, params=_params(faiss, mask)), (D[:1], I[:1]))
    D40, I40 = idx.search(xq[:3], 40, params=_params(faiss, mask))
    _same((np.ascontiguousarray(D40[:, :k]), np.ascontiguousarray(I40[:, :k])), (D[:3], I[:3]))
    assert (I40[:, min(nsel, 40):] == -1).all()


def test_zero_selected_inner_product(faiss):
    xb, xq, _, k, metric = make_case("f")
    idx, _ = _case(faiss, "f")
    D, I = idx.search(xq, k, params=_params(faiss, np.zeros(len(xb), dtype=bool)))
    assert (I == -1).all() and (D == -FLT_MAX).all()
    D, I = idx.search(xq, 40, params=_params(faiss, np.zeros(len(xb), dtype=bool)))
    assert (I == -1).all() and (D == -FLT_MAX).all()


def test_nbits_below_and_above_ntotal(faiss):
    xb, xq, mask, k, metric = make_case("a")
    idx, (D0, I0) = _case(faiss, "a")
    N = len(xb)
    # nbits < ntotal: rows at or past nbits are never returned, whatever the bytes hold
    nbits = 611
    bm = _bitmap(np.ones(N, dtype=bool))
    D, I = _raw(idx, xq, k, bm, nbits)
    assert I.max() < nbits
    _same((D, I), _expect_from_sub(faiss, xb, xq, _edge_mask(N, np.arange(nbits)), k, metric))
    # nbits > ntotal: the bits past ntotal are ignored
    big = np.concatenate([_bitmap(mask), np.full(40, 255, dtype=np.uint8)])
    _same(_raw(idx, xq, k, big, 8 * len(big)), (D0, I0))
    # nbits = 0: nothing selected (the bitmap may be NULL)
    D, I = _raw(idx, xq, k, None, 0)
    assert (I == -1).all() and (D == FLT_MAX).all()


def test_empty_index_and_no_queries(faiss):
    idx = faiss.IndexFlatL2(24)
    xq = np.zeros((3, 24), dtype=np.float32)
    p = faiss.SearchParameters(sel=faiss.IDSelectorAll())
    for k in (4, 50):
        D, I = idx.search(xq, k, params=p)
        assert D.shape == (3, k) and (I == -1).all() and (D == FLT_MAX).all()
    full, _ = _case(faiss, "a")
    D, I = full.search(np.zeros((0, 96), dtype=np.float32), 5, params=p)
    assert D.shape == (0, 5) and I.shape == (0, 5)
    multi = faiss.IndexFlatL2(24, devices=[0, 0])
    D, I = multi.search(xq, 4, params=p)
    assert (I == -1).all() and (D == FLT_MAX).all()


def test_range_selector_skips_whole_corpus_tiles(faiss):
    xb, xq, _, k, metric = make_case("c")
    idx, _ = _case(faiss, "c")
    sel = faiss.IDSelectorRange(2300, 3100)            # corpus tiles 0-16 and 25-39 hold nothing
    D, I = idx.search(xq, k, params=faiss.SearchParameters(sel=sel))
    assert ((I >= 2300) & (I < 3100)).all()
    _same((D, I), _expect_from_sub(faiss, xb, xq, _edge_mask(len(xb), np.arange(2300, 3100)), k, metric))


def test_exact_ties_return_the_smallest_selected_labels(faiss):
    xb, xq, _, _, metric = make_case("a")
    xb = xb.copy()
    rows = np.sort(np.random.default_rng(3).choice(len(xb), 40, replace=False))
    xb[rows] = xq[0]                                    # 40 copies: key 0 for query 0, exact ties
    idx = _index(faiss, xb.shape[1], metric)
    idx.add(xb)
    mask = np.ones(len(xb), dtype=bool)
    mask[rows[::2]] = False                             # half of the copies masked out
    want = rows[1::2][:5]
    for q in (xq[:1], xq):                              # both geometries
        D, I = idx.search(q, 5, params=_params(faiss, mask))
        assert I[0].tolist() == want.tolist() and (D[0] == D[0, 0]).all()
    D, I = idx.search(xq[:1], 40, params=_params(faiss, mask))     # the sort route
    assert I[0, :20].tolist() == rows[1::2].tolist()


def test_errors(faiss):
    from image_recommender_amd._lib import KnnError
    xb, xq, mask, k, _ = make_case("a")
    idx, _ = _case(faiss, "a")
    with pytest.raises(KnnError, match="k must be"):
        _raw(idx, xq, 0, _bitmap(mask), len(xb))
    with pytest.raises(KnnError, match="bitmap is NULL"):
        _raw(idx, xq, k, None, len(xb))
    with pytest.raises(KnnError, match="nbits"):
        _raw(idx, xq, k, _bitmap(mask), -1)


# ---- the recommender's options ---------------------------------------------------------------------
@pytest.fixture()
def color_db(gpu, tmp_path, monkeypatch):
    from tests.golden.make_golden import build_db
    from image_recommender_amd.main.create_index import FAISSIndexBuilderDB
    monkeypatch.chdir(tmp_path)
    build_db(tmp_path / "images.db")
    FAISSIndexBuilderDB(db_path="images.db", vector_types=["color"], batch_size=7,
                        log_dir=str(tmp_path / "logs")).build_index()
    return tmp_path


def _recommender(tmp, **kw):
    from image_recommender_amd.main.search_from_image import ImageRecommender
    rec = ImageRecommender(images_root=".", db_path=str(tmp / "images.db"), top_k=5, **kw)
    rec._plot_results = lambda *a, **k: None
    return rec


def _brute_force(rec, tmp, query_rel, allowed):
    """(path, float64 squared distance) of the 6 nearest stored vectors among the offsets `allowed`
    keeps, from the index's own rows; the gaps between them must dwarf fp32 rounding."""
    index, _, order, id_map = rec._indexes["color"]
    q = rec._extract_query_vector(query_rel, order).astype(np.float64)[0]
    x = index.reconstruct_n(0, index.ntotal).astype(np.float64)
    d = ((x - q) ** 2).sum(1)
    con = sqlite3.connect(tmp / "images.db")
    path = {i: p for i, p in con.execute("SELECT id, path FROM images")}
    con.close()
    offs = [o for o in np.argsort(d, kind="stable") if allowed(path[int(id_map[o])])][:6]
    assert (np.diff(d[offs]) > 1e-5).all()
    return [(path[int(id_map[o])], d[o]) for o in offs]


def _assert_results(res, want, tmp):
    got = [(str(Path(p).relative_to(tmp)), d) for p, d in res]
    assert [p for p, _ in got] == [p for p, _ in want[:len(got)]]
    # 32 unit roundoffs of the key's term scale (|q|^2 + |x|^2 = 2: unit-norm query and rows)
    np.testing.assert_allclose([d for _, d in got], [d for _, d in want[:len(got)]], atol=32 * 2.0 ** -24 * 2)


def test_recommender_exclude_query_and_restrict_to(color_db):
    tmp = color_db
    queries = ["image_data/set0/0000.png", "image_data/set1/0004.png"]
    plain = _recommender(tmp)
    for qp in queries:
        base = plain.search_similar_images([str(tmp / qp)], "color")
        _assert_results(base, _brute_force(plain, tmp, [qp], lambda p: True), tmp)
        assert str(Path(base[0][0]).relative_to(tmp)) == qp           # the query itself comes first

        rec = _recommender(tmp, exclude_query=True)
        res = rec.search_similar_images([str(tmp / qp)], "color")
        assert len(res) == 5 and qp not in [str(Path(p).relative_to(tmp)) for p, _ in res]
        _assert_results(res, _brute_force(rec, tmp, [qp], lambda p: p != qp), tmp)

        rec = _recommender(tmp, restrict_to="image_data/set1/")
        res = rec.search_similar_images([str(tmp / qp)], "color")
        assert len(res) == 5
        assert all(str(Path(p).relative_to(tmp)).startswith("image_data/set1/") for p, _ in res)
        _assert_results(res, _brute_force(rec, tmp, [qp], lambda p: p.startswith("image_data/set1/")), tmp)
        assert rec.search_similar_images([str(tmp / qp)], "color") == res    # the prefix mask is kept

        rec = _recommender(tmp, exclude_query=True, restrict_to="image_data/set1/")
        res = rec.search_similar_images([str(tmp / qp)], "color")
        ok = lambda p: p.startswith("image_data/set1/") and p != qp
        assert all(ok(str(Path(p).relative_to(tmp))) for p, _ in res)
        _assert_results(res, _brute_force(rec, tmp, [qp], ok), tmp)


def test_recommender_default_is_unchanged(color_db):
    """With neither option the plain search runs (no selector is built) and the plumbing
    fixture's colour results come back as before."""
    tmp = color_db
    rec = _recommender(tmp)
    assert rec._selector("color", np.arange(4), ["x"]) is None
    for s in GOLDEN["searches"]:
        if s["index_type"] != "color" or s["error"] or s["results"] is None:
            continue
        res = rec.search_similar_images([str(tmp / p) for p in s["paths"]], "color")
        got = [(str(Path(p).relative_to(tmp)), d) for p, d in res]
        assert [p for p, _ in got] == [p for p, _ in s["results"]]
        # (32 unit roundoffs of the key's term scale |q|^2 + |x|^2 = 2, as the drop-in test allows)
        np.testing.assert_allclose([d for _, d in got], [d for _, d in s["results"]], atol=32 * 2.0 ** -24 * 2)


def test_cli_flags(color_db, capsys):
    from image_recommender_amd.main import search_from_image as sfi
    tmp = color_db
    q = "image_data/set1/0004.png"
    rc = sfi.main(["--db-path", str(tmp / "images.db"), "--images-root", ".", "--query", str(tmp / q),
                   "--index", "color", "--top-k", "4", "--no-plot", "--exclude-query", "--within",
                   "image_data/set1/"])
    lines = [l.split("\t")[1] for l in capsys.readouterr().out.strip().splitlines()]
    assert rc == 0 and len(lines) == 4
    assert all("image_data/set1/" in l and not l.endswith("0004.png") for l in lines)
