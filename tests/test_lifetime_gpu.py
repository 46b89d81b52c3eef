"""Lifetimes and regrowth of the index's device buffers (csrc/dev_buf.h, the corpus column table).

Every buffer an index keeps is an owning member, and the per-row corpus arrays grow, shrink and
are filled through one table.  These tests reach every lazily created buffer with small shapes and
pin what must not change when ownership does: results.

  * regrowth with all eight columns live (d = 256: split + bf16 + int8 copies) and with a row
    stride that is no multiple of 32 and a partial last int8 block (d = 200), against an index that
    received the same rows in one add; then a removal and one more add on both;
  * every workspace route twice on one index, the index freed, three times in one process: the
    repeats and the cycles must agree byte for byte;
  * a two-shard index on one device (remote path forced) against the single index;
  * two k-means trainings on two streams sharing the per-device workspace.

No memory-usage assertion: device-wide free memory is not this process's to read.  The leak
guarantees come from the structure (destructors) and tests/test_dev_buf_cpu.py.
"""
import gc

import numpy as np
import pytest

from tests.datagen import mixture

pytestmark = pytest.mark.gpu

K = 10


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


def _same(a, b, what=""):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert x.tobytes() == y.tobytes(), what


def _modes(d):
    return (["split"] if d >= 256 else []) + ["bf16", "i8", "exact"]


def _search_all(idx, d, xq):
    """(D, I) per mode; the int8 path takes batches of at most 8 queries."""
    out = {}
    for mode in _modes(d):
        idx.search_mode = mode
        out[mode] = idx.search(xq[:4] if mode == "i8" else xq, K)
    return out


# ---- regrowth with every column live ----------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
@pytest.mark.parametrize("d", [256, 200])
def test_regrowth_with_every_column_live(faiss, d, metric):
    x = mixture(650 + 8, d, centres=12, seed=7 + d)
    xb, extra, xq = x[:600], x[600:650], np.ascontiguousarray(x[650:])
    grown, whole = _index(faiss, d, metric), _index(faiss, d, metric)
    grown.add(xb[:300])
    _search_all(grown, d, xq)                   # materialises the split and int8 copies
    grown.add(xb[300:])                         # 600 rows > the 512-row capacity: every column moves
    whole.add(xb)

    def compare(tag):
        assert grown.ntotal == whole.ntotal
        a, b = _search_all(grown, d, xq), _search_all(whole, d, xq)
        for mode in a:
            _same(a[mode], b[mode], f"{tag} {mode}")
        _same([grown.reconstruct_n(0, grown.ntotal)], [whole.reconstruct_n(0, whole.ntotal)], tag)

    compare("regrown")
    ids = np.arange(0, 600, 3)
    for idx in (grown, whole):
        assert idx.remove_ids(ids) == 200
    compare("removed")
    if metric != "cosine":                      # (cosine stores its rows normalised)
        _same([grown.reconstruct_n(0, 400)], [xb[np.arange(600) % 3 != 0]])
    for idx in (grown, whole):
        idx.add(extra)
    compare("added")


# ---- workspace routes, index lifetimes ----------------------------------------------------------------
def _bitmap(mask):
    return np.packbits(mask, bitorder="little")


def _routes(faiss, xb, xq, xbig):
    """Every workspace route of one index, each run twice (the repeat must agree), then the index is
    dropped.  Returns the first runs' results as bytes, keyed by route."""
    n, d = xb.shape
    idx = faiss.IndexFlatL2(d)
    idx.add(xb)
    got = {}

    def twice(name, fn):
        a, b = fn(), fn()
        _same(a, b, name)
        got[name] = [np.asarray(v).tobytes() for v in a]

    for k in (10, 100, 1100):                   # lists, large-k stripes, huge-k sort
        twice(f"k{k}", lambda k=k: idx.search(xq, k))
    # the radius of the 20th neighbour of query 0: some rows for every query's cluster, and more than
    # the 64-entry append buffer holds, so the overflow re-run happens
    r_some = float(idx.search(xq[:1], 20)[0][0, -1]) * 1.5
    lims, _, _ = idx.range_search(xq, r_some)
    assert lims[-1] > 64
    twice("range_some", lambda: idx.range_search(xq, r_some))
    twice("range_none", lambda: idx.range_search(xq, 1e-6))
    assert idx.range_search(xq, 1e-6)[0][-1] == 0
    sel = faiss.SearchParameters(sel=faiss.IDSelectorBitmap(_bitmap(np.arange(n) % 3 == 1)))
    for k in (10, 40):                          # lists, and the sort past KNN_MAX_K
        twice(f"filtered_k{k}", lambda k=k: idx.search(xq, k, params=sel))
    twice("pinned", lambda: idx.search(xq, K))                  # 5 x 64 floats: page-locked staging
    twice("unpinned", lambda: idx.search(xbig, K))              # 300,032 floats: past the 1 MiB limit
    # remove_ids changes the index, so its two runs are two removals, each against numpy
    keep = np.arange(n)
    for rnd in range(2):
        mask = np.arange(keep.size) % 5 == rnd
        assert idx.remove_ids(faiss.IDSelectorBitmap(_bitmap(mask))) == int(mask.sum())
        keep = keep[~mask]
        rows = idx.reconstruct_n(0, idx.ntotal)
        _same([rows], [xb[keep]], f"remove {rnd}")
        got[f"remove{rnd}"] = [rows.tobytes()] + [v.tobytes() for v in idx.search(xq, K)]
    del idx
    gc.collect()
    return got


def test_workspace_routes_over_three_index_lifetimes(faiss, monkeypatch):
    monkeypatch.setenv("IMGREC_RANGE_CAP", "64")            # read when an index is created
    monkeypatch.setenv("IMGREC_REMOVE_CHUNK", "64")
    d = 64
    x = mixture(2000 + 5, d, centres=10, seed=5)
    xb, xq = np.ascontiguousarray(x[:2000]), np.ascontiguousarray(x[2000:])
    xbig = mixture(4688, d, centres=10, seed=6)             # 4688 x 64 = 300,032 floats
    assert xbig.size >= 300_000 and xbig.nbytes > 1 << 20
    first = _routes(faiss, xb, xq, xbig)
    for cycle in (2, 3):
        again = _routes(faiss, xb, xq, xbig)
        assert again.keys() == first.keys()
        for name in first:
            assert again[name] == first[name], f"cycle {cycle}: {name}"


# ---- multi-device --------------------------------------------------------------------------------------
def test_two_forced_remote_shards_equal_one_index(faiss, monkeypatch):
    import torch
    monkeypatch.setenv("IMGREC_MULTI_FORCE_REMOTE", "1")    # read when the index is created
    d = 64
    x = mixture(900 + 5, d, centres=10, seed=9)
    xb, xq = np.ascontiguousarray(x[:900]), np.ascontiguousarray(x[900:])
    one = faiss.IndexFlatL2(d)
    multi = faiss.IndexFlatL2(d, devices=[0, 0])
    assert multi.num_shards == 2
    t = torch.from_numpy(xb[500:]).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for idx in (one, multi):
        idx.search_mode = "exact"
        idx.add(xb[:500])
        idx.add_device(t.data_ptr(), t.shape[0], st)
    torch.cuda.synchronize()
    sel = faiss.SearchParameters(sel=faiss.IDSelectorBitmap(_bitmap(np.arange(900) % 4 != 0)))

    def compare(tag):
        assert one.ntotal == multi.ntotal
        _same(multi.search(xq, K), one.search(xq, K), tag)
        _same(multi.search(xq, K, params=sel), one.search(xq, K, params=sel), tag)
        _same([multi.reconstruct_n(0, multi.ntotal)], [one.reconstruct_n(0, one.ntotal)], tag)

    compare("added")
    mask = np.arange(900) % 3 == 0
    for idx in (one, multi):
        assert idx.remove_ids(faiss.IDSelectorBitmap(_bitmap(mask))) == 300
    compare("removed")
    _same([multi.reconstruct_n(0, 600)], [xb[~mask]])
    del multi, one
    gc.collect()


# ---- k-means ---------------------------------------------------------------------------------------------
def test_kmeans_twice_on_two_streams(faiss):
    import torch
    n, d, k = 1000, 32, 8
    x = mixture(n, d, centres=k, seed=11)
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        km = faiss.Kmeans(d, k, niter=3, seed=1234)
        obj = km.train_device(xd.data_ptr(), n, s.cuda_stream)
        runs.append((km.centroids.copy(), km.obj.copy(), obj))
    _same(runs[0][:2], runs[1][:2])
    assert runs[0][2] == runs[1][2]
