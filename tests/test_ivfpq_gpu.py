"""GPU IVF-PQ (csrc/ivfpq.hip + image_recommender_amd/ivfpq.py) against oracle/ivfpq.py.

The reference's default index is IndexIVFPQ(IndexHNSWFlat(d, 32), d, 2048, m, 12), nprobe 1
(/root/reference/main/create_index.py:218-228).  faiss is absent: parity is pinned against the
oracle's restatement given the SAME centroids, codebooks and codes (labels exact outside distance
ties, distances to fp32 accumulation), and the GPU encoder against the oracle's encoder.
"""
import numpy as np
import pytest

from oracle import ivfpq as oivf
from oracle.flat_knn import recall_at_k, search_exact
from tests.datagen import mixture

pytestmark = pytest.mark.gpu


def _check(Dg, Ig, Do, Io, q, cen, cb, lists, codes, ids, nprobe):
    """GPU vs oracle: same distances per rank (fp32 accumulation), same labels except where the
    oracle itself has a distance tie (or near-tie within fp32) at that rank; and every returned
    label is a row of one of the query's probed lists, once per row of the result, with that row's
    own oracle ADC distance (so right distances under wrong rows' labels do not pass)."""
    np.testing.assert_allclose(Dg, Do, rtol=2e-5, atol=2e-5)
    bad = Ig != Io
    if bad.any():
        for i, j in zip(*np.nonzero(bad)):
            # the GPU label must exist with (nearly) the oracle's distance at that rank
            assert Ig[i, j] >= 0
            assert abs(Dg[i, j] - Do[i, j]) <= 2e-5 * max(1.0, abs(Do[i, j]))
        assert bad.mean() < 0.01
    order = np.argsort(ids)
    probes = oivf.nearest(q, cen, nprobe)
    m = cb.shape[0]
    for i in range(Ig.shape[0]):
        lab = Ig[i][Ig[i] >= 0]
        assert np.unique(lab).size == lab.size, f"query {i}: a label is returned twice"
        assert (Ig[i][lab.size:] == -1).all(), f"query {i}: a result after the padding"
        pos = np.minimum(np.searchsorted(ids, lab, sorter=order), ids.size - 1)
        rows = order[pos]
        assert (ids[rows] == lab).all(), f"query {i}: a label that was never stored"
        assert np.isin(lists[rows], probes[i]).all(), f"query {i}: a label from a list that was not probed"
        for l in np.unique(lists[rows]):
            sel = lists[rows] == l
            T = oivf.tables((q[i].astype(np.float64) - cen[l].astype(np.float64))[None], cb)[0]
            want = T[np.arange(m)[None, :], codes[rows[sel]]].sum(1)
            got = Dg[i, :lab.size][sel]
            assert (np.abs(got - want) <= 2e-5 * np.maximum(1.0, np.abs(want))).all(), \
                f"query {i}, list {l}: a distance that is not its label's"


def _random_index(idx_cls, rng, d, nlist, m, nbits, n, nonneg_ids=True):
    ksub = 1 << nbits
    cen = rng.standard_normal((nlist, d)).astype(np.float32)
    cb = (0.3 * rng.standard_normal((m, ksub, d // m))).astype(np.float32)
    lists = rng.integers(0, nlist, n)
    codes = rng.integers(0, ksub, (n, m))
    ids = rng.permutation(10 * n)[:n].astype(np.int64)
    idx = idx_cls(d, nlist, m, nbits)
    idx.set_trained(cen, cb)
    idx.add_encoded(lists, codes, ids)
    return idx, cen, cb, lists, codes, ids


@pytest.mark.parametrize("d,nlist,m,nbits,n,nq,k,nprobe", [
    (32, 16, 8, 8, 5000, 40, 10, 1),
    (64, 32, 16, 6, 8000, 33, 16, 4),
    (48, 8, 4, 12, 3000, 17, 32, 2),
    (1968, 8, 48, 12, 4000, 12, 10, 1),          # the reference's sub-quantiser shape
    # any k (faiss's range): every probed row keyed and sorted per query (ivfpq_scan_all_device)
    (32, 16, 8, 8, 5000, 40, 100, 1),
    (64, 32, 16, 6, 8000, 33, 700, 4),
    (1968, 8, 48, 12, 4000, 5, 2000, 2),
])
def test_scan_matches_oracle_on_the_same_codes(gpu, d, nlist, m, nbits, n, nq, k, nprobe):
    from image_recommender_amd.ivfpq import IndexIVFPQ
    rng = np.random.default_rng(d + n)
    idx, cen, cb, lists, codes, ids = _random_index(IndexIVFPQ, rng, d, nlist, m, nbits, n)
    idx.nprobe = nprobe
    q = (cen[rng.integers(0, nlist, nq)] + 0.5 * rng.standard_normal((nq, d))).astype(np.float32)
    Dg, Ig = idx.search(q, k)
    Do, Io = oivf.search(q, cen, cb, lists, codes, ids, k, nprobe)
    _check(Dg, Ig, Do, Io, q, cen, cb, lists, codes, ids, nprobe)


def test_duplicate_codes_tie_by_label_and_short_lists_pad(gpu):
    from image_recommender_amd.ivfpq import IndexIVFPQ
    rng = np.random.default_rng(9)
    d, nlist, m, nbits = 16, 4, 4, 4
    idx = IndexIVFPQ(d, nlist, m, nbits)
    cen = rng.standard_normal((nlist, d)).astype(np.float32)
    cb = rng.standard_normal((m, 16, 4)).astype(np.float32)
    idx.set_trained(cen, cb)
    # list 0 holds six rows with one code (exact distance ties), list 1 two rows, lists 2-3 empty
    lists = np.array([0] * 6 + [1, 1])
    codes = np.array([[1, 2, 3, 4]] * 6 + [[0, 0, 0, 0], [5, 5, 5, 5]])
    ids = np.array([50, 7, 31, 2, 99, 12, 1, 3])
    idx.add_encoded(lists, codes, ids)
    idx.nprobe = 1
    D, I = idx.search(cen[:1] + 0.01, 8)
    assert I[0, :6].tolist() == [2, 7, 12, 31, 50, 99]
    assert (I[0, 6:] == -1).all() and (D[0, 6:] == np.finfo(np.float32).max).all()
    assert len(set(D[0, :6].tolist())) == 1
    idx.nprobe = 4
    D, I = idx.search(cen[:1] + 0.01, 10)
    assert sorted(I[0, :8].tolist()) == sorted(ids.tolist()) and (I[0, 8:] == -1).all()
    # the same through the any-k route (k > 32): identical ranks, longer padding
    D2, I2 = idx.search(cen[:1] + 0.01, 40)
    np.testing.assert_array_equal(I2[0, :10], I[0])
    np.testing.assert_array_equal(D2[0, :8], D[0, :8])
    assert (I2[0, 8:] == -1).all() and (D2[0, 8:] == np.finfo(np.float32).max).all()
    idx.nprobe = 1
    D3, I3 = idx.search(cen[:1] + 0.01, 33)
    assert I3[0, :6].tolist() == [2, 7, 12, 31, 50, 99] and (I3[0, 6:] == -1).all()


def test_train_add_search_end_to_end(gpu):
    """Trained on clustered data: the GPU encoder agrees with the oracle encoder given the trained
    parameters, the search agrees with the oracle, and recall against the exact search is in the
    range IVF-PQ reaches (well above chance, below 1)."""
    from image_recommender_amd.ivfpq import IndexIVFPQ
    d, nlist, m, nbits, n = 64, 32, 16, 8, 12000
    xb = mixture(n, d, centres=60, seed=21)
    xq = mixture(64, d, centres=60, seed=22)
    idx = IndexIVFPQ(d, nlist, m, nbits, niter=8, pq_niter=8)
    assert not idx.is_trained
    idx.train(xb)
    assert idx.is_trained and idx.ntotal == 0
    idx.add(xb)
    assert idx.ntotal == n
    cen, cb = idx.centroids.cpu().numpy(), idx.codebooks.cpu().numpy()
    lists_o, codes_o = oivf.encode(xb, cen, cb)
    lists_g, codes_g, ids_g = idx.list_contents()
    order = np.argsort(ids_g)
    assert (lists_g[order] == lists_o).mean() > 0.999
    assert (codes_g[order] == codes_o).mean() > 0.999
    for nprobe, lo in [(1, 0.2), (8, 0.4)]:
        idx.nprobe = nprobe
        D, I = idx.search(xq, 10)
        Do, Io = oivf.search(xq, cen, cb, lists_g, codes_g, ids_g, 10, nprobe)
        _check(D, I, Do, Io, xq, cen, cb, lists_g, codes_g, ids_g, nprobe)
        _, Ie = search_exact(xb, xq, 10, "l2")
        r = recall_at_k(I, Ie, 10)
        assert lo < r < 1.0, (nprobe, r)


def test_rejects_bad_shapes(gpu):
    from image_recommender_amd.ivfpq import IndexIVFPQ
    with pytest.raises(ValueError):
        IndexIVFPQ(30, 4, 7)
    idx = IndexIVFPQ(16, 4, 4, 4)
    with pytest.raises(RuntimeError):
        idx.add(np.zeros((3, 16), np.float32))
    idx.set_trained(np.zeros((4, 16), np.float32), np.zeros((4, 16, 4), np.float32))
    with pytest.raises(ValueError):
        idx.add_encoded([0], [[0, 0, 0, 16]], [0])
    with pytest.raises(ValueError):
        idx.search(np.zeros((1, 16), np.float32), 0)


def test_write_read_roundtrip(gpu, tmp_path):
    from image_recommender_amd.ivfpq import IndexIVFPQ
    rng = np.random.default_rng(12)
    idx, cen, cb, lists, codes, ids = _random_index(IndexIVFPQ, rng, 32, 8, 4, 10, 2000)
    idx.nprobe = 3
    q = rng.standard_normal((9, 32)).astype(np.float32)
    D0, I0 = idx.search(q, 7)
    f = tmp_path / "ivfpq.npz"
    idx.write(f)
    back = IndexIVFPQ.read(f)
    assert back.ntotal == idx.ntotal and back.nprobe == 3 and back.nbits == 10
    D1, I1 = back.search(q, 7)
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1, D0)


def _case_index(name):
    """An index holding a case of tests/ivfpq_check.py (tests/test_ivfpq_check_cpu.py counts its
    near-ties against _check's allowance)."""
    from image_recommender_amd.ivfpq import IndexIVFPQ
    from tests import ivfpq_check as ic
    cs = ic.PY_CASE[name]
    cen, cb, lists, codes, ids, q = (np.array(a) for a in ic.py_case_data(name))   # (writable copies)
    idx = IndexIVFPQ(cs.d, cs.nlist, cs.m, cs.nbits)
    idx.set_trained(cen, cb)
    idx.add_encoded(lists, codes, ids)
    idx.nprobe = cs.nprobe
    return cs, idx, (cen, cb, lists, codes, ids, q)


def _against_oracle(idx, data, k, nprobe):
    cen, cb, lists, codes, ids, q = data
    Dg, Ig = idx.search(q, k)
    Do, Io = oivf.search(q, cen, cb, lists, codes, ids, k, nprobe)
    _check(Dg, Ig, Do, Io, q, cen, cb, lists, codes, ids, nprobe)
    return Dg, Ig


def test_sixteen_bit_codes_pass_through_the_int16_tensor(gpu):
    """nbits = 16: codes >= 32768 are negative in the int16 tensor that stores them; the kernels read
    the same bytes as uint16."""
    cs, idx, data = _case_index("nbits16")
    lists, codes, ids = data[2:5]
    assert codes.min() == 0 and codes.max() == 65535 and (codes >= 32768).mean() > 0.4
    gl, gc, gi = idx.list_contents()
    order = np.argsort(lists, kind="stable")
    np.testing.assert_array_equal(gl, lists[order])
    np.testing.assert_array_equal(gc, codes[order])
    np.testing.assert_array_equal(gi, ids[order])
    for k in cs.ks:
        _against_oracle(idx, data, k, cs.nprobe)


def test_every_list_probed_and_nprobe_clamped(gpu):
    """nprobe = nlist = 40: the coarse top-40 is beyond the exact search's register top-k (k <= 32)
    and takes its large-k route; with every list probed the result is the ADC order of all rows.
    nprobe beyond nlist is clamped to it: the same bytes."""
    cs, idx, data = _case_index("probe_all")
    assert cs.nprobe == cs.nlist == 40
    for k in cs.ks:
        D, I = _against_oracle(idx, data, k, cs.nlist)
        idx.nprobe = 1000
        D2, I2 = idx.search(data[5], k)
        idx.nprobe = cs.nprobe
        np.testing.assert_array_equal(I2, I)
        assert D2.tobytes() == D.tobytes()


def test_table_chunks_give_the_single_chunk_bytes(gpu):
    """table_bytes bounds the distance tables of one chunk of queries (default 1 GiB: 1365 queries at
    the reference's shape).  Set to five queries' tables, 23 queries go in chunks of 5, 5, 5, 5 and
    3; both scan routes return the bytes of the single chunk."""
    cs, idx, data = _case_index("chunks")
    assert idx.table_bytes == 1 << 30
    per_query = cs.nprobe * cs.m * (1 << cs.nbits) * 4
    for k in cs.ks:
        D, I = _against_oracle(idx, data, k, cs.nprobe)
        idx.table_bytes = 5 * per_query + per_query // 2
        D2, I2 = idx.search(data[5], k)
        idx.table_bytes = 1 << 30
        np.testing.assert_array_equal(I2, I)
        assert D2.tobytes() == D.tobytes()


def test_labels_are_held_to_the_range_both_routes_keep(gpu):
    """A negative label would be an empty slot to the register scan (k <= 32) and label 2^32 + id
    to the sort route (k > 32): add_encoded refuses it, as it refuses 2^31.  The ends of the range,
    0 and 2^31 - 1, come back from both routes at the same ranks."""
    from image_recommender_amd.ivfpq import IndexIVFPQ
    rng = np.random.default_rng(16)
    d, nlist, m, nbits, n = 16, 4, 4, 4, 26
    idx, cen, cb, lists, codes, ids = _random_index(IndexIVFPQ, rng, d, nlist, m, nbits, n)
    assert 0 not in ids and ids.max() < 7000          # the labels added below are new
    for bad in (-1, -2 ** 31, 2 ** 31):
        with pytest.raises(ValueError):
            idx.add_encoded([0, 1], [[0] * m, [1] * m], [5000, bad])
    assert idx.ntotal == n
    # the extreme labels share a list and a code, so they tie and rank by label
    idx.add_encoded([0, 0, 1, 1], np.stack([codes[0]] * 4), [2 ** 31 - 1, 0, 7000, 7001])
    idx.nprobe = nlist
    q = (cen + 0.1 * rng.standard_normal((nlist, d))).astype(np.float32)
    D32, I32 = idx.search(q, 32)          # all 30 rows and two ranks of padding
    D33, I33 = idx.search(q, 33)
    np.testing.assert_array_equal(I33[:, :32], I32)
    assert D33[:, :32].tobytes() == D32.tobytes()
    assert (np.sort(I32[:, :30], axis=1) == np.sort(np.concatenate([ids, [0, 2 ** 31 - 1, 7000, 7001]]))).all()
    assert (I32[:, 30:] == -1).all() and (I33[:, 30:] == -1).all()
    for i in range(nlist):
        r0, r1 = (int(np.nonzero(I32[i] == lab)[0][0]) for lab in (0, 2 ** 31 - 1))
        assert r0 < r1 and D32[i, r0] == D32[i, r1]
    # and in a true top-k (fewer ranks than rows): the same prefix from both routes
    D5, I5 = idx.search(q, 5)
    np.testing.assert_array_equal(I5, I33[:, :5])
    assert D5.tobytes() == np.ascontiguousarray(D33[:, :5]).tobytes()
