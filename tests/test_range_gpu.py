"""HIP tests of range_search (faiss Index::range_search on the MI355X kernels): parity with float64
at the shapes where the tile kernel can go wrong, the edge cases of the contract, the overflow
re-run, and the bitwise invariances the fixed arithmetic promises (include/imgrec_knn.h).

Every result checked by tests/range_check.check_range is preceded by the two oracle-side
conditions (band <= 2 % of expected, expected >= 5 nq; tests/test_range_cpu.py proves them for the
whole table on the CPU).
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle.flat_knn import fp32_error_bound
from tests.range_check import (CASES, assert_conditions, check_range, exact_keys, make_case,
                               range_conditions)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
L2_CASES = [n for n in sorted(CASES) if CASES[n][3] == "l2" and CASES[n][6] is not None]
IP_CASES = [n for n in sorted(CASES) if CASES[n][3] != "l2"]


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


def _run_case(faiss, name):
    xb, xq, radius, metric, d64, b = make_case(name)
    band, expected = range_conditions(xb, xq, radius, metric, d64, b)
    assert_conditions(band, expected, xq.shape[0])
    idx = _index(faiss, xb.shape[1], metric)
    idx.add(xb)
    lims, D, I = idx.range_search(xq, radius)
    check_range(lims, D, I, xb, xq, radius, metric, d64, b)
    # the result is the oracle's up to the band
    assert abs(int(lims[-1]) - expected) <= band, (int(lims[-1]), expected, band)
    return idx, (lims, D, I)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", L2_CASES)
def test_parity_l2(faiss, name):
    _run_case(faiss, name)


@pytest.mark.parametrize("name", IP_CASES)
def test_parity_ip_and_cosine(faiss, name):
    _, (lims, D, I) = _run_case(faiss, name)
    for q in range(len(lims) - 1):
        assert (np.diff(D[lims[q]:lims[q + 1]]) <= 0).all()      # inner products descending


def test_one_row_index(faiss):
    """N = 1, d = 64, nq = 3.  Three pairs cannot hold 5 hits per query, so this case is checked
    directly instead of through check_range: the radius is the midpoint of the two largest
    float64 distances (a gap thousands of error bounds wide), so exactly the two nearer queries
    return row 0, at distances within the fp32 bound."""
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((1, 64)).astype(np.float32)
    xq = (xb + np.array([[0.1], [0.5], [1.0]]) * rng.standard_normal((3, 64))).astype(np.float32)
    d64 = exact_keys(xb, xq, "l2")[:, 0]
    b = fp32_error_bound(xb, xq, "l2")[:, 0]
    order = np.argsort(d64)
    radius = float(np.float32((d64[order[1]] + d64[order[2]]) / 2))
    assert d64[order[2]] - radius > 100 * b.max() and radius - d64[order[1]] > 100 * b.max()
    idx = faiss.IndexFlatL2(64)
    idx.add(xb)
    lims, D, I = idx.range_search(xq, radius)
    want = (d64 < radius).astype(np.int64)
    assert lims.tolist() == [0] + np.cumsum(want).tolist()
    assert (I == 0).all() and len(I) == 2
    assert (np.abs(D - d64[want > 0]) <= b[want > 0]).all()


def test_everything_and_nothing(faiss):
    name = "l2_700x96_q5_all"
    xb, xq, radius, metric, d64, b = make_case(name)
    N, nq = xb.shape[0], xq.shape[0]
    idx, (lims, D, I) = _run_case(faiss, name)                     # radius = +inf
    assert lims.tolist() == [N * i for i in range(nq + 1)]
    for q in range(nq):
        assert sorted(I[lims[q]:lims[q + 1]].tolist()) == list(range(N))
    # a k-prefix is a top-k: the label set search(exact) returns, wherever rank 10 is separated
    idx.search_mode = "exact"
    Ds, Is = idx.search(xq, 10)
    checked = 0
    for q in range(nq):
        o = np.argsort(d64[q], kind="stable")
        if d64[q, o[10]] - d64[q, o[9]] > 2 * max(b[q, o[9]], b[q, o[10]]):
            assert set(I[lims[q]:lims[q] + 10].tolist()) == set(Is[q].tolist()) == set(o[:10].tolist())
            checked += 1
    assert checked >= 1
    # the IP counterpart of "everything"
    ip = faiss.IndexFlatIP(xb.shape[1])
    ip.add(xb)
    l2, D2, I2 = ip.range_search(xq, -np.inf)
    assert l2.tolist() == lims.tolist() and (np.diff(D2[:N]) <= 0).all()
    # nothing: radius 0 (and below), no queries, an empty index
    for r in (0.0, -1.0):
        l0, D0, I0 = idx.range_search(xq, r)
        assert l0.tolist() == [0] * (nq + 1) and len(D0) == 0 and len(I0) == 0
    l0, D0, I0 = idx.range_search(np.zeros((0, xb.shape[1]), np.float32), 10.0)
    assert l0.tolist() == [0] and l0.dtype == np.int64 and D0.dtype == np.float32 and I0.dtype == np.int64
    empty = faiss.IndexFlatL2(xb.shape[1])
    l0, D0, I0 = empty.range_search(xq, np.inf)
    assert l0.tolist() == [0] * (nq + 1) and len(D0) == 0 and len(I0) == 0
    with pytest.raises(faiss.KnnError, match="NaN"):
        idx.range_search(xq, float("nan"))
    with pytest.raises(ValueError):
        idx.range_search(xq[:, :5], 1.0)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
from image_recommender_amd import faiss_compat as faiss
from tests.range_check import make_case
xb, xq, radius, metric, d64, b = make_case("l2_1000x96_q33")
idx = faiss.IndexFlatL2(xb.shape[1])
idx.add(xb)
lims, D, I = idx.range_search(xq, radius)
lims2, D2, I2 = idx.range_search(xq, radius)        # the grown buffer: no re-run this time
assert lims.tobytes() == lims2.tobytes() and D.tobytes() == D2.tobytes() and I.tobytes() == I2.tobytes()
np.savez({out!r}, lims=lims, D=D, I=I)
"""


def test_overflow_rerun_is_bit_identical(faiss, tmp_path):
    """IMGREC_RANGE_CAP=64 (read at index creation; a fresh child keeps it out of this process):
    the case's >= 165 hits overflow the append buffer, the chunk runs again into a buffer of the
    counted size, and the result equals the default-capacity one bit for bit."""
    _, ref = _run_case(faiss, "l2_1000x96_q33")
    assert ref[0][-1] > 64
    out = tmp_path / "child.npz"
    env = dict(os.environ, IMGREC_RANGE_CAP="64")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=str(ROOT), out=str(out))], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "IMGREC_RANGE_CAP=64" in r.stderr           # the knob was read
    got = np.load(out)
    _same(ref, (got["lims"], got["D"], got["I"]))


def test_invariance_batch_split_and_repeat(faiss):
    idx, ref = _run_case(faiss, "l2_5000x100_q70")
    xb, xq, radius = make_case("l2_5000x100_q70")[:3]
    _same(ref, idx.range_search(xq, radius))                      # a second identical call
    parts = [idx.range_search(xq[i:i + 1], radius) for i in range(xq.shape[0])]
    lims = np.concatenate([[0], np.cumsum([p[0][1] for p in parts])]).astype(np.int64)
    _same(ref, (lims, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])))


@pytest.mark.parametrize("name", ["l2_1000x96_q33", "cosine_3000x768_q40"])
def test_invariance_adds_and_shards(faiss, name):
    idx, ref = _run_case(faiss, name)
    xb, xq, radius, metric = make_case(name)[:4]
    d = xb.shape[1]
    two = _index(faiss, d, metric)
    two.add(xb[:301])
    two.add(xb[301:])
    _same(ref, two.range_search(xq, radius))
    multi = _index(faiss, d, metric, devices=[0, 0, 0])
    assert multi.num_shards == 3
    multi.add(xb[:301])
    multi.add(xb[301:])
    _same(ref, multi.range_search(xq, radius))
    _same(ref, multi.range_search(xq, radius))


def test_id_offset_shifts_every_label(faiss):
    idx, (lims, D, I) = _run_case(faiss, "l2_1000x96_q33")
    xb, xq, radius = make_case("l2_1000x96_q33")[:3]
    idx.set_id_offset(10 ** 6)
    _same((lims, D, I + 10 ** 6), idx.range_search(xq, radius))


class _DeviceArray:
    """A raw device pointer as a __cuda_array_interface__ object (torch.as_tensor reads it)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False),
                                         "version": 2}


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_device_form(faiss, devices):
    import torch
    idx, ref = _run_case(faiss, "l2_1000x96_q33")
    xb, xq, radius, metric = make_case("l2_1000x96_q33")[:4]
    if devices is not None:
        idx = _index(faiss, xb.shape[1], metric, devices=devices)
        idx.add(xb)
    q = torch.from_numpy(xq.copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    res = idx.range_search_device(q.data_ptr(), q.shape[0], radius, stream)
    assert res.nq == xq.shape[0] and res.size == ref[0][-1]
    _same(ref, res.to_host())
    pl, pd, pi = res.device_ptrs()
    assert pl and pd and pi
    tl = torch.as_tensor(_DeviceArray(pl, res.nq + 1, "<i8"), device="cuda")
    td = torch.as_tensor(_DeviceArray(pd, res.size, "<f4"), device="cuda")
    ti = torch.as_tensor(_DeviceArray(pi, res.size, "<i8"), device="cuda")
    _same(ref, (tl.cpu().numpy(), td.cpu().numpy(), ti.cpu().numpy()))
    del tl, td, ti, res


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("nq", [5, 130])
@pytest.mark.parametrize("d", [48, 80])
def test_exact_topk_equals_range_prefix(faiss, d, nq, metric):
    """The top-k, range and filter kernels run one tile core (csrc/knn_tile.h): one depth order,
    one key formula.  Where the row stride is no multiple of 32 (d = 48, 80) every exact geometry
    and the range kernel use 16-deep stages, so the search_mode="exact" top-k is the k-prefix of
    range_search(all rows) byte for byte, D and I, padded as a search pads.  N = 3000: several tiles
    per geometry, the last one partial; nq = 5 / 130: the 256 x 32 and the 128 x 128 geometry."""
    from tests.test_filter_gpu import _prefix_of_range
    rng = np.random.default_rng(1000 * d + nq)
    xb = rng.standard_normal((3000, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    idx = _index(faiss, d, metric)
    idx.add(xb)
    idx.search_mode = "exact"
    _same(idx.search(xq, 10), _prefix_of_range(idx, xq, 10, metric))
