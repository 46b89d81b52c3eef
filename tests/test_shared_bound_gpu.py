"""The shared per-query screen bound of the 256 x 256 bf16 candidate kernel (csrc/knn_b16w.hip,
DESIGN.md "Shared screen bound"; IMGREC_B16W_SHARED_BOUND, read at index creation).

With the bound on, a workgroup drops rows that no list of its own would have dropped, and which
rows it drops depends on when the other row splits published their keys.  The returned (D, I) must
not: they are the exact fp32 keys of the certified top k.  Every case therefore checks the answer
against the float64 oracle (tests/knn_check.py) AND bit for bit against an index created with the
bound off.

Geometry: IMGREC_CUS plans the launch for few CUs, so a small corpus gives few row splits of
several 256-row tiles each (the bound acts from a split's second tile on).  8-row group g of the
corpus belongs to row split g % nsplit; knn_plan confirms the tile and the split count each case
assumes, knn_plan_kernel the kernel instance (packed lists or not).
"""
import ctypes as C

import numpy as np
import pytest

from tests.datagen import mixture
from tests.knn_check import check_knn

pytestmark = pytest.mark.gpu

D_, N_ = 128, 40_000


@pytest.fixture(scope="module")
def faiss(gpu):
    from image_recommender_amd import faiss_compat
    return faiss_compat


@pytest.fixture(scope="module")
def data():
    """One mixture corpus and 600 queries for every case (cases that patch rows copy it)."""
    return mixture(N_, D_, centres=50, seed=41), mixture(600, D_, centres=50, seed=42)


def _index(faiss, xb, metric, cus, bound, monkeypatch):
    env = {"IMGREC_CUS": str(cus), "IMGREC_B16W_SHARED_BOUND": "1" if bound else "0"}
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    idx = (faiss.IndexFlatL2(xb.shape[1]) if metric == "l2" else
           faiss.IndexFlatIP(xb.shape[1]) if metric == "ip" else
           faiss.IndexFlat(xb.shape[1], faiss.METRIC_COSINE))      # the knobs are read here
    for k_ in env:
        monkeypatch.delenv(k_)
    idx.add(xb)
    idx.search_mode = "bf16"
    return idx


def _plan(idx, nq, k):
    from image_recommender_amd import _lib
    tr, tq, sp, wg = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().knn_plan(idx.handle, nq, k, C.byref(tr), C.byref(tq), C.byref(sp), C.byref(wg)),
               "knn_plan")
    name = C.create_string_buffer(128)
    _lib.check(_lib.load().knn_plan_kernel(idx.handle, nq, k, name, 128), "knn_plan_kernel")
    return (tr.value, tq.value, sp.value), name.value.decode()


def _on_off(faiss, xb, xq, k, metric, cus, monkeypatch, nsplit, packed=True):
    """Search with the bound on and off: the plan is the one the case assumes, the error stays
    inside the certificate bound, the two answers have the same bits.  Returns (D, I, stats on,
    stats off)."""
    out = []
    for bound in (True, False):
        idx = _index(faiss, xb, metric, cus, bound, monkeypatch)
        plan, kernel = _plan(idx, xq.shape[0], k)
        assert plan == (256, 256, nsplit), plan
        assert kernel.startswith("knn_b16w_tile_kernel") and kernel.endswith("true>" if packed else "false>"), kernel
        D, I = idx.search(xq, k)
        st = idx.certificate_stats()
        assert st["candidate_queries"] == xq.shape[0] and 0.0 <= st["max_err_over_bound"] < 1.0, st
        out.append((D, I, st))
        del idx
    (D1, I1, s1), (D0, I0, s0) = out
    assert np.array_equal(I1, I0), np.argwhere(I1 != I0)[:5]
    assert np.array_equal(D1, D0), float(np.abs(D1 - D0).max())
    return D1, I1, s1, s0


@pytest.mark.parametrize("k", [10, 8])                              # list lengths KM = 10 and 8
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_mixture_packed_instances(faiss, data, monkeypatch, metric, k):
    """16 row splits of ~10 tiles: the bound engages from the second tile.  A benign corpus: no
    query may need the exact re-run, with the bound or without (the off-build gives 0 for these
    seeds, so a re-run with the bound on would be one the bound caused)."""
    xb, xq = data
    xq = xq[:512]
    D, I, s1, s0 = _on_off(faiss, xb, xq, k, metric, 32, monkeypatch, nsplit=16)
    assert s0["exact_reruns"] == 0 and s1["exact_reruns"] == 0, (s1, s0)
    check_knn(D, I, xb, xq, k, metric, min_exact_frac=0.5)


def test_mixture_unpacked_instance(faiss, monkeypatch):
    """170,000 rows in 10 row splits: 2125 8-row groups per split, split-local row indices up to
    17151 need 15 bits, above the packed lists' 14 — the separate key / label lists run (the
    smallest shape that reaches them while nsplit >= KM keeps the bound live)."""
    xb = mixture(170_000, 64, centres=50, seed=43)
    xq = mixture(512, 64, centres=50, seed=44)
    D, I, s1, s0 = _on_off(faiss, xb, xq, 10, "l2", 20, monkeypatch, nsplit=10, packed=False)
    assert s0["exact_reruns"] == 0 and s1["exact_reruns"] == 0, (s1, s0)
    check_knn(D, I, xb, xq, 10, "l2", min_exact_frac=0.5)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ragged_shapes(faiss, data, monkeypatch, metric):
    """600 queries (three query blocks, 168 pad queries in the last, which never publish) and
    39,997 rows (not a multiple of 8 or 256) in 11 splits of 454 or 455 groups: every split ends
    in a partial tile of one live quad row."""
    xb, xq = data
    xb = xb[:39_997]
    D, I, _, _ = _on_off(faiss, xb, xq, 10, metric, 32, monkeypatch, nsplit=11)
    check_knn(D, I, xb, xq, 10, metric, min_exact_frac=0.5)


@pytest.mark.parametrize("n,cus,nsplit", [(N_, 8, 4), (200, 32, 1)])
def test_bound_can_never_engage(faiss, data, monkeypatch, n, cus, nsplit):
    """Fewer row splits than slots (4 < KM), and a corpus of one partial tile: a slot stays empty
    for the whole launch, U = +inf and every list screens alone."""
    xb, xq = data
    xb, xq = xb[:n], xq[:512]
    D, I, _, _ = _on_off(faiss, xb, xq, 10, "l2", cus, monkeypatch, nsplit=nsplit)
    check_knn(D, I, xb, xq, 10, "l2", min_exact_frac=0.5)


def test_all_neighbours_in_one_split(faiss, data, monkeypatch):
    """Query 0's ten nearest rows all sit in row split 3 (8-row groups 3, 19, 35, ...), so only
    slot 3 ever gets a good value for it and U stays at the other splits' best, far away."""
    xb, xq = data
    xb, xq = xb.copy(), xq[:512].copy()
    rng = np.random.default_rng(7)
    rows = np.array([8 * (3 + 16 * (20 * i + 1)) + i % 8 for i in range(10)])
    for i, r in enumerate(rows):                       # squared distances 0.0025 (i + 1)^2
        v = rng.standard_normal(D_)
        xb[r] = xq[0] + np.float32(0.05 * (i + 1)) * (v / np.linalg.norm(v)).astype(np.float32)
    D, I, _, _ = _on_off(faiss, xb, xq, 10, "l2", 32, monkeypatch, nsplit=16)
    np.testing.assert_array_equal(I[0], rows)
    check_knn(D, I, xb, xq, 10, "l2", min_exact_frac=0.5)


def test_crowded_band_and_duplicates(faiss, data, monkeypatch):
    """Query 1: 300 rows at squared distances 0.001, 0.002, ... 0.3 — all inside the bf16 band of
    its 10th key (the bound of a d = 128 row of norm ~13 is ~1) — spread over all 16 splits, so
    the K' = 64 candidates cannot certify and the second chance or the exact re-run must find the
    oracle's rows: none of them may have been screened out.  Query 2: corpus row 30001 (entries
    +-1, so that |q|^2 + |x|^2 - 2 q.x is exactly 0 in fp32) and 16
    copies of it in row split 3 (rows 24 + 128 j): that split's list holds 10 keys equal to the
    answer, no certificate can hold, and the exact re-run returns the 10 smallest labels at
    distance 0 (tests/test_configs_gpu.py's cfg2 construction at small size)."""
    xb, xq = data
    xb, xq = xb.copy(), xq[:512].copy()
    rng = np.random.default_rng(8)
    near = 5 + 131 * np.arange(300)                    # row // 8 % 16 takes every value
    assert len(set((near // 8 % 16).tolist())) == 16
    for j, r in enumerate(near):
        v = rng.standard_normal(D_)
        xb[r] = xq[1] + np.float32(np.sqrt(0.001 * (j + 1))) * (v / np.linalg.norm(v)).astype(np.float32)
    dup = np.array([24 + 128 * j for j in range(16)])
    assert not set(dup.tolist()) & set(near.tolist()) and 30001 not in near
    xb[30001] = rng.choice(np.float32([-1.0, 1.0]), D_)     # +-1 entries: its fp32 self key is exactly 0
    xb[dup] = xb[30001]
    xq[2] = xb[30001]
    D, I, s1, s0 = _on_off(faiss, xb, xq, 10, "l2", 32, monkeypatch, nsplit=16)
    for st in (s1, s0):                                # both queries failed the first certificate
        assert st["second_chance"] + st["exact_reruns"] >= 2 and st["exact_reruns"] >= 1, st
    np.testing.assert_array_equal(I[1], near[:10])
    np.testing.assert_array_equal(I[2], dup[:10])
    assert (D[2] == 0.0).all()
    check_knn(D, I, xb, xq, 10, "l2", min_exact_frac=0.5)


def test_repeat_searches_reset_the_slots(faiss, data, monkeypatch):
    """Two searches on one index, the second a different, smaller batch: it must equal a fresh
    index's answer bit for bit (slots or floors left over from the first search would bound
    other queries' keys)."""
    xb, xq = data
    idx = _index(faiss, xb, "l2", 32, True, monkeypatch)
    idx.search(xq, 10)
    xq2 = np.ascontiguousarray(xq[::-1][:512])
    D2, I2 = idx.search(xq2, 10)
    fresh = _index(faiss, xb, "l2", 32, True, monkeypatch)
    Df, If = fresh.search(xq2, 10)
    assert np.array_equal(I2, If) and np.array_equal(D2, Df)
    check_knn(D2, I2, xb, xq2, 10, "l2", min_exact_frac=0.5)
