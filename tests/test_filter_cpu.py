"""CPU tests of the filtered search: the C ABI surface and its argument validation, the id
selectors' lowering to faiss's bitmap layout, the oracle-side condition of every case the GPU
tests run (tests/filter_check.py CASES), and the unchanged plain path.  No GPU compute.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from image_recommender_amd import _lib
from image_recommender_amd import faiss_compat as faiss
from tests.filter_check import (CASES, check_filtered, labels_to_ranks, make_case, make_mask,
                                oracle_filtered)

ROOT = Path(__file__).resolve().parents[1]
FILTER_NAMES = ("knn_search_filtered", "knn_search_filtered_device")


def test_filter_abi_is_declared_bound_and_exported():
    text = (ROOT / "include" / "imgrec_knn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in FILTER_NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared in imgrec_knn.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported by the library"
    assert "IDSelectorBitmap" in text and "(bitmap[i >> 3] >> (i & 7)) & 1" in text


def test_filter_argument_validation():
    """The checks that come before the index is touched (no index exists without a GPU: the fake
    handle is never dereferenced)."""
    lib = _lib.load()
    q = np.zeros((1, 4), np.float32)
    D = np.zeros((1, 3), np.float32)
    I = np.zeros((1, 3), np.int64)
    bm = np.zeros(1, np.uint8)
    fake = C.c_void_p(0x1000)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.knn_search_filtered(None, p(q), 1, 3, p(bm), 8, p(D), p(I)) == _lib.KNN_EINVAL
    assert lib.knn_search_filtered(fake, p(q), 1, 0, p(bm), 8, p(D), p(I)) == _lib.KNN_EINVAL
    assert b"k must be" in lib.knn_last_error()
    assert lib.knn_search_filtered(fake, p(q), 1, 3, p(bm), -1, p(D), p(I)) == _lib.KNN_EINVAL
    assert b"nbits" in lib.knn_last_error()
    assert lib.knn_search_filtered(fake, p(q), 1, 3, None, 8, p(D), p(I)) == _lib.KNN_EINVAL
    assert b"bitmap is NULL" in lib.knn_last_error()
    assert lib.knn_search_filtered(fake, p(q), 1, 3, p(bm), 8, None, p(I)) == _lib.KNN_EINVAL
    assert lib.knn_search_filtered(fake, p(q), 1, 3, p(bm), 8, p(D), None) == _lib.KNN_EINVAL
    assert lib.knn_search_filtered_device(fake, p(q), 1, 3, None, 8, p(D), p(I), None) == _lib.KNN_EINVAL
    assert lib.knn_search_filtered_device(fake, p(q), 1, -2, p(bm), 8, p(D), p(I), None) == _lib.KNN_EINVAL
    assert lib.knn_search_filtered_device(fake, p(q), 1, 3, p(bm), 8, None, None, None) == _lib.KNN_EINVAL


# ---- selectors ---------------------------------------------------------------------------------
def _selectors():
    rng = np.random.default_rng(5)
    ids = rng.choice(np.arange(-20, 400), size=90, replace=False)
    bits = rng.integers(0, 256, 23, dtype=np.uint8)          # labels 0 .. 183
    return {
        "range": faiss.IDSelectorRange(17, 131),
        "range_empty": faiss.IDSelectorRange(50, 50),
        "range_negative": faiss.IDSelectorRange(-5, 9),
        "batch": faiss.IDSelectorBatch(ids),
        "array": faiss.IDSelectorArray(ids[::2]),
        "array_n": faiss.IDSelectorArray(10, ids),           # swig's (n, ids) form
        "bitmap": faiss.IDSelectorBitmap(bits),
        "bitmap_n": faiss.IDSelectorBitmap(5, bits),         # (nbytes, bitmap)
        "all": faiss.IDSelectorAll(),
        "not": faiss.IDSelectorNot(faiss.IDSelectorRange(17, 131)),
        "and": faiss.IDSelectorAnd(faiss.IDSelectorRange(0, 100), faiss.IDSelectorBatch(ids)),
        "or": faiss.IDSelectorOr(faiss.IDSelectorRange(0, 20), faiss.IDSelectorBitmap(bits)),
        "xor": faiss.IDSelectorXOr(faiss.IDSelectorRange(10, 90), faiss.IDSelectorRange(60, 200)),
    }


def _brute(sel, n, offset):
    out = np.zeros((n + 7) // 8, dtype=np.uint8)
    for i in range(n):
        if sel.is_member(i + offset):
            out[i >> 3] |= 1 << (i & 7)
    return out


@pytest.mark.parametrize("name", sorted(_selectors()))
@pytest.mark.parametrize("n,offset", [(0, 0), (1, 0), (8, 0), (131, 0), (257, 0), (300, 40),
                                      (64, -10), (77, 10**6), (50, 350)])
def test_to_bitmap_matches_is_member(name, n, offset):
    sel = _selectors()[name]
    got = sel.to_bitmap(n, offset)
    assert got.dtype == np.uint8 and got.shape == ((n + 7) // 8,)
    assert got.tobytes() == _brute(sel, n, offset).tobytes()


def test_bit_order_is_faiss():
    """Label i sits in byte i >> 3 at bit i & 7 (IDSelectorBitmap::is_member)."""
    assert faiss.IDSelectorArray([0]).to_bitmap(16).tolist() == [1, 0]
    assert faiss.IDSelectorArray([7]).to_bitmap(16).tolist() == [128, 0]
    assert faiss.IDSelectorArray([8, 10]).to_bitmap(16).tolist() == [0, 5]
    assert faiss.IDSelectorRange(3, 6).to_bitmap(9).tolist() == [0b00111000, 0]
    b = faiss.IDSelectorBitmap(np.array([0b00000100, 0b10000000], np.uint8))
    assert [i for i in range(-3, 40) if b.is_member(i)] == [2, 15]
    assert b.to_bitmap(16).tolist() == [4, 128]
    assert b.to_bitmap(10, offset=1).tolist() == [2, 0]      # label 2 -> row 1; label 15 outside
    # ids outside [offset, offset + n) are silently not members of the lowered set
    assert faiss.IDSelectorArray([-1, 5, 99]).to_bitmap(8).tolist() == [32]
    assert faiss.IDSelectorArray([1005]).to_bitmap(8, offset=1000).tolist() == [32]


def test_selector_algebra():
    n = 200
    unpack = lambda s: np.unpackbits(s.to_bitmap(n), bitorder="little")[:n].astype(bool)
    a, b = faiss.IDSelectorRange(10, 120), faiss.IDSelectorBatch(np.arange(0, 200, 3))
    ma, mb = unpack(a), unpack(b)
    assert (unpack(faiss.IDSelectorAnd(a, b)) == (ma & mb)).all()
    assert (unpack(faiss.IDSelectorOr(a, b)) == (ma | mb)).all()
    assert (unpack(faiss.IDSelectorXOr(a, b)) == (ma ^ mb)).all()
    assert (unpack(faiss.IDSelectorNot(a)) == ~ma).all()
    assert unpack(faiss.IDSelectorAll()).all()
    # De Morgan, double negation, xor through and / or
    nt = faiss.IDSelectorNot
    assert (unpack(nt(faiss.IDSelectorAnd(a, b))) == unpack(faiss.IDSelectorOr(nt(a), nt(b)))).all()
    assert (unpack(nt(nt(a))) == ma).all()
    assert (unpack(faiss.IDSelectorXOr(a, b)) ==
            unpack(faiss.IDSelectorAnd(faiss.IDSelectorOr(a, b), nt(faiss.IDSelectorAnd(a, b))))).all()
    # the tail bits of the last byte stay clear, also under Not / All
    assert faiss.IDSelectorNot(faiss.IDSelectorRange(0, 0)).to_bitmap(3).tolist() == [7]
    assert faiss.IDSelectorAll().to_bitmap(9).tolist() == [255, 1]


def test_search_parameters_classes():
    s = faiss.IDSelectorAll()
    assert faiss.SearchParameters().sel is None and faiss.SearchParameters(sel=s).sel is s
    ivf = faiss.SearchParametersIVF(sel=s, nprobe=7)
    hnsw = faiss.SearchParametersHNSW(sel=s, efSearch=99)
    assert isinstance(ivf, faiss.SearchParameters) and ivf.sel is s and ivf.nprobe == 7
    assert isinstance(hnsw, faiss.SearchParameters) and hnsw.sel is s and hnsw.efSearch == 99
    assert faiss.SearchParametersIVF().nprobe == 1 and faiss.SearchParametersHNSW().efSearch == 16


# ---- the oracle alone passes the checker (the 0.6 condition of every case) ---------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_passes_check_filtered(name):
    xb, xq, mask, k, metric = make_case(name)
    N, d, nq, _, _, seed, frac, _ = CASES[name]
    assert xb.shape == (N, d) and xq.shape == (nq, d) and mask.shape == (N,) and mask[-1]
    assert (mask == make_mask(N, seed, frac)).all()
    D, I = oracle_filtered(xb, xq, mask, k, metric)
    checked, total = check_filtered(D, I, xb, xq, mask, k, metric)
    print(f"[filter case {name}] {int(mask.sum())} selected, {checked} of {total} ranks label-checked")
    assert total == nq * min(k, int(mask.sum())) and checked >= 0.6 * total


def test_checker_rejects_planted_faults():
    xb, xq, mask, k, metric = make_case("a")
    D, I = oracle_filtered(xb, xq, mask, k, metric)
    bad = I.copy()
    bad[3, 0] = int(np.nonzero(~mask)[0][0])                 # an unselected row
    with pytest.raises(AssertionError):
        check_filtered(D, bad, xb, xq, mask, k, metric)
    bad = I.copy()
    bad[5, :2] = bad[5, 1::-1]                               # two ranks swapped
    with pytest.raises(AssertionError):
        check_filtered(D, bad, xb, xq, mask, k, metric)
    Dbad = D.copy()
    Dbad[7, 4] *= 1.01                                        # a wrong key
    with pytest.raises(AssertionError):
        check_filtered(Dbad, I, xb, xq, mask, k, metric)
    with pytest.raises(AssertionError):
        labels_to_ranks(np.array([[len(mask)]]), mask)


# ---- the plain path is untouched -----------------------------------------------------------------
class _FakeLib:
    def __init__(self, ntotal):
        self.calls = []
        self._ntotal = ntotal

    def knn_ntotal(self, h):
        return self._ntotal

    def knn_search(self, *a):
        self.calls.append(("knn_search", a))
        return 0

    def knn_search_filtered(self, *a):
        self.calls.append(("knn_search_filtered", a))
        return 0

    def knn_range_search(self, *a):
        self.calls.append(("knn_range_search", a))
        return 0

    def knn_set_id_offset(self, h, off):
        return 0


def _fake_index(monkeypatch, ntotal=20, d=4):
    lib = _FakeLib(ntotal)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    idx = faiss.Index.__new__(faiss.Index)
    idx._h, idx.d, idx.metric_type, idx.verbose = None, d, faiss.METRIC_L2, False
    return idx, lib


def test_params_without_sel_takes_the_old_path(monkeypatch):
    idx, lib = _fake_index(monkeypatch)
    x = np.zeros((3, 4), np.float32)
    idx.search(x, 5)
    idx.search(x, 5, params=None)
    idx.search(x, 5, params=faiss.SearchParameters())
    idx.search(x, 5, params=faiss.SearchParametersHNSW(efSearch=64))
    assert [c[0] for c in lib.calls] == ["knn_search"] * 4
    assert all(len(c[1]) == 6 and c[1][2:4] == (3, 5) for c in lib.calls)


def test_params_with_sel_lowers_to_one_bitmap(monkeypatch):
    idx, lib = _fake_index(monkeypatch, ntotal=20)
    x = np.zeros((2, 4), np.float32)
    idx.search(x, 3, params=faiss.SearchParameters(sel=faiss.IDSelectorRange(4, 12)))
    idx.set_id_offset(1000)                                   # selectors speak labels
    idx.search(x, 3, params=faiss.SearchParametersIVF(sel=faiss.IDSelectorRange(1004, 1012)))
    assert [c[0] for c in lib.calls] == ["knn_search_filtered"] * 2
    for _, a in lib.calls:
        assert a[2:4] == (2, 3) and a[5] == 20
        got = (C.c_uint8 * 3).from_address(a[4].value)
        assert bytes(got) == faiss.IDSelectorRange(4, 12).to_bitmap(20).tobytes()


def test_range_search_with_a_selector_is_not_implemented(monkeypatch):
    idx, lib = _fake_index(monkeypatch)
    with pytest.raises(NotImplementedError, match="search"):
        idx.range_search(np.zeros((1, 4), np.float32), 1.0,
                         params=faiss.SearchParameters(sel=faiss.IDSelectorAll()))
    assert lib.calls == []
