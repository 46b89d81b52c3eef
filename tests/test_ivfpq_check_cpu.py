"""CPU proof that the IVF-PQ checks of tests/ivfpq_check.py can fail.  An emulation of the table
kernel's arithmetic stays within lut_bound at every tested shape, with margin, and three planted
mistakes leave it; expected_scan reproduces a case worked by hand, and each of four planted mistakes
changes its bytes on the inputs the GPU tests use, so equality with it cannot come about by accident;
the cases of tests/test_ivfpq_gpu.py leave _check's label allowance unused.  No GPU compute.
"""
import numpy as np
import pytest

from oracle import ivfpq as oivf
from tests import ivfpq_check as ic


# ---- distance tables --------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ic.LUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulated_table_is_within_the_bound_with_margin(shape):
    """The emulation fuses the multiply-add, so by lut_bound's derivation it has dsub + 2 rounding
    factors where the bound allows dsub + 3: it must stay under (dsub + 2) / (dsub + 3) of the bound.
    At long sub-vectors roundings average out and correct arithmetic uses well under half of it.  At
    dsub = 2 over 655,360 entries the worst case is nearly met (an entry dominated by its first term,
    its four roundings aligned: 0.755 of the bound where the most possible is 0.8): the bound is
    tight, not wrong."""
    resid, cbt = ic.lut_inputs(*shape)
    dsub = shape[2]
    r = ic.lut_ratio(ic.emulate_lut(resid, cbt), resid, cbt)
    print(f"[ivfpq_lut] emulation {shape}: worst error / bound {r:.3f}")
    assert r <= (dsub + 2) / (dsub + 3), (shape, r)
    if dsub >= 16:
        assert r <= 0.5, (shape, r)


def test_emulated_table_is_exact_on_integers():
    for shape in [(9, 3, 5, 257), (3, 2, 256, 64)]:
        resid, cbt = ic.lut_inputs_int(*shape)
        T, _ = ic.lut_bound(resid, cbt)
        lut = ic.emulate_lut(resid, cbt)
        assert T.max() < 2 ** 24 and (T == np.rint(T)).all()
        np.testing.assert_array_equal(lut.astype(np.float64), T)


# (1, 1, 1, 1) has no neighbouring row or centroid; the reference's shape repeats (7, 3, 5, 255) at 7 s
FAULT_SHAPES = [s for s in ic.LUT_SHAPES if s not in ((1, 1, 1, 1), (17, 48, 41, 4096))]


@pytest.mark.parametrize("shape", FAULT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_planted_table_mistakes_break_the_bound(shape):
    resid, cbt = ic.lut_inputs(*shape)
    dsub = shape[2]
    dropped = ic.emulate_lut(resid, cbt, skip_t=dsub - 1)                  # one t term dropped
    assert ic.lut_ratio(dropped, resid, cbt) > 1.0
    shifted = cbt.copy()                                                   # one codebook column (j = 0,
    shifted[0, dsub // 2] = np.roll(cbt[0, dsub // 2], 1)                  # one t) read at centroid i - 1
    assert ic.lut_ratio(ic.emulate_lut(resid, shifted), resid, cbt) > 1.0
    neighbour = resid.copy()                                               # row 0 computed from row 1
    neighbour[0] = resid[1]
    assert ic.lut_ratio(ic.emulate_lut(neighbour, cbt), resid, cbt) > 1.0
    # and on the integer probe the same mistakes are unequal tables
    ri, ci = ic.lut_inputs_int(*shape)
    T, _ = ic.lut_bound(ri, ci)
    assert (ic.emulate_lut(ri, ci, skip_t=0).astype(np.float64) != T).any()


def test_lut_ratio_rejects_unwritten_and_misshapen_tables():
    resid, cbt = ic.lut_inputs(7, 3, 5, 255)
    lut = ic.emulate_lut(resid, cbt)
    hole = lut.copy()
    hole[6, 2, 254] = np.nan
    assert ic.lut_ratio(hole, resid, cbt) == float("inf")
    assert ic.lut_ratio(lut[:6], resid, cbt) == float("inf")


# ---- the scan ---------------------------------------------------------------------------------

def test_expected_scan_on_a_case_worked_by_hand():
    """Two lists (rows 0-2 and 3-4), m = 2, ksub = 2, two queries of two probes.
    Query 0 probes list 1 with table row 0 and list 0 with table row 1:
      row 3 (codes 0, 1): 0.5 + 2 = 2.5      row 4 (1, 1): 1.5 + 2 = 3.5
      row 0 (0, 0): 1 + 1.5 = 2.5            row 1 (1, 0): 3 + 1.5 = 4.5     row 2 (0, 1): 1 + 0.25 = 1.25
    -> (1.25, label 9), then the 2.5 tie by label: 4 (row 3) before 7 (row 0), (3.5, 30), (4.5, 8).
    Query 1 has a -1 probe and list 0 with table row 3: rows 0-2 = 0 + 8 = 8, 4 + 8 = 12, 0 + 16 = 16."""
    lut = np.array([[[0.5, 1.5], [9.0, 2.0]],
                    [[1.0, 3.0], [1.5, 0.25]],
                    [[7.0, 7.0], [7.0, 7.0]],
                    [[0.0, 4.0], [8.0, 16.0]]], np.float32)
    probes = np.array([[1, 0], [-1, 0]])
    list_off = np.array([0, 3, 5])
    codes = np.array([[0, 0], [1, 0], [0, 1], [0, 1], [1, 1]])
    ids = np.array([7, 8, 9, 4, 30])
    D, I = ic.expected_scan(lut, probes, list_off, codes, ids, 6)
    assert D.dtype == np.float32 and I.dtype == np.int64
    F = ic.FLT_MAX
    assert I.tolist() == [[9, 4, 7, 30, 8, -1], [7, 8, 9, -1, -1, -1]]
    assert D.tolist() == [[1.25, 2.5, 2.5, 3.5, 4.5, F], [8.0, 12.0, 16.0, F, F, F]]
    D2, I2 = ic.expected_scan(lut, probes, list_off, codes, ids, 2)
    assert I2.tolist() == [[9, 4], [7, 8]] and D2.tolist() == [[1.25, 2.5], [8.0, 12.0]]
    # every probe -1
    D3, I3 = ic.expected_scan(lut, np.full((2, 2), -1), list_off, codes, ids, 3)
    assert (I3 == -1).all() and (D3 == F).all()


def test_expected_scan_adds_in_float32_in_j_order():
    """1 + 2^-24 + 2^-24: left to right in fp32 each half-ulp addend is rounded away (ties to even)
    and the sum is 1; from the right the two halves first make one ulp."""
    lut = np.array([[[1.0], [2.0 ** -24], [2.0 ** -24]]], np.float32)
    args = (np.array([[0]]), np.array([0, 1]), np.zeros((1, 3), np.int64), np.array([5]), 1)
    assert ic.expected_scan(lut, *args)[0][0, 0] == np.float32(1.0)
    assert ic.expected_scan(lut[:, ::-1], *args)[0][0, 0] == np.float32(1.0) + np.float32(2.0 ** -23)


def _bytes(DI):
    return DI[0].tobytes() + DI[1].tobytes()


def _scan(c, k, **over):
    a = dict(c, **over)
    return ic.expected_scan(a["lut"], a["probes"], a["list_off"], a["codes"], a["ids"], k)


def _without_last_rows(c):
    """The geometry with the last row of every list taken out."""
    off = c["list_off"]
    sizes = np.diff(off)
    keep = np.ones(off[-1], bool)
    keep[off[1:][sizes > 0] - 1] = False
    new_off = np.concatenate([[0], np.cumsum(np.maximum(sizes - 1, 0))])
    return dict(list_off=new_off, codes=c["codes"][keep], ids=c["ids"][keep])


@pytest.mark.parametrize("k", [1, 16, 32, 100])
def test_planted_scan_mistakes_change_the_expected_bytes(k):
    ties, rnd = ic.scan_case("ties"), ic.scan_case("random")
    want = _bytes(_scan(ties, k))
    # ties broken by the larger label: the same scan on mirrored labels, mirrored back
    hi = ic.LABEL_END - 1
    D, I = _scan(ties, k, ids=hi - ties["ids"])
    assert _bytes((D, np.where(I >= 0, hi - I, I))) != want
    # the last row of each list skipped (a loop bound one short)
    assert _bytes(_scan(ties, k, **_without_last_rows(ties))) != want
    # ids read one row further
    assert _bytes(_scan(ties, k, ids=np.roll(ties["ids"], -1))) != want
    # summed over j descending: integer tables add exactly in any order, so this one is shown on the
    # random table, where it moves distance bits
    Dr, Ir = _scan(rnd, k)
    Dd, Id = _scan(rnd, k, lut=rnd["lut"][:, ::-1], codes=rnd["codes"][:, ::-1])
    assert Dd.tobytes() != Dr.tobytes()
    assert _bytes(_scan(ties, k, lut=ties["lut"][:, ::-1], codes=ties["codes"][:, ::-1])) == want


def test_scan_case_has_the_stated_edges():
    for table in ("random", "ties"):
        c = ic.scan_case(table)
        ids, probes, sizes = c["ids"], c["probes"], np.diff(c["list_off"])
        assert sizes.tolist() == list(ic.SCAN_LIST_SIZES) and c["lut"].shape == (36, 8, 64)
        assert np.unique(ids).size == ids.size and ids.min() == 0 and ids.max() == 2 ** 31 - 1
        assert (np.diff(ids) < 0).any() and (np.diff(ids) > 0).any()
        assert (probes[7] == -1).all() and (sizes[probes[8][probes[8] >= 0]] == 0).all()
        assert any((p == -1).any() and (p >= 0).any() for p in probes)
        for p in probes:
            live = p[p >= 0]
            assert np.unique(live).size == live.size
        assert (c["lut"] >= 0).all() and np.isfinite(c["lut"]).all()
        cnt = ic.probe_slots(probes, c["list_off"])[0].reshape(probes.shape).sum(1)
        assert cnt.max() == 1768          # query 0: 1000 + 256 + 257 + 255, below k = 5000
    # hundreds of rows of a query share a distance
    c = ic.scan_case("ties")
    D, _ = _scan(c, 5000)
    vals, n = np.unique(D[0][D[0] < ic.FLT_MAX], return_counts=True)
    assert vals.size <= 17 and n.max() >= 200


def test_expected_scan_of_65539_queries_is_quick():
    import time
    c = ic.scan_case_slices()
    t0 = time.perf_counter()
    D, I = _scan(c, 33)
    dt = time.perf_counter() - t0
    print(f"[ivfpq_scan] expected_scan, nq = 65539: {dt:.2f} s")
    assert D.shape == (65539, 33) and dt < 5.0
    # spot rows against the plain per-query loop
    for q in (0, 1, 2, 65534, 65535, 65538):
        l = int(c["probes"][q, 0])
        rows = np.arange(c["list_off"][l], c["list_off"][l + 1])
        dist = c["lut"][q, 0, c["codes"][rows, 0].astype(np.int64)]
        order = np.lexsort((c["ids"][rows], dist))[:33]
        assert I[q, :order.size].tolist() == c["ids"][rows][order].tolist() and (I[q, order.size:] == -1).all()
        assert D[q, :order.size].tobytes() == dist[order].tobytes()


# ---- the Python-level cases ---------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in ic.PY_CASES])
def test_python_cases_leave_the_label_allowance_unused(name):
    """_check lets under 1 % of the labels differ where distances are within its window.  Ranks of
    the float64 oracle that close to a neighbour are the only ones fp32 may permute; each case keeps
    their share under that 1 %, so a wrong label elsewhere cannot pass as a tie."""
    cs = ic.PY_CASE[name]
    cen, cb, lists, codes, ids, q = ic.py_case_data(name)
    for k in cs.ks:
        D, _ = oivf.search(q, cen, cb, lists, codes, ids, k + 1, min(cs.nprobe, cs.nlist))
        share = ic.near_tie_share(D)
        print(f"[ivfpq] case {name}, k = {k}: {share:.2%} of the ranks within the window of a neighbour")
        assert share < ic.MAX_SHARE, (name, k, share)


def test_near_tie_share_counts_both_neighbours():
    F = float(ic.FLT_MAX)
    D = np.array([[1.0, 1.00001, 2.0, 3.0, 3.0], [5.0, 6.0, F, F, F]])
    # row 0: ranks 0, 1 (close), 3 (equal to the neighbour beyond k); row 1: none, padding is no tie
    assert ic.near_tie_share(D) == 3 / 8


def test_check_rejects_right_distances_under_wrong_labels():
    """test_ivfpq_gpu._check on the oracle's own result, and on that result with two labels of a row
    exchanged (2 of 230 labels: under the 1 % allowance, distances untouched), one label repeated,
    and one label of a list that was not probed."""
    from tests.test_ivfpq_gpu import _check
    cs = ic.PY_CASE["chunks"]
    cen, cb, lists, codes, ids, q = ic.py_case_data("chunks")
    Do, Io = oivf.search(q, cen, cb, lists, codes, ids, 10, cs.nprobe)
    Dg = Do.astype(np.float32)
    args = (q, cen, cb, lists, codes, ids, cs.nprobe)
    _check(Dg, Io.copy(), Do, Io, *args)
    swapped, repeated, foreign = Io.copy(), Io.copy(), Io.copy()
    swapped[3, [2, 5]] = Io[3, [5, 2]]
    repeated[4, 7] = Io[4, 6]
    foreign[0, 9] = ids[np.nonzero(~np.isin(lists, oivf.nearest(q, cen, cs.nprobe)[0]))[0][0]]
    for I in (swapped, repeated, foreign):
        assert (I != Io).mean() < ic.MAX_SHARE
        with pytest.raises(AssertionError):
            _check(Dg, I, Do, Io, *args)
