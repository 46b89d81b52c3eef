"""tests/merge_check.py itself, without a GPU: the reference gives a hand-worked answer,
check_merge rejects every planted mistake a merge kernel could make, make_lists keeps its own
contract, and the inputs of every case of tests/test_merge_kernels_gpu.py tie on at least half of
their ranks — so the GPU cases cannot quietly become tie-free.  Also the label-range refusal of
ShardedIndex.search, which needs no device.
"""
import numpy as np
import pytest

from tests import merge_check as mc

FLT_MAX = mc.FLT_MAX
METRICS = ("l2", "ip")


def _ordered_bits(key):
    """The u32 whose unsigned order is the float order of key, except that it splits the zeros:
    every -0.0 before every +0.0 (csrc/wave_ops.h key_bits_ordered)."""
    u = np.asarray(key, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def _merge_by(gD, gI, k, metric, order):
    """A merge that ranks a query's valid entries by order(d, labels, flat index) -> permutation."""
    nlists, nq, kin = gD.shape
    D = np.full((nq, k), mc.pad_value(metric), np.float32)
    I = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        d, i = gD[:, q, :].reshape(-1), gI[:, q, :].reshape(-1)
        ok = np.flatnonzero(i >= 0)
        o = ok[order(d[ok], i[ok], ok)][:k]
        D[q, :len(o)], I[q, :len(o)] = d[o], i[o]
    return D, I


def _rejected(D, I, gD, gI, k, metric):
    """check_merge raises on (D, I); the planted answer really differs from the reference."""
    Dr, Ir = mc.merge_reference(gD, gI, k, metric)
    assert (I != Ir).any() or (D != Dr).any(), "the corruption changed nothing"
    mc.check_merge(Dr, Ir, gD, gI, k, metric)          # the reference itself passes
    with pytest.raises(AssertionError, match="merge differs first at query") as e:
        mc.check_merge(D, I, gD, gI, k, metric)
    return str(e.value)


def test_reference_on_a_hand_worked_merge():
    """Two queries over three lists of three, worked by hand."""
    P = FLT_MAX
    gD = np.array([[[1.0, 2.0, P], [0.0, P, P]],
                   [[1.0, 1.0, 3.0], [-0.0, 5.0, P]],
                   [[P, P, P], [P, P, P]]], np.float32)
    gI = np.array([[[7, 1, -1], [9, -1, -1]],
                   [[2, 8, 0], [4, 6, -1]],
                   [[-1, -1, -1], [-1, -1, -1]]], np.int64)
    D, I = mc.merge_reference(gD, gI, 4, "l2")
    np.testing.assert_array_equal(I, [[2, 7, 8, 1], [4, 9, 6, -1]])
    np.testing.assert_array_equal(D, np.array([[1, 1, 1, 2], [-0.0, 0.0, 5, P]], np.float32))
    assert np.signbit(D[1, 0]) and not np.signbit(D[1, 1])         # d as it came in
    # IP: the largest d first, the same tie rule, -FLT_MAX padding (the +FLT_MAX d's carry no label)
    D, I = mc.merge_reference(gD, gI, 6, "ip")
    np.testing.assert_array_equal(I, [[0, 1, 2, 7, 8, -1], [6, 4, 9, -1, -1, -1]])
    np.testing.assert_array_equal(D, np.array([[3, 2, 1, 1, 1, -P], [5, -0.0, 0, -P, -P, -P]], np.float32))
    assert mc.merge_reference(gD.astype(np.float64), gI, 2, "l2")[0].dtype == np.float64
    mc.check_merge(D, I, gD, gI, 6, "cosine")                    # cosine merges as IP


@pytest.mark.parametrize("metric", METRICS)
def test_rejects_a_tie_broken_by_list_index(metric):
    gD, gI = mc.make_lists(5, 3, 6, metric, seed=1, full=True)
    D, I = _merge_by(gD, gI, 8, metric, lambda d, i, at: np.lexsort((at, mc._key(d, metric))))
    msg = _rejected(D, I, gD, gI, 8, metric)
    assert "rank" in msg and "from list" in msg and "position" in msg and "label=" in msg


@pytest.mark.parametrize("metric", METRICS)
def test_rejects_negative_zero_ranked_before_positive_zero(metric):
    """What packing key_bits_ordered(key) | label does without folding the zeros."""
    gD, gI = mc.make_lists(4, 2, 8, metric, seed=2, full=True, pool=(0.0, -0.0))
    split = lambda d, i, at: np.lexsort((i, _ordered_bits(d if mc.is_l2(metric) else -d)))
    D, I = _merge_by(gD, gI, 12, metric, split)
    _rejected(D, I, gD, gI, 12, metric)
    Ir = mc.merge_reference(gD, gI, 12, metric)[1]
    assert (np.diff(Ir, axis=1) > 0).all()              # one key: the answer is label-ascending


def test_rejects_a_label_without_its_upper_32_bits():
    gD, gI = mc.make_lists(3, 2, 5, "l2", seed=3, full=True, label_range=mc.WIDE_LABELS)
    D, I = mc.merge_reference(gD, gI, 7, "l2")
    assert (I >= 1 << 32).all() and I.max() == 1 << 62
    _rejected(D, I & 0xFFFFFFFF, gD, gI, 7, "l2")
    one = I.copy()
    one[1, 6] &= 0xFFFFFFFF
    assert "query 1 rank 6" in _rejected(D, one, gD, gI, 7, "l2")


@pytest.mark.parametrize("metric", METRICS)
def test_rejects_a_missing_entry_of_a_list_past_64(metric):
    gD, gI = mc.make_lists(130, 2, 3, metric, seed=4, full=True)
    hD, hI = gD.copy(), gI.copy()
    hI[64:] = -1                                        # a merge that never walks a second list
    D, I = mc.merge_reference(hD, hI, 16, metric)
    msg = _rejected(D, I, gD, gI, 16, metric)
    assert int(msg.split("from list ")[1].split()[0]) >= 64


@pytest.mark.parametrize("metric", METRICS)
def test_rejects_the_kth_entry_replaced_by_the_next(metric):
    gD, gI = mc.make_lists(6, 3, 9, metric, seed=5, full=True)
    D1, I1 = mc.merge_reference(gD, gI, 11, metric)
    D, I = D1[:, :10].copy(), I1[:, :10].copy()
    D[:, 9], I[:, 9] = D1[:, 10], I1[:, 10]
    assert "rank 9" in _rejected(D, I, gD, gI, 10, metric)


def test_rejects_ip_padding_with_positive_flt_max():
    gD, gI = mc.make_lists(2, 2, 4, "ip", seed=6)
    D, I = mc.merge_reference(gD, gI, 12, "ip")
    assert (I == -1).any()
    _rejected(np.where(I < 0, FLT_MAX, D).astype(np.float32), I, gD, gI, 12, "ip")
    # and L2 padding with -FLT_MAX
    gD, gI = mc.make_lists(2, 2, 4, "l2", seed=6)
    D, I = mc.merge_reference(gD, gI, 12, "l2")
    _rejected(np.where(I < 0, -FLT_MAX, D).astype(np.float32), I, gD, gI, 12, "l2")


@pytest.mark.parametrize("metric", METRICS)
def test_rejects_a_padded_slot_with_a_valid_label(metric):
    gD, gI = mc.make_lists(2, 2, 4, metric, seed=7)
    D, I = mc.merge_reference(gD, gI, 12, metric)
    q, r = np.argwhere(I < 0)[0]
    bad = I.copy()
    bad[q, r] = gI[gI >= 0][0]
    assert "padding is expected" in _rejected(D, bad, gD, gI, 12, metric)


def test_rejects_a_valid_flt_max_entry_replaced_by_padding():
    """A kernel that takes key == FLT_MAX for `empty`: the slot's D is right, its label is not."""
    for metric, worst in (("l2", FLT_MAX), ("ip", -FLT_MAX)):
        gD, gI = mc.make_lists(3, 2, 4, metric, seed=8, full=True, pool=(1.0, worst))
        D, I = mc.merge_reference(gD, gI, 12, metric)
        hit = (D == np.float32(worst)) & (I >= 0)
        assert hit.any()
        _rejected(D, np.where(hit, -1, I), gD, gI, 12, metric)


def test_rejects_nan_and_unwritten_slots():
    gD, gI = mc.make_lists(3, 2, 4, "l2", seed=9, full=True)
    D, I = mc.merge_reference(gD, gI, 5, "l2")
    bad = D.copy()
    bad[1, 2] = np.nan
    assert "query 1 rank 2" in _rejected(bad, I, gD, gI, 5, "l2")


# ---- the inputs -------------------------------------------------------------------------------------

def _assert_contract(gD, gI, metric, label_range):
    nlists, nq, kin = gD.shape
    assert gD.dtype == np.float32 and gI.dtype == np.int64
    assert np.isfinite(gD).all()
    valid = gI >= 0
    assert (gI[~valid] == -1).all() and (gD[~valid] == np.float32(mc.pad_value(metric))).all()
    assert not (valid[:, :, 1:] & ~valid[:, :, :-1]).any(), "an entry after an empty slot"
    lo, hi = label_range
    assert (gI[valid] >= lo).all() and (gI[valid] < hi).all()
    key = mc._key(gD, metric)
    both = valid[:, :, 1:] & valid[:, :, :-1]
    up = (key[:, :, 1:] > key[:, :, :-1]) | ((key[:, :, 1:] == key[:, :, :-1]) & (gI[:, :, 1:] > gI[:, :, :-1]))
    assert up[both].all(), "a list is not sorted by (key, label)"
    for q in range(nq):
        lab = gI[:, q, :][valid[:, q, :]]
        assert len(np.unique(lab)) == len(lab), "a label in two slots of one query"
        if len(lab) >= 2:
            assert lab.min() == lo and lab.max() == hi - 1


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", mc.ALL_CASES, ids=mc.CASE_IDS)
def test_case_inputs_are_in_contract_and_tie(case, metric):
    gD, gI, ref = mc.case_inputs(case, metric)
    opts = dict(case["opts"])
    assert gD.shape == (case["nlists"], case["nq"], case["kin"])
    _assert_contract(gD, gI, metric, opts.get("label_range", (0, 1 << 20)))
    valid = gI >= 0
    for l in opts.get("empty_lists", ()):
        assert not valid[l].any()
    for q in opts.get("empty_queries", ()):
        assert not valid[:, q].any()
    for q, n in opts.get("valid_total", ()):
        assert valid[:, q].sum() == n
    if opts.get("full"):
        assert valid.all()
    if "pool" in opts:
        assert set(np.unique(gD[valid]).tolist()) <= set(np.float32(opts["pool"]).tolist())
    else:
        assert set(np.unique(gD[valid]).tolist()) <= set(mc.key_pool(metric).tolist())
    assert valid.any()
    share = mc.tied_share(gD, gI, case["k"], metric)
    assert share >= 0.5, f"only {share:.2f} of the ranks tie"
    mc.check_merge(ref[0], ref[1], gD, gI, case["k"], metric, ref=ref)


def test_cases_reach_every_kernel_and_edge():
    """The dispatch of csrc/knn_capi.cpp, knn_kernels.hip and knn_hugek.hip, restated in
    merge_check.route_of, sends each group of cases where its name says."""
    def routes(cases):
        return {mc.route_of(c["nlists"], c["nq"], c["kin"], c["k"]) for c in cases}
    assert routes(mc.WAVE_CASES) == {"wave"} and routes(mc.WAVE4_CASES) == {"wave4"}
    assert routes(mc.RADIX_CASES) == {"radix"} and routes(mc.SORT_CASES) == {"sort"}
    assert routes([mc.WPQ_PAIR]) == {"wave"}
    assert mc.route_of(257, 3, 2, 3) == "wave4"
    for name, (nl, kin, k) in mc.ROUTES.items():
        assert mc.route_of(nl, 3, kin, k) == name.split("-")[0]
        assert (3 * kin) % 2 == 1                      # the packed layout's padding float exists
    for name, (nl, nq, kin) in mc.ZERO_SHAPES.items():
        assert [mc.route_of(nl, nq, kin, 32), mc.route_of(nl, nq, kin, 33)] == name.split("|")
    wave = mc.WAVE_CASES
    assert {c["k"] for c in wave} == {1, 8, 9, 10, 11, 16, 17, 32}
    assert {c["nlists"] for c in wave} == {1, 2, 63, 64, 65, 130}
    assert {c["kin"] for c in wave} == {1, 7, 8, 9, 32, 40}
    assert {c["nq"] for c in wave} == {1, 3, 4, 5}
    assert any(c["nlists"] * c["kin"] == 8192 for c in mc.RADIX_CASES)
    assert any(c["nlists"] * c["kin"] < c["k"] for c in mc.RADIX_CASES)
    assert any(c["nlists"] * c["kin"] < c["k"] for c in mc.SORT_CASES)
    # the all-keys-equal inputs hold one key; the signed-zero lists hold both zeros in every query
    for c in mc.ZERO_CASES:
        for metric in METRICS:
            gD, gI, _ = mc.case_inputs(c, metric)
            neg = np.signbit(gD) & (gI >= 0)
            pos = ~np.signbit(gD) & (gI >= 0)
            assert neg.any(axis=(0, 2)).all() and pos.any(axis=(0, 2)).all()
    a, b = mc.ZERO_CASES[0], mc.ZERO_CASES[1]
    assert (a["k"], b["k"]) == (32, 33)
    np.testing.assert_array_equal(mc.case_inputs(a, "l2")[1], mc.case_inputs(b, "l2")[1])


def test_make_lists_options():
    gD, gI = mc.make_lists(4, 3, 5, "ip", seed=3, empty_lists=(1,), empty_queries=(2,),
                           valid_total={0: 7}, label_range=mc.LABEL_RANGES["around-2^31"])
    _assert_contract(gD, gI, "ip", mc.LABEL_RANGES["around-2^31"])
    assert (gI[1] == -1).all() and (gI[:, 2] == -1).all() and (gI[:, 0] >= 0).sum() == 7
    lab = gI[gI >= 0]
    assert ((1 << 31) - 1 < lab).any() and (lab < (1 << 31)).any()
    h = mc.make_lists(4, 3, 5, "ip", seed=3)
    np.testing.assert_array_equal(h[1], mc.make_lists(4, 3, 5, "ip", seed=3)[1])
    assert (h[1] != mc.make_lists(4, 3, 5, "ip", seed=4)[1]).any()


@pytest.mark.parametrize("nq,kin", [(3, 5), (2, 5), (1, 1)])
def test_pack_chunks_is_the_packed_layout(nq, kin):
    import torch
    from image_recommender_amd.sharded import packed_layout, packed_views
    gD, gI = mc.make_lists(3, nq, kin, "l2", seed=1)
    buf = mc.pack_chunks(gD, gI)
    nbytes, off = packed_layout(nq, kin)
    assert buf.shape == (3, nbytes) and buf.dtype == np.uint8
    for l in range(3):
        D, I = packed_views(torch.from_numpy(buf[l]), nq, kin)
        np.testing.assert_array_equal(D.numpy(), gD[l])
        np.testing.assert_array_equal(I.numpy(), gI[l])
    if (nq * kin) % 2:
        pad = buf[:, 4 * nq * kin:off].copy().view(np.uint32)
        assert off == 4 * nq * kin + 4 and (pad == mc.NAN_BITS).all() and np.isnan(pad.view(np.float32)).all()
    else:
        assert off == 4 * nq * kin


# ---- the label-range refusal (include/imgrec_knn.h knn_merge_device) --------------------------------

def test_sharded_search_refuses_labels_past_2_32_for_large_k():
    from image_recommender_amd import sharded
    sharded.check_merge_labels(1 << 32, 33)            # labels 0 .. 2^32 - 1 fit
    sharded.check_merge_labels(1 << 40, 32)            # k <= KNN_MAX_K carries 64 bits
    with pytest.raises(ValueError, match="below 2\\^32"):
        sharded.check_merge_labels((1 << 32) + 1, 33)
    # ShardedIndex.search asks before it touches a device (the instance is built without one)
    ix = object.__new__(sharded.ShardedIndex)
    ix.ntotal_global = (1 << 32) + 1
    with pytest.raises(ValueError, match="below 2\\^32"):
        ix.search(None, 1025)
    with pytest.raises(ValueError, match="below 2\\^32"):
        ix.search(None, 33)
