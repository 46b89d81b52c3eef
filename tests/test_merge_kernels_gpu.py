"""The three k-list merge kernels through their C ABI (include/imgrec_knn.h knn_merge_device and
knn_merge_packed_device, via sharded.merge_gathered_device / merge_packed_device) against the exact
answer of tests/merge_check.py: I equal, D equal under ==, no tolerance.  The inputs are
merge_check.make_lists': labels distinct per query, keys from a pool of 12 values so that most
ranks tie across lists (tests/test_merge_check_cpu.py asserts at least half, per case), lists of
random length, empty lists and queries, FLT_MAX and subnormal keys with valid labels.

Which kernel a call reaches, quoted from the dispatch:

* csrc/knn_capi.cpp, both entry points: ``if (k > KNN_MAX_K) { launch_merge_any(...) }`` else
  ``launch_merge`` / ``launch_merge_strided`` (KNN_MAX_K = 32);
* csrc/knn_kernels.hip launch_merge_strided: ``const bool wide = nq < 1024 && nlists > 256;`` —
  knn_merge_kernel<KM, 4> (four waves per query) when wide, else knn_merge_kernel<KM, 1>, with
  ``if (k <= 8) ... (8); else if (k <= 10) ... (10); else if (k <= 16) ... (16); else if (k <= 32)
  ... (32)``;
* csrc/knn_hugek.hip launch_merge_any: ``if (k <= KNN_MAX_K_LARGE && (int64_t)nlists * kin <=
  8192) return launch_merge_large(...)`` (largek_merge_kernel, csrc/knn_largek.hip: the in-LDS
  radix select), else ``launch_merge_huge`` (pack, rocPRIM segmented sort, write).

Cases (merge_check.py; route_of restates the conditions above and test_merge_check_cpu.py checks
each group lands where it says):

* WAVE_CASES -> knn_merge_kernel<KM, 1>: k on both sides of every KM boundary, 1 .. 130 lists (a
  lane walks one, two, three lists), kin below / at / above k and around the 8-wide batch loads,
  nq 1 .. 5 (a partly idle last block); WPQ_PAIR: nq = 1024 x 257 lists, still one wave per query;
* WAVE4_CASES -> knn_merge_kernel<KM, 4>: 257 .. 513 lists, nq 1 and 3, every entry in lists
  >= 256, every entry in one wave's lists;
* RADIX_CASES -> largek_merge_kernel: M = nlists * kin from below k to exactly 8192;
* SORT_CASES -> launch_merge_huge: k <= 1024 with M > 8192, and k > 1024 with M >= k and M < k;
* ROUTE_CASES, on one shape per kernel: an empty query beside one with exactly k - 1 entries, one
  key everywhere, labels around 2^31 and up to 2^32 - 1 (up to 2^62 on the k <= 32 kernel, which
  carries 64 bits; the k > 32 kernels' contract is [0, 2^32)), all with an odd nq * kin, so the
  packed layout's padding float (a NaN here) sits between keys and labels;
* ZERO_CASES: +0.0 and -0.0 keys over interleaved labels, merged at k = 32 and k = 33.

Every call writes between two guard rows, which must stay untouched, into a body pre-filled with
the guard values (an unwritten slot fails the comparison), leaves its inputs as they were, and the
packed and gathered forms must return the same bytes.

Not covered, by decision: launch_merge_huge's loop over query chunks.  It takes a second chunk
only past 2^27 gathered entries per call or 65535 queries — gigabytes of sort workspace, outside
a test that runs in seconds.
"""
import numpy as np
import pytest
import torch

from tests import merge_check as mc

pytestmark = pytest.mark.gpu

GUARD_I = -7777                 # no label: labels are >= 0 or the padding -1
GUARD_D = 0x7FC12345            # a NaN's bits: equal to no distance
METRICS = ("l2", "ip")


def _metric_code(metric):
    from image_recommender_amd import faiss_compat as faiss
    return {"l2": faiss.METRIC_L2, "ip": faiss.METRIC_INNER_PRODUCT, "cosine": faiss.METRIC_COSINE}[metric]


def _guarded(nq, k):
    D = torch.full((nq + 2, k), GUARD_D, dtype=torch.int32, device="cuda").view(torch.float32)
    I = torch.full((nq + 2, k), GUARD_I, dtype=torch.int64, device="cuda")
    return D, I


def _body(bufD, bufI, what):
    """Host copies of the rows between the guard rows, after asserting the guards are intact."""
    hD, hI = bufD.cpu().numpy(), bufI.cpu().numpy()
    for row in (0, -1):
        assert (hD[row].view(np.uint32) == GUARD_D).all() and (hI[row] == GUARD_I).all(), \
            f"{what}: wrote outside its output (guard row {row})"
    return hD[1:-1], hI[1:-1]


def _merge_both(gD, gI, k, metric, stream=None):
    """[(D, I) of merge_gathered_device, (D, I) of merge_packed_device] on the host."""
    from image_recommender_amd.sharded import merge_gathered_device, merge_packed_device
    nlists, nq, kin = gD.shape
    packed = mc.pack_chunks(gD, gI)
    dD, dI, dP = (torch.from_numpy(np.array(a)).cuda() for a in (gD, gI, packed))   # (read-only inputs: copies)
    code, handle = _metric_code(metric), (stream.cuda_stream if stream is not None else 0)
    outs = []
    for what in ("gathered", "packed"):
        bufD, bufI = _guarded(nq, k)
        out = (bufD[1:nq + 1], bufI[1:nq + 1])
        torch.cuda.synchronize()
        if what == "gathered":
            merge_gathered_device(dD, dI, k, code, handle, out=out)
        else:
            merge_packed_device(dP, nq, kin, k, code, handle, out=out)
        (stream if stream is not None else torch.cuda.current_stream()).synchronize()
        outs.append(_body(bufD, bufI, what))
    torch.cuda.synchronize()
    assert (dD.cpu().numpy().view(np.uint32) == gD.view(np.uint32)).all(), "the keys were written to"
    assert (dI.cpu().numpy() == gI).all(), "the labels were written to"
    assert (dP.cpu().numpy() == packed).all(), "the packed chunks were written to"
    return outs


def _check_case(case, metric, stream=None):
    gD, gI, ref = mc.case_inputs(case, metric)
    (D, I), (Dp, Ip) = _merge_both(gD, gI, case["k"], metric, stream)
    mc.check_merge(D, I, gD, gI, case["k"], metric, ref=ref)
    mc.check_merge(Dp, Ip, gD, gI, case["k"], metric, ref=ref)
    assert (D.view(np.uint32) == Dp.view(np.uint32)).all() and (I == Ip).all(), \
        "the packed and the gathered merge differ"
    return D, I


def _ids(cases):
    return [c["id"] for c in cases]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", mc.WAVE_CASES, ids=_ids(mc.WAVE_CASES))
def test_one_wave_per_query(gpu, case, metric):
    _check_case(case, metric)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", mc.WAVE4_CASES, ids=_ids(mc.WAVE4_CASES))
def test_four_waves_per_query(gpu, case, metric):
    _check_case(case, metric)


@pytest.mark.parametrize("metric", METRICS)
def test_one_and_four_waves_agree_on_the_same_lists(gpu, metric):
    """nq = 1024 x 257 lists runs one wave per query; its first 3 queries alone run four."""
    c = mc.WPQ_PAIR
    assert mc.route_of(c["nlists"], c["nq"], c["kin"], c["k"]) == "wave"
    assert mc.route_of(c["nlists"], 3, c["kin"], c["k"]) == "wave4"
    D, I = _check_case(c, metric)
    gD, gI, _ = mc.case_inputs(c, metric)
    hD, hI = np.ascontiguousarray(gD[:, :3]), np.ascontiguousarray(gI[:, :3])
    (D4, I4), (D4p, I4p) = _merge_both(hD, hI, c["k"], metric)
    mc.check_merge(D4, I4, hD, hI, c["k"], metric)
    mc.check_merge(D4p, I4p, hD, hI, c["k"], metric)
    assert (D4.view(np.uint32) == D[:3].view(np.uint32)).all() and (I4 == I[:3]).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", mc.RADIX_CASES, ids=_ids(mc.RADIX_CASES))
def test_radix_select(gpu, case, metric):
    _check_case(case, metric)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", mc.SORT_CASES, ids=_ids(mc.SORT_CASES))
def test_segmented_sort(gpu, case, metric):
    _check_case(case, metric)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", mc.ROUTE_CASES, ids=_ids(mc.ROUTE_CASES))
def test_every_route(gpu, case, metric):
    """Empty and k - 1 queries, one key everywhere (the answer is the k smallest labels), label
    ranges, an odd nq * kin: merge_check.ROUTE_CASES on one shape per kernel."""
    D, I = _check_case(case, metric)
    opts = dict(case["opts"])
    if "valid_total" in opts:
        assert (I[0] == -1).all() and (I[1, :-1] >= 0).all() and I[1, -1] == -1
    if "pool" in opts:
        assert (np.diff(I, axis=1)[I[:, 1:] >= 0] > 0).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", list(mc.ZERO_SHAPES), ids=lambda s: s.replace("|", "-then-"))
def test_signed_zeros_order_by_label_on_every_route(gpu, shape, metric):
    """+0.0 and -0.0 are one key: the same lists merged at k = 32 (register lists, a float
    comparison) and at k = 33 (key bits packed beside the label) agree on their first 32."""
    c32, c33 = (c for c in mc.ZERO_CASES if c["id"].startswith(f"zeros-{shape}-"))
    assert (c32["k"], c33["k"]) == (32, 33)
    D32, I32 = _check_case(c32, metric)
    D33, I33 = _check_case(c33, metric)
    assert (I32 == I33[:, :32]).all() and (D32 == D33[:, :32]).all()
    assert (np.diff(I33, axis=1)[I33[:, 1:] >= 0] > 0).all()      # label-ascending: one key


def test_cosine_merges_as_inner_product(gpu):
    for name in ("wave-plain", "radix-plain"):
        case = next(c for c in mc.ROUTE_CASES if c["id"].startswith(name))
        D, I = _check_case(case, "cosine")
        Dip, Iip = _check_case(case, "ip")
        assert (D.view(np.uint32) == Dip.view(np.uint32)).all() and (I == Iip).all()


@pytest.mark.parametrize("route", list(mc.ROUTES))
def test_on_a_side_stream_and_twice(gpu, route):
    """The merge runs on the stream it is given (the sort route allocates its workspace in stream
    order there), and a second call returns the same bytes."""
    case = next(c for c in mc.ROUTE_CASES if c["id"].startswith(f"{route}-plain"))
    side = torch.cuda.Stream()
    first = _check_case(case, "l2", stream=side)
    again = _check_case(case, "l2", stream=side)
    default = _check_case(case, "l2")
    for D, I in (again, default):
        assert (D.view(np.uint32) == first[0].view(np.uint32)).all() and (I == first[1]).all()


def test_multi_device_index_refuses_labels_past_2_32_for_large_k(gpu):
    """include/imgrec_knn.h knn_merge_device: the k > KNN_MAX_K merges carry labels below 2^32, so
    a sharded index whose labels pass it refuses such a search; k <= KNN_MAX_K carries them."""
    from image_recommender_amd import faiss_compat as faiss
    xb = np.eye(4, 8, dtype=np.float32)
    idx = faiss.IndexFlatL2(8, devices=[0, 0])
    idx.add(xb)
    idx.set_id_offset((1 << 32) - 3)                   # labels 2^32 - 3 .. 2^32: one too far
    D, I = idx.search(xb[:1], 32)
    assert I[0, :4].tolist() == [(1 << 32) - 3 + j for j in (0, 1, 2, 3)] and (I[0, 4:] == -1).all()
    with pytest.raises(faiss.KnnError, match="2\\^32"):
        idx.search(xb[:1], 33)
    idx.set_id_offset((1 << 32) - 4)                   # 2^32 - 4 .. 2^32 - 1: inside the contract
    D, I = idx.search(xb[:1], 33)
    assert I[0, :4].tolist() == [(1 << 32) - 4 + j for j in (0, 1, 2, 3)] and (I[0, 4:] == -1).all()
