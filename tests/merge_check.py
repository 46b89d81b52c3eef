"""The exact answer of a k-list merge (include/imgrec_knn.h knn_merge_device,
knn_merge_packed_device) in plain numpy, adversarial in-contract inputs, and the cases of
tests/test_merge_kernels_gpu.py.  Used by tests/test_merge_check_cpu.py (the checker itself: every
planted mistake moves it, and the cases' inputs tie as much as they claim), by
tests/test_merge_kernels_gpu.py (the three merge kernels through the C ABI) and by
tests/test_sharded_gloo.py (the sharded protocol with this reference in place of the GPU merge).
No GPU use.

A merge is a pure function: of the gathered entries of a query that carry a label >= 0, the k
smallest by (key, label) — key = d for L2, -d for IP / cosine, compared as floats, so -0.0 ties
+0.0 and the smaller label decides (faiss's rule) — with their d as it came in; then label -1 and
+FLT_MAX (L2) or -FLT_MAX (IP).  Labels are compared for equality and D under ==: no tolerance.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.float32(1.4e-45)            # the smallest positive subnormal, 2^-149
NAN_BITS = 0x7FC00000                       # what pack_chunks writes into the padding float


def is_l2(metric) -> bool:
    return metric == "l2"


def pad_value(metric) -> float:
    return FLT_MAX if is_l2(metric) else -FLT_MAX


def _key(d, metric):
    """The merge key of distances d: d (L2) or -d (IP / cosine), with -0.0 folded into +0.0."""
    d = np.asarray(d)
    return (d if is_l2(metric) else -d) + d.dtype.type(0)


def _reference(gD, gI, k, metric):
    """(D, I, L, P): merge_reference's D and I, and per output slot the list and the position its
    entry came from (-1, -1 for padding)."""
    gD, gI = np.asarray(gD), np.asarray(gI)
    nlists, nq, kin = gD.shape
    D = np.full((nq, k), pad_value(metric), gD.dtype)
    I = np.full((nq, k), -1, np.int64)
    L = np.full((nq, k), -1, np.int64)
    P = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        d = gD[:, q, :].reshape(-1)
        i = gI[:, q, :].reshape(-1).astype(np.int64)
        ok = np.flatnonzero(i >= 0)
        # (lexsort is stable and compares floats: equal keys keep the order of the labels)
        order = ok[np.lexsort((i[ok], _key(d[ok], metric)))][:k]
        n = len(order)
        D[q, :n], I[q, :n] = d[order], i[order]
        L[q, :n], P[q, :n] = order // kin, order % kin
    return D, I, L, P


def merge_reference(gD, gI, k, metric):
    """Best k of the gathered lists gD, gI ([nlists][nq][kin]; label < 0 = no entry) by
    (key, label) -> (D (nq, k) of gD's dtype, I (nq, k) int64), padded with -1 / +-FLT_MAX."""
    return _reference(gD, gI, k, metric)[:2]


# ---- inputs -----------------------------------------------------------------------------------

def key_pool(metric):
    """12 finite float32 distances a list entry can carry: 0, the smallest subnormal, FLT_MAX (the
    padding's value, here with a valid label), neighbours one ulp apart, and for IP both signs."""
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    if is_l2(metric):
        return np.array([0.0, DENORM_MIN, 1e-3, 0.5, one, up, np.nextafter(up, np.float32(2.0)), 2.0,
                         3.5, 1e30, np.nextafter(np.float32(FLT_MAX), np.float32(0.0)), FLT_MAX],
                        np.float32)
    return np.array([0.0, DENORM_MIN, -DENORM_MIN, 0.5, one, up, -one,
                     np.nextafter(-one, np.float32(-2.0)), -2.5, 1e30, FLT_MAX, -FLT_MAX], np.float32)


def _labels(rng, n, lo, hi):
    """n distinct labels of [lo, hi), both ends of the range among them when n >= 2."""
    span = hi - lo
    assert span >= n, f"label range [{lo}, {hi}) holds fewer than {n} labels"
    if span <= 1 << 22:
        out = rng.choice(span, size=n, replace=False).astype(np.int64) + lo
    else:
        out = np.empty(0, np.int64)
        while len(out) < n:
            out = np.unique(np.concatenate([out, rng.integers(lo, hi, 2 * n + 8, dtype=np.int64)]))
        out = rng.permutation(out)[:n]
    if n >= 2:
        for slot, v in ((0, lo), (1, hi - 1)):
            hit = np.flatnonzero(out == v)
            if len(hit):
                out[hit[0]] = out[slot]
            out[slot] = v
        out = rng.permutation(out)
    return out


def make_lists(nlists, nq, kin, metric, seed=0, label_range=(0, 1 << 20), full=False,
               empty_lists=(), empty_queries=(), valid_total=None, pool=None, pool_size=0):
    """Gathered lists (gD float32, gI int64), both [nlists][nq][kin], inside the merge's contract:

    * per query the labels are distinct over all lists: a random subset of label_range = [lo, hi)
      that holds lo and hi - 1;
    * distances come from `pool` (default key_pool(metric)): 12 values, so most ranks tie
      (pool_size: a random pool_size of them, for inputs of a dozen entries);
    * a list holds a random number of entries in [0, kin] (full: kin; lists in empty_lists and
      queries in empty_queries: 0; valid_total = {query: n}: exactly n entries in that query);
    * each list is sorted best-first by (key, label); its tail is label -1 with the padding value.

    Never generated (out of contract): +-inf, NaN, -1 before an entry, a label in two lists."""
    rng = np.random.default_rng([seed, nlists, nq, kin, 0 if is_l2(metric) else 1])
    pool = key_pool(metric) if pool is None else np.asarray(pool, np.float32)
    if pool_size:
        pool = rng.permutation(pool)[:pool_size]
    gD = np.full((nlists, nq, kin), pad_value(metric), np.float32)
    gI = np.full((nlists, nq, kin), -1, np.int64)
    live = np.setdiff1d(np.arange(nlists), np.asarray(list(empty_lists), np.int64))
    for q in range(nq):
        cnt = np.zeros(nlists, np.int64)
        if q in empty_queries:
            continue
        if valid_total is not None and q in valid_total:
            slots = rng.permutation(np.repeat(live, kin))[:valid_total[q]]
            assert len(slots) == valid_total[q], "valid_total exceeds the live lists' capacity"
            np.add.at(cnt, slots, 1)
        else:
            cnt[live] = kin if full else rng.integers(0, kin + 1, len(live))
        n = int(cnt.sum())
        lab = _labels(rng, n, *label_range)
        d = pool[rng.integers(0, len(pool), n)]
        lst = np.repeat(np.arange(nlists), cnt)
        o = np.lexsort((lab, _key(d, metric), lst))          # by list, then (key, label)
        pos = np.arange(n) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        gD[lst, q, pos], gI[lst, q, pos] = d[o], lab[o]
    return gD, gI


def pack_chunks(gD, gI):
    """The packed layout knn_merge_packed_device reads (image_recommender_amd.sharded.packed_layout):
    (nlists, knn_packed_bytes(nq, kin)) uint8, a chunk = nq * kin float32 keys, one padding float
    when that count is odd — here a NaN's bits, so a kernel that reads it shows — then the int64
    labels."""
    from image_recommender_amd.sharded import packed_layout
    nlists, nq, kin = gD.shape
    n = nq * kin
    nbytes, off = packed_layout(nq, kin)
    buf = np.zeros((nlists, nbytes), np.uint8)
    buf[:, :4 * n] = np.ascontiguousarray(gD, np.float32).reshape(nlists, n).view(np.uint8)
    if off > 4 * n:
        buf[:, 4 * n:off] = np.array([NAN_BITS], np.uint32).view(np.uint8)
    buf[:, off:] = np.ascontiguousarray(gI, np.int64).reshape(nlists, n).view(np.uint8)
    return buf


def check_merge(D, I, gD, gI, k, metric, ref=None):
    """Assert that (D, I) is the merge of gD, gI: I equal to merge_reference's, D equal under ==.
    ref: a precomputed _reference(gD, gI, k, metric)."""
    Dr, Ir, L, P = _reference(gD, gI, k, metric) if ref is None else ref
    D, I = np.asarray(D), np.asarray(I)
    assert D.shape == Dr.shape and I.shape == Ir.shape, (D.shape, I.shape, Dr.shape)
    bad = (I != Ir) | ~(D == Dr)
    if not bad.any():
        return
    q, r = map(int, np.argwhere(bad)[0])
    where = (f"list {L[q, r]} position {P[q, r]}" if L[q, r] >= 0
             else "nowhere: padding is expected here")
    raise AssertionError(
        f"merge differs first at query {q} rank {r}: got (d={D[q, r]!r}, label={int(I[q, r])}), "
        f"expected (d={Dr[q, r]!r}, label={int(Ir[q, r])}) from {where}; "
        f"{int(bad.sum())} of {bad.size} slots differ (k={k}, {metric}, lists {gD.shape})")


def tied_share(gD, gI, k, metric):
    """Share of the answer's occupied ranks whose key equals a neighbour's key (float comparison).
    The neighbours are those of the full order of the query's entries, so the k-th rank's
    successor — the entry a wrong tie-break would return instead — counts."""
    Dr, Ir, _, _ = _reference(gD, gI, k + 1, metric)
    key = _key(Dr, metric)
    have = Ir >= 0
    eq = (key[:, 1:] == key[:, :-1]) & have[:, 1:] & have[:, :-1]
    tied = np.zeros_like(have)
    tied[:, 1:] |= eq
    tied[:, :-1] |= eq
    ranks = have[:, :k]
    return float(tied[:, :k][ranks].sum()) / max(1, int(ranks.sum()))


# ---- the cases of tests/test_merge_kernels_gpu.py ------------------------------------------------

def _case(name, nlists, nq, kin, k, **opts):
    return dict(id=f"{name}-{nlists}x{nq}x{kin}-k{k}", nlists=nlists, nq=nq, kin=kin, k=k,
                opts=tuple(sorted(opts.items())))


# one wave per query (k <= 32, not (nq < 1024 and nlists > 256)): every k around the KM = 8, 10, 16,
# 32 boundaries, a lane walking one, two and three lists, kin below / at / above k and around the
# 8-wide batch, a partly idle last block of 4 queries
WAVE_CASES = [
    _case("wave", 1, 4, 40, 8),
    _case("wave", 2, 1, 32, 9),
    _case("wave", 63, 3, 7, 10),
    _case("wave", 64, 5, 8, 11),
    _case("wave", 65, 4, 9, 16),
    _case("wave", 130, 5, 1, 17),
    _case("wave", 130, 3, 40, 32),
    _case("wave", 65, 1, 1, 1),
    _case("wave", 2, 3, 8, 32, pool_size=4),             # nlists * kin < k
    _case("wave", 64, 4, 32, 32, full=True),
    _case("wave", 130, 5, 9, 1),
    _case("wave", 63, 1, 40, 17),
]

# four waves per query (nq < 1024 and nlists > 256); wave w walks lists 64 w .. 64 w + 63, + 256, ...
WAVE4_CASES = [
    _case("wave4", 257, 1, 2, 1),
    _case("wave4", 257, 3, 9, 10),
    _case("wave4", 300, 3, 2, 32),
    _case("wave4", 300, 1, 9, 10),
    _case("wave4", 513, 1, 9, 32),
    _case("wave4", 513, 3, 2, 1),
    _case("wave4-lists-from-256", 513, 3, 9, 10, empty_lists=tuple(range(256))),
    _case("wave4-one-wave-only", 513, 1, 2, 32,
          empty_lists=tuple(l for l in range(513) if (l % 256) // 64 != 1)),
]

# in-LDS radix select (32 < k <= 1024, nlists * kin <= 8192)
# (a dozen entries tie only over fewer keys; a lone list is full, or one query could hold nothing)
RADIX_CASES = [_case("radix", nl, nq, kin, k, **({"pool_size": 3} if nl * kin < k else {}),
                     **({"full": True} if nl == 1 or (nq == 1 and nl * kin < k) else {}))
               for nq in (1, 3) for nl, kin, k in
               [(2, 10, 33), (1, 40, 33), (8, 100, 100), (64, 128, 1024), (3, 1000, 1024),
                (8, 1024, 1000), (130, 63, 64)]]

# segmented sort (k <= 1024 with nlists * kin > 8192, or k > 1024)
SORT_CASES = [_case("sort", nl, 3, kin, k) for nl, kin, k in
              [(65, 128, 1024), (9, 1000, 33), (8, 2000, 2000), (3, 600, 2000), (2, 1025, 1025),
               (1, 1500, 1025)]]

# one shape per kernel for what runs "on all routes": (nlists, kin, k), nq = 3 and kin odd, so
# nq * kin is odd and the packed layout's padding float is in play
ROUTES = {"wave": (9, 11, 10), "wave4": (260, 5, 10), "radix": (6, 51, 100),
          "sort": (9, 1001, 40), "sort-k>1024": (3, 701, 1100)}

# label ranges [lo, hi): a sign-extending or truncating cast shows at 2^31 - 1 | 2^31 and at
# 2^32 - 1; make_lists puts lo and hi - 1 among every query's labels
LABEL_RANGES = {"around-2^31": ((1 << 31) - 6000, (1 << 31) + 6000),
                "up-to-2^32": ((1 << 32) - 12000, 1 << 32)}
WIDE_LABELS = (1 << 32, (1 << 62) + 1)      # k <= KNN_MAX_K only: carried exactly

# the lists of the signed-zero case: (nlists, nq, kin), merged at k = 32 and at k = 33
ZERO_SHAPES = {"wave|radix": (6, 3, 11), "wave4|radix": (260, 3, 5), "wave|sort": (9, 3, 1001)}


def _route_cases():
    out = []
    for name, (nl, kin, k) in ROUTES.items():
        out.append(_case(f"{name}-empty-and-k-1", nl, 3, kin, k, empty_queries=(0,),
                         valid_total=((1, k - 1),)))
        out.append(_case(f"{name}-one-key", nl, 3, kin, k, pool=(2.5,)))
        out.append(_case(f"{name}-plain", nl, 3, kin, k))
        for rname, rng_ in LABEL_RANGES.items():
            out.append(_case(f"{name}-labels-{rname}", nl, 3, kin, k, label_range=rng_))
    for name in ("wave", "wave4"):
        nl, kin, k = ROUTES[name]
        out.append(_case(f"{name}-labels-to-2^62", nl, 3, kin, k, label_range=WIDE_LABELS))
    return out


ROUTE_CASES = _route_cases()
# (one seed: k = 32 and k = 33 merge the same lists)
ZERO_CASES = [_case(f"zeros-{name}", nl, nq, kin, k, pool=(0.0, -0.0), seed=1000)
              for name, (nl, nq, kin) in ZERO_SHAPES.items() for k in (32, 33)]
# the same lists at nq = 1024 (one wave per query) and their first 3 queries (four waves)
WPQ_PAIR = _case("wave-nq1024", 257, 1024, 2, 3)

ALL_CASES = WAVE_CASES + WAVE4_CASES + RADIX_CASES + SORT_CASES + ROUTE_CASES + ZERO_CASES + [WPQ_PAIR]
CASE_IDS = [c["id"] for c in ALL_CASES]


def route_of(nlists, nq, kin, k):
    """The kernel a merge dispatches to (csrc/knn_capi.cpp, knn_kernels.hip, knn_hugek.hip)."""
    if k <= 32:
        return "wave4" if nq < 1024 and nlists > 256 else "wave"
    return "radix" if k <= 1024 and nlists * kin <= 8192 else "sort"


@lru_cache(maxsize=None)
def _case_inputs(cid, metric):
    c = next(c for c in ALL_CASES if c["id"] == cid)
    opts = dict(c["opts"])
    if "valid_total" in opts:
        opts["valid_total"] = dict(opts["valid_total"])
    seed = opts.pop("seed", CASE_IDS.index(cid))
    gD, gI = make_lists(c["nlists"], c["nq"], c["kin"], metric, seed=seed, **opts)
    ref = _reference(gD, gI, c["k"], metric)
    for a in (gD, gI) + ref:
        a.setflags(write=False)
    return gD, gI, ref


def case_inputs(case, metric):
    """(gD, gI, ref) of a case, computed once per (case, metric) and read-only: ref is
    _reference(gD, gI, k, metric), what check_merge takes as `ref`.  cosine = IP in a merge."""
    return _case_inputs(case["id"], "l2" if is_l2(metric) else "ip")
