"""Checker and parameter table of the range-search tests (test helper).

check_range(lims, D, I, xb, xq, radius, metric) checks a range_search result against float64,
with b = oracle.flat_knn.fp32_error_bound per pair:
  (a) lims is monotone, lims[0] == 0, lims[-1] == len(D) == len(I); labels are unique per query
      and lie in [0, ntotal);
  (b) every returned D satisfies the strict threshold (D < radius for L2, D > radius for IP);
  (c) |D - d64(pair)| <= b for every returned pair;
  (d) every pair with d64 < radius - b is present and no pair with d64 > radius + b is (signs
      mirrored for IP / cosine); pairs inside the band may go either way;
  (e) every segment is sorted by (D best first, label).
It returns (band, expected): the pairs with |d64 - radius| <= b and the pairs inside the radius.

range_conditions gives the same two numbers from the oracle alone.  Every test that uses the
checker first asserts band <= 0.02 x expected and expected >= 5 x nq (assert_conditions): a band
that is thin beside a result that is not tiny, so the band cannot hide a wrong kernel.

CASES is the one table of (shape, seed, radius) both test files use: the CPU file proves the two
conditions for every entry, the GPU file runs them.  A radius is the float32 value of a low
quantile of the case's float64 distances (a high one of the inner products).
"""
import functools

import numpy as np

from oracle.flat_knn import fp32_error_bound
from tests.datagen import concat_rows, mixture

BAND_FRAC = 0.02     # band <= BAND_FRAC x expected
MIN_HITS = 5         # expected >= MIN_HITS x nq

# name: (N, d, nq, metric, data, seed, quantile); data "mixture[:centres]" (20 centres unless
# stated: at d = 768 the same-cluster L2 distances of 20 centres sit so close together that the
# band at their 10 % point holds 4 % of the hits; with 300 centres the radius falls past them)
CASES = {
    "l2_1000x96_q33": (1000, 96, 33, "l2", "mixture", 11, 0.01),       # partial row tile / query block
    "l2_257x48_q1": (257, 48, 1, "l2", "mixture", 12, 0.05),           # one row past a tile, d < 64
    "l2_5000x100_q70": (5000, 100, 70, "l2", "mixture", 13, 0.005),    # d not a multiple of 16
    "l2_3000x768_q40": (3000, 768, 40, "l2", "mixture:300", 14, 0.005),   # 32-deep stride
    "l2_3000x1968_q40": (3000, 1968, 40, "l2", "concat", 15, 0.005),   # concat rows, stride 16 mod 32
    "ip_1000x96_q33": (1000, 96, 33, "ip", "mixture", 16, 0.01),
    "ip_3000x768_q40": (3000, 768, 40, "ip", "mixture", 17, 0.005),
    "cosine_1000x96_q33": (1000, 96, 33, "cosine", "mixture", 18, 0.01),
    "cosine_3000x768_q40": (3000, 768, 40, "cosine", "mixture", 19, 0.005),
    "l2_700x96_q5_all": (700, 96, 5, "l2", "mixture", 20, None),       # radius = inf
}


def _normalize64(x):
    n = np.sqrt((x * x).sum(1, keepdims=True))
    return np.where(n > 0, x / np.where(n > 0, n, 1.0), x)


def exact_keys(xb, xq, metric):
    """float64 squared L2 distance (clamped at 0) or inner product of every (query, row) pair."""
    x = np.asarray(xb, dtype=np.float64)
    q = np.asarray(xq, dtype=np.float64)
    if metric == "cosine":
        x, q = _normalize64(x), _normalize64(q)
    ip = q @ x.T
    if metric != "l2":
        return ip
    return np.maximum((q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * ip, 0.0)


def make_data(name):
    """(xb, xq) of a case: rows and queries are disjoint draws of one mixture (queries fall into
    the rows' clusters); the concat layout gets L2-normalised queries, as the reference's CLI."""
    N, d, nq, metric, data, seed, _ = CASES[name]
    if data == "concat":
        assert d == 1968
        allx = concat_rows(N + nq, seed=seed)
        xq = allx[N:].astype(np.float64)
        xq = (xq / np.linalg.norm(xq, axis=1, keepdims=True)).astype(np.float32)
    else:
        centres = int(data.split(":")[1]) if ":" in data else 20
        allx = mixture(N + nq, d, centres=centres, seed=seed)
        xq = allx[N:].copy()
    return np.ascontiguousarray(allx[:N]), np.ascontiguousarray(xq)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(xb, xq, radius, metric, d64, b) of a table entry, computed once per process."""
    metric, quantile = CASES[name][3], CASES[name][6]
    xb, xq = make_data(name)
    d64 = exact_keys(xb, xq, metric)
    b = fp32_error_bound(xb, xq, metric)
    if quantile is None:
        radius = float("inf") if metric == "l2" else float("-inf")
    else:
        radius = float(np.float32(np.quantile(d64, quantile if metric == "l2" else 1.0 - quantile)))
    for a in (xb, xq, d64, b):
        a.setflags(write=False)
    return xb, xq, radius, metric, d64, b


def _inside(d64, radius, metric):
    return d64 < radius if metric == "l2" else d64 > radius


def range_conditions(xb, xq, radius, metric, d64=None, b=None):
    """(band, expected) from the oracle alone."""
    d64 = exact_keys(xb, xq, metric) if d64 is None else d64
    b = fp32_error_bound(xb, xq, metric) if b is None else b
    with np.errstate(invalid="ignore"):
        band = int((np.abs(d64 - radius) <= b).sum()) if np.isfinite(radius) else 0
    return band, int(_inside(d64, radius, metric).sum())


def assert_conditions(band, expected, nq):
    assert band <= BAND_FRAC * expected, (band, expected)
    assert expected >= MIN_HITS * nq, (expected, nq)


def check_range(lims, D, I, xb, xq, radius, metric, d64=None, b=None):
    lims, D, I = np.asarray(lims), np.asarray(D), np.asarray(I)
    nq, n = xq.shape[0], xb.shape[0]
    d64 = exact_keys(xb, xq, metric) if d64 is None else d64
    b = fp32_error_bound(xb, xq, metric) if b is None else b
    band, expected = range_conditions(xb, xq, radius, metric, d64, b)
    # (a)
    assert lims.dtype == np.int64 and D.dtype == np.float32 and I.dtype == np.int64
    assert lims.shape == (nq + 1,) and lims[0] == 0, lims[:4]
    assert (np.diff(lims) >= 0).all(), "lims not monotone"
    assert lims[-1] == len(D) == len(I), (lims[-1], len(D), len(I))
    tol = b * 1.0001 + 1e-30
    r32 = np.float32(radius)
    for q in range(nq):
        ids, dq = I[lims[q]:lims[q + 1]], D[lims[q]:lims[q + 1]]
        assert ((ids >= 0) & (ids < n)).all(), (q, ids)
        assert len(np.unique(ids)) == len(ids), f"duplicate labels for query {q}"
        # (b)
        assert (dq < r32).all() if metric == "l2" else (dq > r32).all(), (q, dq, radius)
        # (c)
        assert (np.abs(dq.astype(np.float64) - d64[q, ids]) <= tol[q, ids]).all(), \
            (q, np.abs(dq - d64[q, ids]).max())
        # (d)
        got = np.zeros(n, dtype=bool)
        got[ids] = True
        if metric == "l2":
            must, never = d64[q] < radius - tol[q], d64[q] > radius + tol[q]
        else:
            must, never = d64[q] > radius + tol[q], d64[q] < radius - tol[q]
        assert got[must].all(), (q, "missing", np.nonzero(must & ~got)[0][:8])
        assert not got[never].any(), (q, "extra", np.nonzero(never & got)[0][:8])
        # (e) best first, exact ties by the smaller label
        key = dq if metric == "l2" else -dq
        order = np.lexsort((ids, key))
        assert (order == np.arange(len(ids))).all(), (q, "segment not sorted by (D, label)")
    return band, expected


def oracle_result(xb, xq, radius, metric, d64=None):
    """A correct result built from float64 (keys rounded to float32): what the planted-fault
    tests corrupt."""
    d64 = exact_keys(xb, xq, metric) if d64 is None else d64
    d32 = d64.astype(np.float32)
    r32 = np.float32(radius)
    lims, Ds, Is = [0], [], []
    for q in range(xq.shape[0]):
        ids = np.nonzero(d32[q] < r32 if metric == "l2" else d32[q] > r32)[0]
        key = d32[q, ids] if metric == "l2" else -d32[q, ids]
        ids = ids[np.lexsort((ids, key))]
        Ds.append(d32[q, ids])
        Is.append(ids.astype(np.int64))
        lims.append(lims[-1] + len(ids))
    return (np.asarray(lims, dtype=np.int64), np.concatenate(Ds).astype(np.float32),
            np.concatenate(Is).astype(np.int64))
