"""Acceptance rules of one Lloyd k-means step (include/imgrec_kmeans.h kmeans_step_device) and of the
empty-cluster split, against a numpy float64 restatement.  Used by tests/test_kmeans_cpu.py (the
checker itself, on an fp32 numpy step and on perturbed outputs) and tests/test_kmeans_gpu.py (the
HIP kernels).

The rules rest on one derived bound, the worst-case rounding of the GEMM form of a squared distance
in fp32 (d products and d + 2 additions per key, every partial sum at most (|x| + |c|)^2):

    E(x, c) = (d + 2) * 2^-24 * (|x| + |c|)^2

* assign: every point gets the float64 label (exact float64 ties, which only bitwise-equal centroid
  rows produce, go to the smallest id — always).  Exception: a point whose float64 gap between the
  best and the second-best distinct key is below E(x, c1) + E(x, c2); there the chosen centroid
  must lie within that margin of the best.  At most MAX_SHARE of a case's points may be such
  exceptions, or the case itself fails: it would test nothing.  Spherical: the same on -x.c.
* dist: |dist - D64(x, c_assigned)| <= E.
* counts: bincount of the step's own assign, exactly.
* new_centroids: against the float64 mean over the step's own assign, every coordinate within
  cnt * 2^-24 * mean_i |x_ij| (sequential summation of cnt terms, so any fixed order passes) plus
  one fp32 ulp of the mean (the division); an empty cluster's row is the old row, byte for byte.
* obj: numpy's float64 sum of the step's own fp32 dist within n * 2^-53 relative to sum |dist|
  (float64 summation of n terms in any order).
* split: see check_split.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests.datagen import mixture

U = 2.0 ** -24
MAX_SHARE = 0.01
EPS = np.float32(1.0 / 1024.0)
UP, DN = np.float32(1) + EPS, np.float32(1) - EPS


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    d: int
    k: int
    init: str            # "sample": k seeded rows of x; "iter": one float64 Lloyd iteration from them
    part: int = 0        # IMGREC_KMEANS_PART for the GPU run (0: the default)


CASES = [
    Case("sift128", 3000, 128, 256, "sample"),       # the reference's codebook shape, scaled down
    Case("concat1968", 1500, 1968, 37, "iter"),      # concat width; k no tile multiple; empty clusters
    Case("dreamsim768", 3000, 768, 300, "iter"),     # DreamSim width, two centroid tiles
    Case("manyk", 2000, 48, 1000, "sample"),         # k >> tile, clusters of a few members
    Case("parts", 4099, 16, 7, "sample", part=64),   # segments of up to ~1,000 members in parts of 64; ragged n
    Case("odd19", 1000, 19, 33, "sample"),           # odd d: scalar loads, padded depth
]
CASE = {c.name: c for c in CASES}


def dist64(x, c, spherical=False):
    """(n, k) float64 keys: squared L2 distance, or -x.c.  Bitwise-equal centroid rows get
    bitwise-equal columns (computed once per distinct row)."""
    cu, inv = np.unique(np.asarray(c), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    x64, c64 = np.asarray(x, np.float64), cu.astype(np.float64)
    ip = x64 @ c64.T
    if spherical:
        D = -ip
    else:
        D = (x64 * x64).sum(1)[:, None] + (c64 * c64).sum(1)[None, :] - 2.0 * ip
    return D[:, inv]


def err_bound(x, c):
    """E(x_i, c_j) for every pair, (n, k)."""
    d = x.shape[1]
    xn = np.linalg.norm(np.asarray(x, np.float64), axis=1)
    cn = np.linalg.norm(np.asarray(c, np.float64), axis=1)
    return (d + 2) * U * (xn[:, None] + cn[None, :]) ** 2


def step64(x, c, spherical=False):
    """One float64 Lloyd step: (assign, new centroids as float64, counts)."""
    a = dist64(x, c, spherical).argmin(1)
    k = c.shape[0]
    cnt = np.bincount(a, minlength=k)
    new = np.asarray(c, np.float64).copy()
    for j in np.nonzero(cnt)[0]:
        new[j] = np.asarray(x[a == j], np.float64).mean(0)
    return a, new, cnt


@lru_cache(maxsize=None)
def case_data(name):
    """(x, centroids) of a case, float32, read-only."""
    cs = CASE[name]
    x = mixture(cs.n, cs.d, centres=20, seed=7)
    rows = np.random.default_rng(11).choice(cs.n, cs.k, replace=False)
    c = np.ascontiguousarray(x[rows])
    if cs.init == "iter":
        c = step64(x, c)[1].astype(np.float32)
    x.setflags(write=False)
    c.setflags(write=False)
    return x, c


def margins(x, c, spherical=False):
    """Per point: (best id, exception flag, margin, D) of the float64 oracle."""
    D = dist64(x, c, spherical)
    E = err_bound(x, c)
    n = D.shape[0]
    rows = np.arange(n)
    best = D.argmin(1)                       # first minimum: the smallest id of an exact tie
    d1 = D[rows, best]
    D2 = np.where(D == d1[:, None], np.inf, D)      # the second-best DISTINCT key
    second = D2.argmin(1)
    d2 = D2[rows, second]
    margin = E[rows, best] + E[rows, second]
    exc = (d2 - d1) < margin
    return best, exc, margin, D


def exception_share(x, c, spherical=False):
    return float(margins(x, c, spherical)[1].mean())


def check_assign(x, c, assign, spherical=False):
    """Returns the case's exception share; raises AssertionError on a violation."""
    assign = np.asarray(assign).astype(np.int64)
    n, k = x.shape[0], c.shape[0]
    assert assign.shape == (n,), f"assign has shape {assign.shape}"
    assert ((assign >= 0) & (assign < k)).all(), "assign out of range"
    best, exc, margin, D = margins(x, c, spherical)
    share = float(exc.mean())
    assert share <= MAX_SHARE, f"{share:.2%} of the points lie within the fp32 margin: the case tests nothing"
    rows = np.arange(n)
    da = D[rows, assign]
    # an exact float64 tie (bitwise-equal rows) must go to the smallest id
    first_equal = (D == da[:, None]).argmax(1)
    bad = np.nonzero(first_equal != assign)[0]
    assert bad.size == 0, (f"{bad.size} points given to the larger id of an exact tie, e.g. point {bad[0]}: "
                           f"{assign[bad[0]]} instead of {first_equal[bad[0]]}")
    wrong = np.nonzero(~exc & (assign != best))[0]
    assert wrong.size == 0, (f"{wrong.size} clear points mislabelled, e.g. point {wrong[0]}: "
                             f"{assign[wrong[0]]} instead of {best[wrong[0]]}")
    far = np.nonzero(exc & (da - D[rows, best] > margin))[0]
    assert far.size == 0, f"{far.size} near-tie points given a centroid outside the margin, e.g. {far[0]}"
    return share


def check_dist(x, c, assign, dist, spherical=False):
    assign = np.asarray(assign).astype(np.int64)
    x64, ca = np.asarray(x, np.float64), np.asarray(c, np.float64)[assign]
    ref = (x64 * ca).sum(1) if spherical else ((x64 - ca) ** 2).sum(1)
    d = x.shape[1]
    E = (d + 2) * U * (np.linalg.norm(x64, axis=1) + np.linalg.norm(ca, axis=1)) ** 2
    err = np.abs(np.asarray(dist, np.float64) - ref)
    bad = np.nonzero(~(err <= E))[0]
    assert bad.size == 0, f"{bad.size} distances off, worst {err.max():.3e} at bound {E[err.argmax()]:.3e}"


def check_counts(assign, counts, k):
    np.testing.assert_array_equal(np.asarray(counts).astype(np.int64),
                                  np.bincount(np.asarray(assign).astype(np.int64), minlength=k))


def check_centroids(x, c_old, assign, new):
    assign = np.asarray(assign).astype(np.int64)
    k = c_old.shape[0]
    new = np.asarray(new)
    assert new.dtype == np.float32 and new.shape == c_old.shape
    cnt = np.bincount(assign, minlength=k)
    x64 = np.asarray(x, np.float64)
    for j in range(k):
        if cnt[j] == 0:
            assert new[j].tobytes() == np.asarray(c_old[j], np.float32).tobytes(), \
                f"empty cluster {j}: the old row was not copied through"
            continue
        m = x64[assign == j]
        mean = m.mean(0)
        tol = cnt[j] * U * np.abs(m).mean(0) + np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
        err = np.abs(new[j].astype(np.float64) - mean)
        assert (err <= tol).all(), (f"cluster {j} ({cnt[j]} members): coordinate {err.argmax()} off by "
                                    f"{err.max():.3e}, bound {tol[err.argmax()]:.3e}")


def check_obj(dist, obj):
    d = np.asarray(dist, np.float32).astype(np.float64)
    ref, scale = d.sum(), np.abs(d).sum()
    assert abs(float(obj) - ref) <= d.size * 2.0 ** -53 * scale, f"objective {obj!r} vs {ref!r}"


def check_step(x, c, out, spherical=False):
    """out = (assign, dist, new_centroids, counts, obj).  Returns the exception share."""
    assign, dist, new, counts, obj = out
    share = check_assign(x, c, assign, spherical)
    check_dist(x, c, assign, dist, spherical)
    check_counts(assign, counts, c.shape[0])
    check_centroids(x, c, assign, new)
    check_obj(dist, obj)
    return share


def split_rows(row):
    """(the empty cluster's new row, the donor's new row) from the donor's row, faiss's pattern:
    even columns of the new row times 1 + EPS, odd ones times 1 - EPS, the donor the opposite."""
    row = np.asarray(row, np.float32)
    even = np.arange(row.size) % 2 == 0
    return (row * np.where(even, UP, DN)).astype(np.float32), (row * np.where(even, DN, UP)).astype(np.float32)


def check_split(old, old_counts, new):
    """Every previously empty cluster ci (ascending, as the repair walks them) has a donor cj whose
    count at that moment is > 1, row ci is byte-equal to the donor's row in the (1 +- EPS) pattern and
    the donor's row takes the opposite pattern; every other row is byte-equal to before.  The draw
    itself is not compared.  (A repaired cluster that donates again later in the same call is not
    recognised: rows are matched against the final state.)  Returns the (ci, cj) pairs."""
    old, new = np.asarray(old, np.float32), np.asarray(new, np.float32)
    cnt = np.asarray(old_counts).astype(np.int64).copy()
    state = old.copy()
    pairs = []
    for ci in np.nonzero(cnt == 0)[0]:
        donor = None
        for cj in np.nonzero(cnt > 1)[0]:
            ri, _ = split_rows(state[cj])
            if ri.tobytes() == new[ci].tobytes():
                donor = int(cj)
                break
        assert donor is not None, f"empty cluster {ci}: no donor row reproduces it in the split pattern"
        state[ci], state[donor] = split_rows(state[donor])
        cnt[ci] = cnt[donor] // 2
        cnt[donor] -= cnt[ci]
        pairs.append((int(ci), donor))
    bad = [j for j in range(old.shape[0]) if state[j].tobytes() != new[j].tobytes()]
    assert not bad, f"rows {bad[:8]} differ from the split rule's result"
    return pairs


def step32(x, c, spherical=False):
    """An fp32 numpy step in the GEMM form (what a correct fp32 implementation computes):
    (assign, dist, new_centroids, counts, obj)."""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    ip = x @ c.T
    key = -ip if spherical else (c * c).sum(1, dtype=np.float32)[None, :] - np.float32(2) * ip
    a = key.argmin(1).astype(np.int32)
    ca = c[a]
    dist = (x * ca).sum(1, dtype=np.float32) if spherical else ((x - ca) ** 2).sum(1, dtype=np.float32)
    k = c.shape[0]
    cnt = np.bincount(a, minlength=k).astype(np.int64)
    new = c.copy()
    for j in np.nonzero(cnt)[0]:
        new[j] = x[a == j].sum(0, dtype=np.float32) / np.float32(cnt[j])
    return a, dist, new, cnt, float(dist.astype(np.float64).sum())
