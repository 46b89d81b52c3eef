"""Acceptance rules of the soft-VLAD encoding (include/imgrec_vlad.h vlad_encode_device) against a
numpy float64 restatement.  Used by tests/test_vlad_cpu.py (the checker itself, on an fp32 numpy
encoding and on perturbed outputs) and tests/test_vlad_gpu.py (the HIP kernels).

U = 2^-24 and E(x, c) = (d + 2) U (|x| + |c|)^2 are kmeans_check's: the worst-case rounding of the
GEMM form of a squared distance in fp32.

* neighbours (check_neighbours).  Per descriptor the float64 distances are ranked by (distance, id);
  bitwise-equal codebook rows have equal float64 distances (kmeans_check.dist64), so among them the
  smaller id ranks first.  The returned ids are distinct and in range.  The returned SET equals the
  float64 top-nn.  Exception (needs k > nn): a descriptor whose float64 gap between the rank-nn
  distance and the next DISTINCT distance is below E_nn + E_next; there every returned id must lie
  within that margin of the rank-nn distance.  At most MAX_SHARE of a case's descriptors may be
  such exceptions, or the case itself fails.  Along every list the float64 distances are
  non-decreasing within E_a + E_b of adjacent entries.  Of a group of bitwise-equal codebook rows
  the ids present in a list are the group's smallest, in ascending order — always.
* distances (check_dist): |nn_dist - D64| <= E, and nn_dist >= 0.
* raw accumulator (check_raw), against float64 over the encoding's OWN nn_idx and nn_dist, with
  w64 = exp(-nn_dist / (2 sigma^2)) (sigma the fp32 value, the rest float64).  Per coordinate c of
  row i of an image, with m the descriptors j of that image that list i and a the largest
  |nn_dist / (2 sigma^2)| among them:

      |raw - sum_j w_j (x_jc - C_ic)| <= (m + 5 + 2a) U sum_j w_j (|x_jc| + |C_ic|)

  Derivation, first order in U, every term relative to sum_j w_j (|x_jc| + |C_ic|):
    2a      the weight's argument: 2 sigma^2 rounded to fp32 and one fp32 division, each U relative,
            so the argument moves by at most 2aU and exp of it by the same relative amount;
    2       expf, within one ulp = 2U;
    1       the rounding of x - C (residual form), or of the final (sum w x) - (sum w) C (factored
            form: its result is at most the sum of magnitudes above);
    1       the product w * (x - C), w * x or (sum w) * C where it is not fused into the addition;
    m       the summation: m - 1 additions in any order (sequential is the worst case; a tree is
            smaller); in the factored form both sums have m terms, and each is bounded by its part
            of the magnitude sum, so together they still take m;
    1       slack for the second-order terms dropped above (they are O((m + 2a)^2 U^2): below U
            while m + 2a < 4096, which every case here satisfies).
  So the bound covers sequential or tree summation of either algebraic form.  A codebook row that no
  descriptor of the image lists is exactly 0.
* final output (check_final), against the float64 epilogue applied to the encoding's own raw output
  (a second run with VLAD_RAW): relative error per element <= 8 U.  Derivation for an fp32
  epilogue whose two norms are accumulated in float64: the row norm rounded to fp32 (U), v / r (U),
  the square root halves what came in and adds its own (U + U = 2U so far), the global norm of
  values that are 2U off is 2U off plus its own rounding (3U), the last division adds both and
  rounds (2U + 3U + U = 6U); 8U leaves two for second-order terms.  Zero rows stay exactly zero; an
  empty image's vector is exactly zero.

Data.  RootSIFT of tests.datagen.mixture is too clumped for this check (at d = 128, k = 256,
nn = 4, 2.1 % of the descriptors fall within the margin), so the descriptors come from a sparser
generator (descriptors(), below): 40 sparse gamma prototypes, a per-descriptor gamma modulation,
sparse gamma noise, then RootSIFT.  The codebook is k rows of x drawn by default_rng(11).choice,
then one float64 Lloyd iteration (kmeans_check.step64).
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from image_recommender_amd.vlad import rootsift
from tests import kmeans_check as kc

U = kc.U
MAX_SHARE = 0.01
SIFT_SIZES = (0, 1, 3, 64, 65, 300, 0, 1000)     # empty images first and in the middle, a tile edge, nfeatures


@dataclass(frozen=True)
class Case:
    name: str
    d: int
    k: int
    nn: int
    sizes: tuple            # descriptors per image
    sigma: float = 125.0    # the reference's
    dup: tuple = ()         # (dst, src): codebook row dst := row src


CASES = [
    Case("sift", 128, 256, 4, SIFT_SIZES),                       # the reference's shape
    Case("sift_sharp", 128, 256, 4, SIFT_SIZES, sigma=0.5),      # weights far from 1: a wrong weight shows
    Case("k300", 48, 300, 4, (200, 0, 129, 71)),                 # more than one codebook tile
    Case("odd19", 19, 33, 4, (37, 0, 100, 1, 0)),                # odd d: scalar loads, padded depth; empty last
    Case("few5", 128, 5, 4, (50, 3, 0, 77)),                     # k barely above nn
    Case("all4", 32, 4, 4, (9, 0, 70)),                          # k = nn: every row is listed
    Case("hard", 64, 40, 1, (100, 0, 33)),                       # nn = 1: plain VLAD
    Case("nn8", 128, 256, 8, SIFT_SIZES),                        # the largest list
    Case("dup", 128, 256, 4, SIFT_SIZES, dup=(9, 5)),            # two bitwise-equal codebook rows
]
CASE = {c.name: c for c in CASES}


def descriptors(n, d, seed=7):
    """(n, d) float32 RootSIFT-like rows; all draws from one default_rng(seed), in this order."""
    rng = np.random.default_rng(seed)
    proto = rng.gamma(0.6, 1.0, (40, d)) * (rng.uniform(size=(40, d)) < 0.35)
    label = rng.integers(0, 40, n)
    a = proto[label] * rng.gamma(4.0, 0.25, (n, d)) \
        + 0.05 * rng.gamma(0.5, 1.0, (n, d)) * (rng.uniform(size=(n, d)) < 0.2)
    return np.ascontiguousarray(rootsift(a))


@lru_cache(maxsize=None)
def _base(n, d, k):
    x = descriptors(n, d)
    rows = np.random.default_rng(11).choice(n, k, replace=False)
    c = kc.step64(x, np.ascontiguousarray(x[rows]))[1].astype(np.float32)
    x.setflags(write=False)
    c.setflags(write=False)
    return x, c


@lru_cache(maxsize=None)
def case_data(name):
    """(x (N, d), offsets int64[nimg + 1], codebook (k, d)) of a case, read-only."""
    cs = CASE[name]
    off = np.concatenate([[0], np.cumsum(cs.sizes)]).astype(np.int64)
    x, c = _base(int(off[-1]), cs.d, cs.k)
    if cs.dup:
        c = c.copy()
        c[cs.dup[0]] = c[cs.dup[1]]
        c.setflags(write=False)
    off.setflags(write=False)
    return x, off, c


def margins(x, c, nn):
    """Per descriptor: (float64 top-nn ids in rank order, exception flag, margin, rank-nn distance, D, E)."""
    D = kc.dist64(x, c)
    E = kc.err_bound(x, c)
    n, k = D.shape
    rows = np.arange(n)
    order = np.argsort(D, axis=1, kind="stable")         # equal distances (equal rows): ascending id
    top = order[:, :nn]
    last = top[:, nn - 1]
    d_last = D[rows, last]
    if k > nn:
        D2 = np.where(D <= d_last[:, None], np.inf, D)   # the next DISTINCT distance
        nxt = D2.argmin(1)
        d_next = D2[rows, nxt]
        margin = E[rows, last] + E[rows, nxt]
        exc = (d_next - d_last) < margin
    else:
        margin = np.zeros(n)
        exc = np.zeros(n, bool)
    return top, exc, margin, d_last, D, E


def exception_share(x, c, nn):
    return float(margins(x, c, nn)[1].mean()) if x.shape[0] else 0.0


def check_neighbours(x, c, nn, idx):
    """Returns (the exception share, the mask of clear descriptors); raises AssertionError on a violation."""
    n, k = x.shape[0], c.shape[0]
    idx = np.asarray(idx)
    assert idx.shape == (n, nn), f"nn_idx has shape {idx.shape}"
    idx = idx.astype(np.int64)
    assert ((idx >= 0) & (idx < k)).all(), "nn_idx out of range"
    if n == 0:
        return 0.0, np.zeros(0, bool)
    srt = np.sort(idx, axis=1)
    assert (np.diff(srt, axis=1) != 0).all(), "a list names a codebook row twice"
    top, exc, margin, d_last, D, E = margins(x, c, nn)
    share = float(exc.mean())
    assert share <= MAX_SHARE, f"{share:.2%} of the descriptors lie within the fp32 margin: the case tests nothing"
    rows = np.arange(n)
    # equal rows: the ids present are the group's smallest, ascending
    _, inv, cnt = np.unique(np.asarray(c), axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    for g in np.nonzero(cnt > 1)[0]:
        members = np.nonzero(inv == g)[0]                 # ascending ids
        pos = np.full((n, members.size), nn)
        for t, m in enumerate(members):
            hit = idx == m
            pos[hit.any(1), t] = hit.argmax(1)[hit.any(1)]
        bad = np.nonzero((np.diff(pos, axis=1) < 0).any(1) | ((pos[:, :-1] == nn) & (pos[:, 1:] < nn)).any(1))[0]
        assert bad.size == 0, (f"{bad.size} lists name the larger id of bitwise-equal rows {members.tolist()} first "
                               f"(or without the smaller), e.g. descriptor {bad[0]}: {idx[bad[0]].tolist()}")
    wrong = np.nonzero(~exc & (srt != np.sort(top, axis=1)).any(1))[0]
    assert wrong.size == 0, (f"{wrong.size} clear descriptors with a wrong neighbour set, e.g. descriptor {wrong[0]}: "
                             f"{idx[wrong[0]].tolist()} instead of {top[wrong[0]].tolist()}")
    Dl = D[rows[:, None], idx]
    far = np.nonzero(exc & (Dl > (d_last + margin)[:, None]).any(1))[0]
    assert far.size == 0, f"{far.size} near-tie descriptors list a row outside the margin, e.g. {far[0]}"
    El = E[rows[:, None], idx]
    if nn > 1:
        drop = Dl[:, :-1] - Dl[:, 1:] > El[:, :-1] + El[:, 1:]
        bad = np.nonzero(drop.any(1))[0]
        assert bad.size == 0, (f"{bad.size} lists are not best first, e.g. descriptor {bad[0]}: {idx[bad[0]].tolist()} "
                               f"at distances {Dl[bad[0]].tolist()}")
    return share, ~exc


def check_dist(x, c, idx, dist):
    idx = np.asarray(idx).astype(np.int64)
    dist = np.asarray(dist)
    assert dist.dtype == np.float32 and dist.shape == idx.shape
    if idx.size == 0:
        return
    D, E = kc.dist64(x, c), kc.err_bound(x, c)
    rows = np.arange(x.shape[0])[:, None]
    err = np.abs(dist.astype(np.float64) - D[rows, idx])
    bad = ~(err <= E[rows, idx])
    assert not bad.any(), f"{int(bad.sum())} distances off, worst {np.nanmax(err):.3e} at bound {E[rows, idx][bad].min():.3e}"
    assert (dist >= 0).all(), "a negative distance"


def image_of(off):
    """The image of every descriptor."""
    off = np.asarray(off)
    return np.repeat(np.arange(off.size - 1), np.diff(off))


def raw64(x, off, c, sigma, idx, dist):
    """(float64 raw accumulator (nimg, k, d), its bound (nimg, k, d), members (nimg, k)) over the given lists."""
    n, d = x.shape
    k, nimg = c.shape[0], len(off) - 1
    idx = np.asarray(idx).astype(np.int64)
    nn = idx.shape[1]
    s = float(np.float32(sigma))
    arg = np.asarray(dist, np.float64) / (2.0 * s * s)
    w = np.exp(-arg)
    key = (image_of(off)[:, None] * k + idx).ravel()
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    xr = np.repeat(x64, nn, axis=0)                        # entry (j, s) -> row j
    cr = c64[idx.ravel()]
    wv = w.ravel()[:, None]
    ref = np.zeros((nimg * k, d))
    mag = np.zeros((nimg * k, d))
    np.add.at(ref, key, wv * (xr - cr))
    np.add.at(mag, key, wv * (np.abs(xr) + np.abs(cr)))
    m = np.bincount(key, minlength=nimg * k).astype(np.float64)
    a = np.zeros(nimg * k)
    np.maximum.at(a, key, np.abs(arg).ravel())
    bound = ((m + 5.0 + 2.0 * a) * U)[:, None] * mag
    return ref.reshape(nimg, k, d), bound.reshape(nimg, k, d), m.reshape(nimg, k)


def check_raw(x, off, c, sigma, idx, dist, raw):
    k, d, nimg = c.shape[0], c.shape[1], len(off) - 1
    raw = np.asarray(raw)
    assert raw.dtype == np.float32 and raw.shape == (nimg, k * d), f"raw has shape {raw.shape}, dtype {raw.dtype}"
    raw = raw.reshape(nimg, k, d)
    ref, bound, m = raw64(x, off, c, sigma, idx, dist)
    unlisted = m == 0
    assert (raw[unlisted] == 0).all(), "a codebook row that no descriptor of the image lists is not exactly 0"
    err = np.abs(raw.astype(np.float64) - ref)
    bad = ~(err <= bound)
    if bad.any():
        i, r, col = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{int(bad.sum())} accumulator coordinates off, e.g. image {i} row {r} column {col}: "
                             f"{err[i, r, col]:.3e}, bound {bound[i, r, col]:.3e} ({int(m[i, r])} members)")


def final64(raw, k, d):
    """The float64 epilogue of (nimg, k * d) raw rows."""
    v = np.asarray(raw, np.float64).reshape(raw.shape[0], k, d)
    r = np.sqrt((v * v).sum(-1, keepdims=True))
    v = np.divide(v, r, out=np.zeros_like(v), where=r > 0)
    v = np.sign(v) * np.sqrt(np.abs(v))
    g = np.sqrt((v * v).sum((1, 2), keepdims=True))
    v = np.divide(v, g, out=np.zeros_like(v), where=g > 0)
    return v.reshape(raw.shape[0], k * d)


def check_final(raw, vlad, off, k, d):
    raw, vlad = np.asarray(raw), np.asarray(vlad)
    assert vlad.dtype == np.float32 and vlad.shape == raw.shape == (len(off) - 1, k * d)
    empty = np.diff(np.asarray(off)) == 0
    assert (vlad[empty] == 0).all(), "an image without descriptors has a nonzero vector"
    ref = final64(raw, k, d)
    zero_rows = ~(raw.reshape(-1, d) != 0).any(1)
    assert (vlad.reshape(-1, d)[zero_rows] == 0).all(), "a zero row did not stay zero"
    err = np.abs(vlad.astype(np.float64) - ref)
    bad = ~(err <= 8.0 * U * np.abs(ref))
    if bad.any():
        i, e = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{int(bad.sum())} output elements off, e.g. image {i} element {e}: {vlad[i, e]!r} vs "
                             f"{ref[i, e]!r} (relative {err[i, e] / max(abs(ref[i, e]), 1e-300):.3e}, bound {8 * U:.3e})")


def check_all(x, off, c, nn, sigma, out):
    """out = (vlad, raw, nn_idx, nn_dist).  Returns (the exception share, the mask of clear descriptors)."""
    vlad, raw, idx, dist = out
    share, clear = check_neighbours(x, c, nn, idx)
    check_dist(x, c, idx, dist)
    check_raw(x, off, c, sigma, idx, dist, raw)
    check_final(raw, vlad, off, c.shape[0], c.shape[1])
    return share, clear


# ---- an fp32 numpy encoding (what a correct fp32 implementation computes) ----------------------------
def neighbours32(x, c, nn):
    """(nn_idx, nn_dist): fp32 GEMM-form keys (equal rows share one column), ties to the smaller id."""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    cu, inv = np.unique(c, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    key = ((cu * cu).sum(1, dtype=np.float32)[None, :] - np.float32(2) * (x @ cu.T))[:, inv]
    idx = np.argsort(key, axis=1, kind="stable")[:, :nn].astype(np.int32)
    dist = ((x[:, None, :] - c[idx]) ** 2).sum(-1, dtype=np.float32)
    return idx, dist


def raw32(x, off, c, sigma, idx, dist, weight_factor=None):
    """The fp32 accumulator (nimg, k * d), members added in descriptor order.  weight_factor =
    (descriptor, slot, factor) scales that one weight (a defect for the checker to find)."""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    k, d, nimg = c.shape[0], c.shape[1], len(off) - 1
    t = np.float32(2.0 * float(np.float32(sigma)) ** 2)
    w = np.exp(-dist / t).astype(np.float32)
    if weight_factor is not None:
        w = w.copy()
        w[weight_factor[0], weight_factor[1]] *= np.float32(weight_factor[2])
    key = (image_of(off)[:, None] * k + idx.astype(np.int64)).ravel()
    raw = np.zeros((nimg * k, d), np.float32)
    np.add.at(raw, key, (w[:, :, None] * (x[:, None, :] - c[idx])).reshape(-1, d))
    return raw.reshape(nimg, k * d)


def final32(raw, k, d):
    v = np.asarray(raw, np.float32).reshape(raw.shape[0], k, d)
    r = np.sqrt((v.astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32)
    v = np.divide(v, r, out=np.zeros_like(v), where=r > 0)
    v = (np.sign(v) * np.sqrt(np.abs(v))).astype(np.float32)
    g = np.sqrt((v.astype(np.float64) ** 2).sum((1, 2), keepdims=True)).astype(np.float32)
    v = np.divide(v, g, out=np.zeros_like(v), where=g > 0)
    return v.reshape(raw.shape[0], k * d)


def encode32(x, off, c, nn, sigma):
    """(vlad, raw, nn_idx, nn_dist) in fp32 numpy."""
    idx, dist = neighbours32(x, c, nn)
    raw = raw32(x, off, c, sigma, idx, dist)
    return final32(raw, c.shape[0], c.shape[1]), raw, idx, dist
