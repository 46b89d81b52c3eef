"""Expected values of the IVF-PQ kernels (include/imgrec_ivfpq.h, csrc/ivfpq.hip) in plain numpy, and
the shared inputs of their tests.  Used by tests/test_ivfpq_check_cpu.py (the checker itself: it holds
for correct arithmetic with margin, and every planted mistake moves it), tests/test_ivfpq_kernels_gpu.py
(the kernels through the C ABI) and tests/test_ivfpq_gpu.py (the Python class).  No GPU use.

* expected_scan: the scan is specified exactly — a row's distance is the fp32 sum over j ascending of
  lut[q * nprobe + p][j][code_j], rows rank by (distance bits, label), the first k are kept, then
  -1 / FLT_MAX — so the expected D and I are computed here bit for bit, with sequential np.float32
  additions and a lexsort.  Both scan routes are compared with it for equality; no tolerance.
* lut_bound: the float64 table and the derived per-entry bound of the distance-table kernel.
* emulate_lut: the table kernel's arithmetic restated in numpy, for the CPU tests only.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

U = 2.0 ** -24
FLT_MAX = np.finfo(np.float32).max
LABEL_END = 1 << 31          # stored labels lie in [0, 2^31)

# (nr, m, dsub, ksub) of the distance-table tests
LUT_SHAPES = [
    (1, 1, 1, 1),
    (7, 3, 5, 255),             # nr % 8 != 0, ksub one short of a pass of the 256 threads
    (8, 2, 4, 256),
    (9, 2, 4, 257),             # a 1-row tail block, one centroid in a second pass
    (17, 48, 41, 4096),         # the reference's sub-quantiser, 1-row tail block
    (3, 2, 256, 64),            # the dsub limit
    (5, 2, 2, 65536),
]


# ---- distance tables --------------------------------------------------------------------------

def lut_inputs(nr, m, dsub, ksub, seed=0):
    """(resid (nr, m * dsub), cbt (m, dsub, ksub)) float32: standard normal residuals, codebooks
    scaled by 0.3 (the scales of tests/test_ivfpq_gpu.py)."""
    rng = np.random.default_rng([seed, nr, m, dsub, ksub])
    resid = rng.standard_normal((nr, m * dsub)).astype(np.float32)
    cbt = (0.3 * rng.standard_normal((m, dsub, ksub))).astype(np.float32)
    return resid, cbt


def lut_inputs_int(nr, m, dsub, ksub, seed=0):
    """Integer-valued inputs, |values| <= 8: every (r - c)^2 <= 256 and every table entry
    <= 256 * dsub < 2^24 is an integer fp32 holds exactly, so the kernel's table must EQUAL the
    float64 one."""
    rng = np.random.default_rng([seed, nr, m, dsub, ksub, 1])
    resid = rng.integers(-8, 9, (nr, m * dsub)).astype(np.float32)
    cbt = rng.integers(-8, 9, (m, dsub, ksub)).astype(np.float32)
    return resid, cbt


def lut_bound(resid, cbt):
    """(T64, bound), both (nr, m, ksub) float64: T64[r][j][i] = sum_t (resid[r][j*dsub + t] -
    cbt[j][t][i])^2 and the largest |lut - T64| a correct fp32 kernel can show.

    Derivation.  With u = 2^-24 and x_t = r_t - c_t (exact), the kernel computes
        df_t  = fl(r_t - c_t)               = x_t (1 + a_t),                 |a_t| <= u
        acc_t = fl(df_t * df_t + acc_{t-1}) = (df_t^2 + acc_{t-1}) (1 + e_t), |e_t| <= u   (one fma)
    for t = 0 .. dsub - 1 from acc_{-1} = 0, so
        lut = sum_t x_t^2 (1 + a_t)^2 prod_{s >= t} (1 + e_s).
    Term t carries 2 + (dsub - t) <= dsub + 2 factors (1 + delta), |delta| <= u; a multiply-add that
    is not fused rounds the product as well: dsub + 3 factors.  Every term x_t^2 is non-negative, so
    the factors cannot cancel and the error is relative to T64 itself (Higham, Accuracy and Stability
    of Numerical Algorithms, lemma 3.1):
        |lut - T64| <= gamma * T64,    gamma = n u / (1 - n u),  n = dsub + 3.
    Underflow: a subtraction or a sum that lands in the subnormal range is exact, and the fma does not
    round its product; an unfused product below 2^-126 loses at most 2^-150.  The floor of
    dsub * 2^-149 covers that with room.  T64 itself is off by at most (dsub + 2) 2^-53 T64, 2^-29 of
    the bound.
    """
    resid, cbt = np.asarray(resid, np.float64), np.asarray(cbt, np.float64)
    m, dsub, ksub = cbt.shape
    r = resid.reshape(resid.shape[0], m, dsub)
    T = np.zeros((r.shape[0], m, ksub))
    for t in range(dsub):
        T += (r[:, :, t, None] - cbt[None, :, t, :]) ** 2
    n = (dsub + 3) * U
    return T, n / (1.0 - n) * T + dsub * 2.0 ** -149


def lut_ratio(lut, resid, cbt):
    """max |lut - T64| / bound over the table (<= 1 passes); inf for a NaN or a wrong shape."""
    T, bound = lut_bound(resid, cbt)
    lut = np.asarray(lut)
    if lut.shape != T.shape or lut.dtype != np.float32 or not np.isfinite(lut).all():
        return float("inf")
    return float((np.abs(lut.astype(np.float64) - T) / bound).max())


def emulate_lut(resid, cbt, skip_t=None):
    """The table kernel's arithmetic in numpy: df = fl32(r - c); acc = fl32(acc + df * df) with the
    product exact (in float64), t ascending.  skip_t: a planted mistake, that term left out."""
    resid, cbt = np.asarray(resid, np.float32), np.asarray(cbt, np.float32)
    m, dsub, ksub = cbt.shape
    r = resid.reshape(resid.shape[0], m, dsub)
    acc = np.zeros((r.shape[0], m, ksub), np.float32)
    for t in range(dsub):
        if t == skip_t:
            continue
        df = (r[:, :, t, None] - cbt[None, :, t, :]).astype(np.float64)      # an fp32 difference
        acc = (acc.astype(np.float64) + df * df).astype(np.float32)
    return acc


# ---- the scan ---------------------------------------------------------------------------------

def ordered_bits(d):
    """uint32 whose unsigned order is the float order of the fp32 array d (wave_ops.h key_bits_ordered)."""
    b = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def probe_slots(probes, list_off):
    """(cnt, probe_off, seg_off, total) of ivfpq_scan_all_device, as IndexIVFPQ.search builds them:
    rows per (query, probe), its first slot, each query's first slot followed by total."""
    probes, list_off = np.asarray(probes, np.int64), np.asarray(list_off, np.int64)
    pr = probes.reshape(-1)
    l = np.maximum(pr, 0)
    cnt = np.where(pr >= 0, list_off[l + 1] - list_off[l], 0)
    probe_off = np.cumsum(cnt) - cnt
    total = int(cnt.sum())
    seg_off = np.concatenate([probe_off.reshape(probes.shape)[:, 0], [total]])
    return cnt, probe_off, seg_off, total


def expected_scan(lut, probes, list_off, codes, ids, k):
    """(D (nq, k) float32, I (nq, k) int64) of ivfpq_scan_device / ivfpq_scan_all_device, bit for bit.

    lut (nq * nprobe, m, ksub) float32, probes (nq, nprobe) int64 (-1: none), list_off (nlist + 1),
    codes (ntotal, m) integers < ksub, ids (ntotal,) int64.  Per query the rows of each probe >= 0, in
    probe order then list order; distance = fp32 sum over j ascending of lut[q * nprobe + p, j, code_j]
    from 0; rows ordered by (distance bits, label); the first k, then -1 / FLT_MAX.
    Vectorised over all (query, probe, row) entries."""
    lut = np.asarray(lut)
    assert lut.dtype == np.float32 and lut.ndim == 3
    probes, list_off = np.asarray(probes, np.int64), np.asarray(list_off, np.int64)
    codes, ids = np.asarray(codes).astype(np.int64), np.asarray(ids, np.int64)
    nq, nprobe = probes.shape
    m = lut.shape[1]
    assert lut.shape[0] == nq * nprobe and codes.shape == (ids.shape[0], m)
    cnt, probe_off, _, total = probe_slots(probes, list_off)
    D = np.full((nq, k), FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    if total == 0:
        return D, I
    qp = np.repeat(np.arange(nq * nprobe), cnt)                    # entry -> q * nprobe + p
    row = list_off[probes.reshape(-1)[qp]] + np.arange(total) - probe_off[qp]
    acc = np.zeros(total, np.float32)
    for j in range(m):
        acc = acc + lut[qp, j, codes[row, j]]                      # float32 + float32
    assert acc.dtype == np.float32
    lab, q = ids[row], qp // nprobe
    order = np.lexsort((lab, ordered_bits(acc), q))
    q, acc, lab = q[order], acc[order], lab[order]
    first = np.searchsorted(q, np.arange(nq))                      # each query's first sorted entry
    rank = np.arange(total) - first[q]
    keep = rank < k
    D[q[keep], rank[keep]] = acc[keep]
    I[q[keep], rank[keep]] = lab[keep]
    return D, I


SCAN_LIST_SIZES = (0, 1, 255, 256, 257, 1000, 0, 3, 512, 31, 33, 64)   # around the 256-lane round-robin
SCAN_KS = (1, 15, 16, 17, 31, 32)              # both sides of the KM = 16 / KM = 32 instantiations
SCAN_ALL_KS = SCAN_KS + (33, 100, 5000)        # 5000: above every query's entry count


def _labels(rng, n):
    """n distinct labels of [0, 2^31) in random (not monotone) order, 0 and 2^31 - 1 among them."""
    lab = np.unique(np.concatenate([rng.integers(1, LABEL_END - 1, 2 * n), [0, LABEL_END - 1]]))
    assert lab.size >= n
    lab = np.concatenate([[0, LABEL_END - 1], rng.permutation(lab[1:-1])[:n - 2]])
    return rng.permutation(lab).astype(np.int64)


@lru_cache(maxsize=None)
def scan_case(table):
    """The shared scan geometry: 12 lists of SCAN_LIST_SIZES rows, m = 8, ksub = 64, 9 queries of 4
    probes drawn without repetition, some of them -1, query 7 with every probe -1, query 8 probing
    only the two empty lists; table "random" (uniform in [0, 4)) or "ties" (entries in {0, 1, 2}: 17
    possible distances for up to 2025 rows, so hundreds rank by label alone).  Read-only arrays."""
    rng = np.random.default_rng(31)
    m, ksub, nq, nprobe = 8, 64, 9, 4
    sizes = np.array(SCAN_LIST_SIZES)
    list_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(sizes.sum())
    codes = rng.integers(0, ksub, (n, m)).astype(np.uint16)
    ids = _labels(rng, n)
    probes = np.stack([rng.permutation(len(sizes))[:nprobe] for _ in range(nq)]).astype(np.int64)
    probes[0] = [5, 3, 4, 2]                    # the four largest lists: 1000 + 256 + 257 + 255 rows
    probes[1, 0] = probes[2, 3] = probes[3, 1] = probes[3, 2] = -1
    probes[7] = -1
    probes[8] = [0, -1, 6, -1]
    if table == "random":
        lut = (4.0 * rng.random((nq * nprobe, m, ksub))).astype(np.float32)
    else:
        assert table == "ties"
        lut = rng.integers(0, 3, (nq * nprobe, m, ksub)).astype(np.float32)
    case = dict(lut=lut, probes=probes, list_off=list_off, codes=codes, ids=ids, m=m, ksub=ksub)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@lru_cache(maxsize=None)
def scan_case_wide():
    """The reference's code shape (m = 48, ksub = 4096: table rows 16 KiB apart): two lists of 300 and
    700 rows, 3 queries of 2 probes."""
    rng = np.random.default_rng(32)
    m, ksub, nq, nprobe = 48, 4096, 3, 2
    list_off = np.array([0, 300, 1000], np.int64)
    codes = rng.integers(0, ksub, (1000, m)).astype(np.uint16)
    probes = np.array([[0, 1], [1, 0], [1, -1]], np.int64)
    lut = (4.0 * rng.random((nq * nprobe, m, ksub))).astype(np.float32)
    return dict(lut=lut, probes=probes, list_off=list_off, codes=codes, ids=_labels(rng, 1000), m=m, ksub=ksub)


@lru_cache(maxsize=None)
def scan_case_slices():
    """65539 queries (the sort route writes D / I in slices of 65535 queries) at m = 1, ksub = 2, one
    probe each, cycling over lists of 0, 5 and 40 rows."""
    rng = np.random.default_rng(33)
    nq = 65539
    list_off = np.array([0, 0, 5, 45], np.int64)
    codes = rng.integers(0, 2, (45, 1)).astype(np.uint16)
    probes = (np.arange(nq, dtype=np.int64) % 3).reshape(nq, 1)
    lut = (4.0 * rng.random((nq, 1, 2))).astype(np.float32)
    return dict(lut=lut, probes=probes, list_off=list_off, codes=codes, ids=_labels(rng, 45), m=1, ksub=2)


# ---- cases of the Python class (tests/test_ivfpq_gpu.py) -------------------------------------------

@dataclass(frozen=True)
class PyCase:
    name: str
    d: int
    nlist: int
    m: int
    nbits: int
    n: int
    nq: int
    nprobe: int
    ks: tuple
    seed: int


PY_CASES = [
    PyCase("nbits16", 8, 4, 2, 16, 3000, 16, 2, (10,), 41),          # codes >= 32768 in an int16 tensor
    PyCase("probe_all", 32, 40, 8, 6, 3000, 12, 40, (10, 50), 44),   # nprobe = nlist = 40 > 32
    PyCase("chunks", 32, 16, 8, 8, 4000, 23, 3, (10, 40), 43),       # 23 queries in table chunks of 5
]
PY_CASE = {c.name: c for c in PY_CASES}
CHECK_RTOL = 2e-5            # the window of test_ivfpq_gpu._check: 2e-5 * max(1, |D|)
MAX_SHARE = 0.01             # and the share of labels it may leave mismatched


@lru_cache(maxsize=None)
def py_case_data(name):
    """(cen, cb, lists, codes, ids, q) of a case, as test_ivfpq_gpu._random_index draws them: normal
    centroids, codebooks scaled by 0.3, random lists and codes (over the full code range, the
    extremes included), labels a random draw of [0, 10 n); queries around centroids.  Read-only."""
    cs = PY_CASE[name]
    rng = np.random.default_rng(cs.seed)
    ksub = 1 << cs.nbits
    cen = rng.standard_normal((cs.nlist, cs.d)).astype(np.float32)
    cb = (0.3 * rng.standard_normal((cs.m, ksub, cs.d // cs.m))).astype(np.float32)
    lists = rng.integers(0, cs.nlist, cs.n)
    codes = rng.integers(0, ksub, (cs.n, cs.m))
    codes[0], codes[1] = 0, ksub - 1
    ids = rng.permutation(10 * cs.n)[:cs.n].astype(np.int64)
    q = (cen[rng.integers(0, cs.nlist, cs.nq)] + 0.5 * rng.standard_normal((cs.nq, cs.d))).astype(np.float32)
    out = (cen, cb, lists, codes, ids, q)
    for v in out:
        v.setflags(write=False)
    return out


def near_tie_share(D):
    """Share of the ranks of D (nq, k + 1 float64 oracle distances; the last column only serves as
    rank k - 1's neighbour) that lie within CHECK_RTOL * max(1, |D|) of a neighbouring rank: the
    ranks that fp32 rounding may permute.  Padding (FLT_MAX) is no neighbour."""
    D = np.asarray(D, np.float64)
    real = D < float(FLT_MAX)
    close = (np.diff(D, axis=1) <= CHECK_RTOL * np.maximum(1.0, np.abs(D[:, :-1]))) & real[:, 1:]
    tied = np.zeros(D.shape, bool)
    tied[:, :-1] |= close
    tied[:, 1:] |= close
    return float(tied[:, :-1].mean())
