"""Checker and parameter table of the filtered-search tests (test helper).

check_filtered(D, I, xb, xq, mask, k, metric) checks a search restricted to the rows `mask`
selects: every returned label is selected, and with the labels mapped to ranks in xb[mask] the
result passes tests.knn_check.check_knn against the float64 oracle of the sub-corpus xb[mask]
(rigorous window, then the empirical one: tight stays on) with at least 0.6 of the ranks
label-checked.  The 0.6 is a condition on the cases, not a measurement of the kernel:
tests/test_filter_cpu.py proves it for every table entry by running the float64 oracle's own
result, rounded to fp32, through this checker.

CASES is the one table both test files use.  A case's data is tests.datagen.mixture(N + nq, d,
centres=20, seed=seed) — rows are the first N, queries the rest — except the 1968-wide concat
layout, built as tests.range_check.make_data builds it (L2-normalised queries).  Its mask is
np.random.default_rng(seed + 100).random(N) < frac with the last row forced selected.
"""
import functools

import numpy as np

from oracle.flat_knn import search_exact
from tests.datagen import concat_rows, mixture
from tests.knn_check import check_knn

MIN_EXACT_FRAC = 0.6

# name: (N, d, nq, metric, data, seed, frac, k)                       what it can break
CASES = {
    "a": (1000, 96, 33, "l2", "mixture", 31, 0.5, 10),      # partial last gathered tile; partial query block; 128 x 128
    "b": (257, 48, 1, "l2", "mixture", 32, 0.9, 5),         # one row past a corpus tile; d < 64; 256 x 32
    "c": (5000, 100, 70, "l2", "mixture", 33, 0.03, 10),    # fewer selected than one tile; d not a multiple of 16
    "d": (3000, 768, 40, "cosine", "mixture", 34, 0.3, 32),  # 32-deep stride; km = 32
    "e": (3000, 1968, 40, "l2", "concat", 35, 0.5, 10),     # stride 16 mod 32
    "f": (1000, 96, 33, "ip", "mixture", 36, 0.1, 16),      # inner product sign
    "g": (2000, 96, 9, "l2", "mixture", 37, 0.4, 100),      # the any-k sort route
    "h": (3000, 768, 300, "l2", "mixture", 38, 0.5, 10),    # several query blocks x several row splits
}


def make_mask(N, seed, frac):
    mask = np.random.default_rng(seed + 100).random(N) < frac
    mask[N - 1] = True
    return mask


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(xb, xq, mask, k, metric) of a table entry, computed once per process, read-only."""
    N, d, nq, metric, data, seed, frac, k = CASES[name]
    if data == "concat":
        assert d == 1968
        allx = concat_rows(N + nq, seed=seed)
        xq = allx[N:].astype(np.float64)
        xq = (xq / np.linalg.norm(xq, axis=1, keepdims=True)).astype(np.float32)
    else:
        allx = mixture(N + nq, d, centres=20, seed=seed)
        xq = allx[N:].copy()
    xb = np.ascontiguousarray(allx[:N])
    xq = np.ascontiguousarray(xq)
    mask = make_mask(N, seed, frac)
    for a in (xb, xq, mask):
        a.setflags(write=False)
    return xb, xq, mask, k, metric


def labels_to_ranks(I, mask):
    """Labels of the full corpus -> ranks in xb[mask] (-1 kept); every label must be selected."""
    I = np.asarray(I)
    real = I >= 0
    assert (I[real] < mask.shape[0]).all(), "label past ntotal"
    assert mask[I[real]].all(), ("unselected label returned", I[real][~mask[I[real]]][:8])
    rank = np.cumsum(mask) - 1
    out = np.full(I.shape, -1, dtype=np.int64)
    out[real] = rank[I[real]]
    return out


def check_filtered(D, I, xb, xq, mask, k, metric):
    mask = np.asarray(mask, dtype=bool)
    I_sub = labels_to_ranks(I, mask)
    return check_knn(D, I_sub, np.ascontiguousarray(xb[mask]), xq, k, metric,
                     min_exact_frac=MIN_EXACT_FRAC)


def oracle_filtered(xb, xq, mask, k, metric):
    """The float64 oracle's filtered result in the library's conventions: keys rounded to fp32,
    labels of the full corpus, -1 / +-FLT_MAX past the selected count."""
    sel = np.nonzero(mask)[0]
    Dg, Ig = search_exact(np.ascontiguousarray(xb[mask]), xq, k, metric)
    real = Ig >= 0
    I = np.full(Ig.shape, -1, dtype=np.int64)
    I[real] = sel[Ig[real]]
    pad = np.finfo(np.float32).max * (1 if metric == "l2" else -1)
    D = np.where(real, Dg, pad).astype(np.float32)
    return D, I
