"""Helpers of the remove_ids tests: the removal patterns and what must be left (test helper).

A pattern is a bool mask over the N stored rows, True = removed.  `CHUNK` is the bounce chunk the
GPU tests force (IMGREC_REMOVE_CHUNK), so that every shape moves its rows in several chunks and the
"straddle" block crosses a chunk boundary of the destination rows.
"""
import numpy as np

CHUNK = 96

PATTERNS = ("none", "all", "first", "last", "alternate", "all_but_one", "straddle", "random30")


def pattern(name: str, n: int, chunk: int = CHUNK) -> np.ndarray:
    m = np.zeros(n, dtype=bool)
    if name == "none":
        pass
    elif name == "all":
        m[:] = True
    elif name == "first":
        m[0] = True
    elif name == "last":
        m[n - 1] = True
    elif name == "alternate":
        m[::2] = True
    elif name == "all_but_one":
        m[:] = True
        m[n // 3] = False
    elif name == "straddle":
        # one contiguous block; the first moved row is row 10, so the destination chunks are
        # [10, 10 + chunk), ...: a block of chunk + 40 rows from row 30 on makes the sources of the
        # first chunk and of the next ones overlap their own destinations across a chunk boundary
        m[30:30 + chunk + 40] = True
        m[10] = True
    elif name == "random30":
        m = np.random.default_rng(1234 + n).random(n) < 0.3
    else:
        raise KeyError(name)
    return m


def keep_of(mask: np.ndarray) -> np.ndarray:
    """keep = ~mask."""
    return ~np.asarray(mask, dtype=bool)


def survivors(xb: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """The rows a fresh index of the survivors is built from, in their order."""
    return np.ascontiguousarray(xb[keep_of(mask)])


def bitmap(mask) -> np.ndarray:
    return np.packbits(np.asarray(mask, dtype=bool), bitorder="little")
