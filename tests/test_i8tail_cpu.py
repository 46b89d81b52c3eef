"""The int8 tail of the 256 x 256 candidate kernel, on the CPU (DESIGN.md "int8 tail"): the numpy
restatement of its arithmetic and of its error bound e_ip (tests/i8tail_ref.py) must satisfy
|approximate q.x - float64 q.x| <= e_ip on random and on crafted inputs, every term of the bound
must be needed by at least one of them, and the split-column rule must give the values the design
states.
"""
import numpy as np
import pytest

from tests import i8tail_ref as R
from tests.datagen import concat_rows, mixture

D_, HEAD, DPB, DPT = 704, 64, 704, 640


def _errs(x, qs, head=HEAD, dpb=DPB, dpt=DPT, drop=None):
    """max over the queries of (|approx - exact| / e_ip) and whether every pair is inside."""
    mx = R.corpus_maxima(x, head, dpb, dpt)
    xn_max = float((x.astype(np.float64) ** 2).sum(1).max())
    worst = 0.0
    for q in qs:
        a = R.approx_ip(x, q, head, dpb, dpt).astype(np.float64)
        e = np.abs(a - x.astype(np.float64) @ q.astype(np.float64)).max()
        worst = max(worst, e / float(R.e_ip(q, head, dpb, dpt, mx, xn_max, drop=drop)))
    return worst


def _lead(x, f=6.0):
    x = x.copy()
    x[:, :48] *= np.float32(f)
    return x


@pytest.fixture(scope="module")
def rows():
    return _lead(mixture(400, D_, centres=8, seed=1, normalize=True))


@pytest.fixture(scope="module")
def queries():
    return _lead(mixture(6, D_, centres=8, seed=2, normalize=True))


def test_random_rows_and_queries(rows, queries):
    assert 0.0 < _errs(rows, queries) <= 1.0


def test_row_with_one_huge_tail_element(rows, queries):
    x = rows.copy()
    x[7, 300] = 50.0                    # its scale is 50 / 127: every other code of the row is 0
    x[8, 100] = -20.0
    assert _errs(x, queries) <= 1.0


def test_all_zero_tail(rows, queries):
    x = rows.copy()
    x[3, HEAD:] = 0.0
    codes, s = R.quantize_tail(x, HEAD, DPB, DPT)
    assert s[3] == 0.0 and not codes[3].any()
    assert _errs(x, queries) <= 1.0
    q = queries.copy()
    q[0, HEAD:] = 0.0                   # and a query without a tail
    assert _errs(x, q[:1]) <= 1.0


def test_query_with_all_mass_in_the_head(rows):
    q = np.zeros((2, D_), np.float32)
    q[0, :48] = np.linspace(0.1, 1.0, 48, dtype=np.float32)
    q[1, :64] = np.float32(1.0 / 3.0)
    assert _errs(rows, q) <= 1.0


def test_pad_columns_and_no_head():
    x = mixture(300, 760, centres=8, seed=3, normalize=True)      # dpb 768, H = 0, no pad needed
    q = mixture(3, 760, centres=8, seed=4, normalize=True)
    assert _errs(x, q, head=0, dpb=768, dpt=768) <= 1.0
    xl, ql = _lead(x), _lead(q)                                   # H = 64: 704 tail columns + 64 pad
    assert _errs(xl, ql, head=64, dpb=768, dpt=768) <= 1.0


# inputs on which one term carries the whole error: exactly representable on every other side
def _grid_tail(rng, n):
    """tails whose entries are whole multiples of max / 127 (the int8 codes are exact)"""
    c = rng.integers(-127, 128, (n, D_ - HEAD)).astype(np.float32)
    c[:, 0] = 127.0
    return c * np.float32(2.0 ** -9)


def _bf16_head(rng, n):
    return R.bf16_rne(rng.standard_normal((n, HEAD)).astype(np.float32))


@pytest.mark.parametrize("drop", ["qt_Rt", "dqt_Xt", "qh_Rh", "dqh_Xh", "acc"])
def test_every_term_is_needed(drop):
    """Leaving `drop` out of e_ip must be caught: on the input built for it the error exceeds the
    remaining bound, while the full bound holds on the same input."""
    rng = np.random.default_rng(11)
    n = 64
    x = np.zeros((n, D_), np.float32)
    q = np.zeros((4, D_), np.float32)
    z = np.zeros
    if drop == "qt_Rt":          # exact query tail, no heads: only the rows' tail residual acts
        x[:, HEAD:] = rng.standard_normal((n, D_ - HEAD)).astype(np.float32)
        q[:, HEAD:] = _grid_tail(rng, 4)
    elif drop == "dqt_Xt":       # exact row tails, no heads: only the query's tail residual acts
        x[:, HEAD:] = _grid_tail(rng, n)
        q[:, HEAD:] = rng.standard_normal((4, D_ - HEAD)).astype(np.float32)
    elif drop == "qh_Rh":        # bf16-exact query head, no tails: only the rows' head residual acts
        x[:, :HEAD] = rng.standard_normal((n, HEAD)).astype(np.float32)
        q[:, :HEAD] = _bf16_head(rng, 4)
    elif drop == "dqh_Xh":
        x[:, :HEAD] = _bf16_head(rng, n)
        q[:, :HEAD] = rng.standard_normal((4, HEAD)).astype(np.float32)
    else:                        # everything exactly representable: only the fp32 arithmetic acts
        x[:, HEAD:], x[:, :HEAD] = _grid_tail(rng, n), _bf16_head(rng, n)
        q[:, HEAD:], q[:, :HEAD] = _grid_tail(rng, 4), _bf16_head(rng, 4)
    assert _errs(x, q) <= 1.0
    assert _errs(x, q, drop=drop) > 1.0


def test_split_column_rule():
    cfg3 = concat_rows(2000)                                        # 48 | 128 | 1792, parts unit-norm
    assert R.pick_head(R.block_absmax(cfg3, 1984)) == 192
    homog = mixture(2000, 768, centres=16, seed=5, normalize=True)
    assert R.pick_head(R.block_absmax(homog, 768)) == 0
    short = _lead(mixture(500, 512, centres=8, seed=6, normalize=True))    # H = 64 leaves 448 < 512
    assert R.pick_head(R.block_absmax(short, 512)) == -1
    wide_head = mixture(500, 1024, centres=8, seed=7, normalize=True)
    wide_head[:, :640] *= 8.0                                       # H = 640 > dpb / 2
    assert R.pick_head(R.block_absmax(wide_head, 1024)) == -1
