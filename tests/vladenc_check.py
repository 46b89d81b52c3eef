"""Acceptance rules of the VLAD encoder's forward pass (include/imgrec_vladenc.h) against a numpy
float64 restatement.  Used by tests/test_vladenc_cpu.py (the checker itself, on an fp32 numpy
encoding and on defective ones) and tests/test_vladenc_gpu.py (the HIP kernels).

U = 2^-24, the relative rounding error of one fp32 operation.  Every stage is checked against
float64 applied to the encoding's OWN input of that stage (x, or the `hidden` it returned), so no
stage inherits the error of the one before.

* hidden layers (check_linear).  Layer l has depth K, N features, input a (fp32), y64 = W a + b.
  The pre-activation y of any fp32 implementation satisfies

      |y_f - y64_f| <= E_f = (K + 2) U sum_j |w_fj| |a_j| + U |b_f|

  (K products, at most K - 1 additions of partial sums in ANY order, tree or sequential, split or
  not: an element passes through at most K - 1 additions; one more for the bias, whose own rounding
  is U |y| <= U (sum + |b|)).  y is not output, so E is folded through the LayerNorm and Mish, first
  order plus the explicit second-order terms written below; N means per row over the features:
    mean        |mu - mu64| <= Em = mean(E) + (N + 1) U mean|y64|: the propagated part, plus an fp32
                sum of N terms in any order and the division (a float64 sum is far inside it).
    deviation   d = y - mu:  |d - d64| <= Ed = E + Em + U |d64|  (the subtraction's rounding).
    variance    v = mean(d^2) (biased):  |v - v64| <= Ev = mean(2 |d64| Ed + Ed^2) + (N + 2) U v64
                (the squares, an fp32 sum in any order, the division).
    1 / sigma   r = 1 / sqrt(v + eps), s = v64 + eps.  By the mean value theorem, |dr/dv| =
                (v + eps)^-3/2 / 2 <= (s - Ev)^-3/2 / 2 on the interval, so
                |r - r64| <= Er = Ev (s - Ev)^-3/2 / 2 + 3 U r64  (the addition of eps, the square
                root and the division, U each).  The case fails unless Ev < s.
    normalised  n = d r:  |n - n64| <= En = Ed r64 + |d64| Er + Ed Er + U |n64|.
    affine      z = n gamma + beta:  |z - z64| <= Ez = |gamma| En + U (2 |n64 gamma| + |beta|)
                (a product and an addition; fused they round once, which is less).
    Mish        h = z tanh(softplus(z)).  Propagated: LIP Ez with LIP = sup |mish'| = 1.088498...
                (attained near z = 1.49; rounded up to 1.0885, asserted on a grid by the CPU test).
                Its own term assumes the formula x * tanhf(x > 20 ? x : log1pf(expf(x))) with the
                OpenCL C full-profile ulp bounds that the HIP device library implements: expf 3,
                log1pf 2, tanhf 5 ulp, an ulp being at most 2 U relative.  e = expf(x) is off by
                6 U relative; log1p(e (1 + t)) moves by t e / (1 + e) <= t log1p(e) (because
                log(1 + e) >= e / (1 + e)), so softplus is off by 6 U + 4 U; tanh(p (1 + t)) moves
                by t p sech^2 p = t tanh(p) (2 p / sinh 2 p) <= t tanh(p), so tanh is off by
                10 U + 10 U; the product adds U:  MISH_U = 2 (3 + 2 + 5) + 1 = 21, relative to
                |mish(z)| <= |h64| + LIP Ez.  For x > 20 softplus is x itself and tanhf is 1.
    So the per-element bound on a hidden activation is

      |h - h64| <= Eh = LIP Ez + 21 U (|h64| + LIP Ez).

* output (check_output), against float64 of the encoding's own last pre-normalisation input.  The
  last layer's z is not output and out * |...| recovers it only up to scale, so the DIRECTION is
  checked: with |z - z64| <= E as above and |E| its 2-norm, u = z / |z| satisfies
      |u_f - u64_f| <= (E_f + |u64_f| |E|) / (|z64| - |E|) + U (1 + 2^-20) |u64_f|
  (|z| differs from |z64| by at most |E|; the norm is accumulated in float64, whose error is below
  2^-20 U, and the quotient is rounded once), and the model output's norm is within 2 U of 1
  (each element within U of the unit vector, relative).  VLADENC_MODEL_OUTPUT relates to the default by one
  division: stored = u / (|u| + 1e-7) over the RETURNED fp32 u, float64 and rounded once, so
  |stored - that| <= U (1 + 2^-20) |stored|.  1e-7 is 1.68 U: leaving the division out, or
  applying it twice, moves every element by more than the bound.
* end to end (check_end_to_end): the stored vector against forward64 of the true input, within
  E2E_TOL[case] = 4 x the largest absolute difference between forward64 and torch's own fp32 CPU
  forward of the same nn.Sequential (the reference's arithmetic) on that case's inputs; 4 because
  two valid fp32 summation orders differ from float64 independently.  Measured (E2E_MEASURED,
  printed again by tests/test_vladenc_cpu.py):
      ref_small 2.56e-07   odd 7.96e-07   one_layer 5.43e-08   deep 2.21e-07
      ref_full  2.34e-07   one_hot 5.93e-08

Cases.  Parameters come from default_rng(seed): W ~ N(0, 1) / sqrt(K) (so pre-activations of O(1)
inputs are O(1); ref_full's inputs are unit VLAD vectors, so its first layer is N(0, 1)),
b ~ 0.1 N(0, 1), gamma ~ 1 + 0.1 N(0, 1), beta ~ 0.1 N(0, 1); inputs N(0, 1).  The smallest
hidden-row variance of every case is asserted by the CPU test (MIN_VAR).
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

U = 2.0 ** -24
LIP = 1.0885
MISH_U = 2 * (3 + 2 + 5) + 1
LN_EPS = 1e-5
MIN_VAR = 1e-3
E2E_MEASURED = {"ref_small": 2.56e-07, "odd": 7.96e-07, "one_layer": 5.43e-08, "deep": 2.21e-07,
                "ref_full": 2.34e-07, "one_hot": 5.93e-08}
E2E_TOL = {k: 4.0 * v for k, v in E2E_MEASURED.items()}


@dataclass(frozen=True)
class Case:
    name: str
    widths: tuple
    batches: tuple           # batch sizes the GPU suite runs
    seed: int
    w0_scale: float = 1.0    # the first layer's extra scale


CASES = [
    Case("ref_small", (1024, 669, 317, 128), (0, 1, 3, 129), 1),   # the reference's odd widths, three feature tiles
    Case("odd", (1000, 37, 19, 5), (0, 1, 3, 129), 2),             # K % 32 != 0, K % 4 != 0 later: scalar loads
    Case("one_layer", (70, 3), (5,), 3),                           # no LayerNorm at all
    Case("deep", (11, 9, 7, 5, 3, 6), (7,), 4),                    # five layers: the layer loop
    Case("ref_full", (32768, 669, 317, 128), (8,), 5, 32768 ** 0.5),   # the real depth and split count
    Case("one_hot", (1024, 669, 317, 128), (2,), 1),               # ref_small's weights, one-hot inputs
]
CASE = {c.name: c for c in CASES}


def split_rule(K, N):
    """(tiles, stages, stages per split, splits) of include/imgrec_vladenc.h "linear"."""
    tiles, stages = -(-N // 256), -(-K // 32)
    s0 = min(max(1, 512 // tiles), max(1, stages // 4))
    per = -(-stages // s0)
    return tiles, stages, per, -(-stages // per)


@dataclass(frozen=True, eq=False)
class Params:
    W: tuple
    b: tuple
    g: tuple
    be: tuple
    eps: float = LN_EPS

    @property
    def widths(self):
        return (self.W[0].shape[1],) + tuple(w.shape[0] for w in self.W)

    @property
    def hidden_widths(self):
        return self.widths[1:-1]


@lru_cache(maxsize=None)
def case_params(name) -> Params:
    cs = CASE[name]
    rng = np.random.default_rng(cs.seed)
    W, b, g, be = [], [], [], []
    nl = len(cs.widths) - 1
    for l in range(nl):
        K, N = cs.widths[l], cs.widths[l + 1]
        w = rng.standard_normal((N, K), dtype=np.float32) * np.float32((cs.w0_scale if l == 0 else 1.0) / np.sqrt(K))
        W.append(w)
        b.append((0.1 * rng.standard_normal(N)).astype(np.float32))
        if l < nl - 1:
            g.append((1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32))
            be.append((0.1 * rng.standard_normal(N)).astype(np.float32))
    for a in (*W, *b, *g, *be):
        a.setflags(write=False)
    return Params(tuple(W), tuple(b), tuple(g), tuple(be))


@lru_cache(maxsize=None)
def case_input(name, n=None) -> np.ndarray:
    """The (n, K) float32 input of a case (n defaults to its largest batch), read-only; a smaller
    batch is a prefix of a larger one."""
    cs = CASE[name]
    K = cs.widths[0]
    if name == "ref_full":
        from tests import vlad_check as vc
        v = vc.CASE["sift"]
        x, off, c = vc.case_data("sift")
        out = np.ascontiguousarray(vc.encode32(x, off, c, v.nn, v.sigma)[0])
    elif name == "one_hot":
        out = np.zeros((2, K), np.float32)
        out[0, K - 1] = 1.5                                 # the very last column
        out[1, split_rule(K, cs.widths[1])[2] * 32 - 1] = -2.0      # the last column of the first split
    else:
        out = np.random.default_rng(100 + cs.seed).standard_normal((max(cs.batches), K), dtype=np.float32)
    if n is not None:
        out = np.ascontiguousarray(out[:n])
    out.setflags(write=False)
    return out


# ---- float64 -------------------------------------------------------------------------------------------
def mish64(z):
    z = np.asarray(z, np.float64)
    sp = np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0))))
    return z * np.tanh(sp)


def layer64(p: Params, l, a):
    """(y64, hidden64 or None) of layer l on input a."""
    y = np.asarray(a, np.float64) @ p.W[l].astype(np.float64).T + p.b[l].astype(np.float64)
    if l == len(p.W) - 1:
        return y, None
    mu = y.mean(1, keepdims=True)
    d = y - mu
    v = (d * d).mean(1, keepdims=True)
    z = d / np.sqrt(v + p.eps) * p.g[l].astype(np.float64) + p.be[l].astype(np.float64)
    return y, mish64(z)


def normalize64(z):
    return z / np.maximum(np.sqrt((z * z).sum(1, keepdims=True)), 1e-12)


def second64(u):
    u = np.asarray(u, np.float64)
    return u / (np.sqrt((u * u).sum(1, keepdims=True)) + 1e-7)


def forward64(p: Params, x):
    """{"pre": [y of every layer], "hidden": [every hidden activation], "model", "stored"} in float64."""
    a = np.asarray(x, np.float64)
    pre, hidden = [], []
    for l in range(len(p.W)):
        y, h = layer64(p, l, a)
        pre.append(y)
        if h is not None:
            hidden.append(h)
            a = h
    model = normalize64(pre[-1])
    return {"pre": pre, "hidden": hidden, "model": model, "stored": second64(model)}


def min_hidden_variance(p: Params, x):
    f = forward64(p, x)
    return min((float(y.var(1).min()) for y in f["pre"][:-1] if y.shape[0]), default=np.inf)


# ---- a plain fp32 numpy encoding, and its defective variants -----------------------------------------
def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def mish32(z):
    """x * tanhf(softplus) with every function correctly rounded to fp32 (float64, then one rounding)."""
    z = np.asarray(z, np.float32)
    e = _f32(np.exp(np.minimum(z, np.float32(20)).astype(np.float64)))
    sp = np.where(z > 20, z, _f32(np.log1p(e.astype(np.float64))))
    return z * _f32(np.tanh(sp.astype(np.float64)))


def gelu32(z):
    z = np.asarray(z, np.float64)
    return _f32(0.5 * z * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (z + 0.044715 * z ** 3))))


def forward32(p: Params, x, drop_cols=None, no_bias=False, unbiased=False, no_gamma=False, act=mish32, second=1):
    """(stored, model, hidden (n, sum of hidden widths)) in fp32 numpy: BLAS products, float64 sums
    for the LayerNorm statistics and the norms (rounded once), fp32 elsewhere.  The keyword
    arguments switch on one defect each: columns of the first layer dropped (a slice), no bias, the
    unbiased variance, no gamma, another activation, the second division applied `second` times (by the same divisor: dividing
    the result by ITS norm + 1e-7 again changes it by 1e-14, which no fp32 check can see)."""
    a = np.asarray(x, np.float32)
    n = a.shape[0]
    hidden = []
    nl = len(p.W)
    for l in range(nl):
        w = p.W[l]
        if l == 0 and drop_cols is not None:
            w = w.copy()
            w[:, drop_cols] = 0
        y = a @ w.T
        if not no_bias:
            y = y + p.b[l]
        if l == nl - 1:
            break
        y64 = y.astype(np.float64)
        mu = y64.mean(1, keepdims=True)
        d = y64 - mu
        v = (d * d).sum(1, keepdims=True) / (y.shape[1] - (1 if unbiased else 0))
        nrm = _f32(d / np.sqrt(v + np.float64(np.float32(p.eps))))
        z = nrm * (np.float32(1) if no_gamma else p.g[l]) + p.be[l]
        a = act(z).astype(np.float32)
        hidden.append(a)
    model = _f32(normalize64(y.astype(np.float64)))
    div = np.sqrt((model.astype(np.float64) ** 2).sum(1, keepdims=True)) + 1e-7
    stored = _f32(model.astype(np.float64) / div ** second)
    hid = np.concatenate(hidden, axis=1) if hidden else np.zeros((n, 0), np.float32)
    return stored, model, np.ascontiguousarray(hid)


# ---- the checks --------------------------------------------------------------------------------------
def linear_bound(p: Params, l, a):
    """(y64, E) of layer l on the float64 input a."""
    W = p.W[l].astype(np.float64)
    b = p.b[l].astype(np.float64)
    K = W.shape[1]
    return a @ W.T + b, (K + 2) * U * (np.abs(a) @ np.abs(W).T) + U * np.abs(b)


def hidden_bound(p: Params, l, a):
    """(h64, Eh) of hidden layer l on input a: the derivation of the module docstring, term by term."""
    a = np.asarray(a, np.float64)
    y, E = linear_bound(p, l, a)
    N = y.shape[1]
    g, be = p.g[l].astype(np.float64), p.be[l].astype(np.float64)
    mu = y.mean(1, keepdims=True)
    d = y - mu
    Em = E.mean(1, keepdims=True) + (N + 1) * U * np.abs(y).mean(1, keepdims=True)
    Ed = E + Em + U * np.abs(d)
    v = (d * d).mean(1, keepdims=True)
    Ev = (2 * np.abs(d) * Ed + Ed * Ed).mean(1, keepdims=True) + (N + 2) * U * v
    s = v + p.eps
    assert (Ev < s).all(), "a row's variance is within its own error bound: the case tests nothing"
    r = 1.0 / np.sqrt(s)
    Er = 0.5 * Ev * (s - Ev) ** -1.5 + 3 * U * r
    n64 = d * r
    En = Ed * r + np.abs(d) * Er + Ed * Er + U * np.abs(n64)
    z = n64 * g + be
    Ez = np.abs(g) * En + U * (2 * np.abs(n64 * g) + np.abs(be))
    h = mish64(z)
    return h, LIP * Ez + MISH_U * U * (np.abs(h) + LIP * Ez)


def split_hidden(p: Params, hidden):
    hw = p.hidden_widths
    hidden = np.asarray(hidden)
    assert hidden.dtype == np.float32 and hidden.ndim == 2 and hidden.shape[1] == sum(hw), \
        f"hidden has shape {hidden.shape}, dtype {hidden.dtype}"
    cuts = np.cumsum((0,) + tuple(hw))
    return [hidden[:, cuts[i]:cuts[i + 1]] for i in range(len(hw))]


def check_linear(p: Params, x, hidden):
    """Every hidden layer against float64 of its own input.  Returns the largest error / bound."""
    parts = split_hidden(p, hidden)
    a = np.asarray(x, np.float64)
    worst = 0.0
    for l, got in enumerate(parts):
        assert got.shape[0] == a.shape[0], f"hidden has {got.shape[0]} rows for {a.shape[0]} inputs"
        if a.shape[0]:
            h, Eh = hidden_bound(p, l, a)
            err = np.abs(got.astype(np.float64) - h)
            bad = ~(err <= Eh)
            if bad.any():
                i, f = (int(v[0]) for v in np.nonzero(bad))
                raise AssertionError(f"{int(bad.sum())} hidden activations of layer {l} off, e.g. row {i} feature {f}: "
                                     f"{err[i, f]:.3e}, bound {Eh[i, f]:.3e}")
            worst = max(worst, float((err / Eh).max()))
        a = got.astype(np.float64)
    return worst


def last_input(p: Params, x, hidden):
    """The last layer's own input: the last hidden activation the encoding returned, or x."""
    parts = split_hidden(p, hidden)
    return np.asarray(parts[-1] if parts else x, np.float64)


def check_output(p: Params, x, hidden, model, stored):
    model, stored = np.asarray(model), np.asarray(stored)
    a = last_input(p, x, hidden)
    n, N = a.shape[0], p.widths[-1]
    for name, o in (("model output", model), ("stored vector", stored)):
        assert o.dtype == np.float32 and o.shape == (n, N), f"{name} has shape {o.shape}, dtype {o.dtype}"
    if n == 0:
        return
    z, E = linear_bound(p, len(p.W) - 1, a)
    zn = np.sqrt((z * z).sum(1, keepdims=True))
    En = np.sqrt((E * E).sum(1, keepdims=True))
    assert (En < zn).all(), "an output row is within its own error bound of zero: the case tests nothing"
    u = z / zn
    own = U * (1 + 2.0 ** -20)
    bound = (E + np.abs(u) * En) / (zn - En) + own * np.abs(u)
    err = np.abs(model.astype(np.float64) - u)
    bad = ~(err <= bound)
    if bad.any():
        i, f = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{int(bad.sum())} model outputs off in direction, e.g. row {i} feature {f}: "
                             f"{err[i, f]:.3e}, bound {bound[i, f]:.3e}")
    norm = np.sqrt((model.astype(np.float64) ** 2).sum(1))
    assert (np.abs(norm - 1.0) <= 2 * U).all(), f"a model output is not a unit vector: |.| - 1 = {np.abs(norm - 1).max():.3e}"
    ref = second64(model)
    err = np.abs(stored.astype(np.float64) - ref)
    bad = ~(err <= own * np.abs(ref))
    if bad.any():
        i, f = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{int(bad.sum())} stored elements are not the model output / (its norm + 1e-7), e.g. row {i} "
                             f"feature {f}: {stored[i, f]!r} vs {ref[i, f]!r}")


def end_to_end_error(p: Params, x, stored):
    if np.asarray(x).shape[0] == 0:
        return 0.0
    return float(np.abs(np.asarray(stored, np.float64) - forward64(p, x)["stored"]).max())


def check_end_to_end(name, p: Params, x, stored):
    err = end_to_end_error(p, x, stored)
    assert err <= E2E_TOL[name], f"{name}: end-to-end error {err:.3e} above 4 x torch's own {E2E_MEASURED[name]:.3e}"
    return err


def check_all(name, p: Params, x, stored, model, hidden):
    """Returns (largest hidden error / bound, end-to-end error)."""
    ratio = check_linear(p, x, hidden)
    check_output(p, x, hidden, model, stored)
    return ratio, check_end_to_end(name, p, x, stored)


# ---- torch's own forward (the reference's arithmetic) ---------------------------------------------------
def torch_sequential(p: Params, dropout=0.1):
    """nn.Sequential(Linear, LayerNorm, Mish, Dropout, ..., Linear) with p's parameters, fp32, eval."""
    import torch
    from torch import nn
    mods = []
    nl = len(p.W)
    for l in range(nl):
        lin = nn.Linear(p.W[l].shape[1], p.W[l].shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.array(p.W[l])))
            lin.bias.copy_(torch.from_numpy(np.array(p.b[l])))
        mods.append(lin)
        if l < nl - 1:
            ln = nn.LayerNorm(p.W[l].shape[0], eps=p.eps)
            with torch.no_grad():
                ln.weight.copy_(torch.from_numpy(np.array(p.g[l])))
                ln.bias.copy_(torch.from_numpy(np.array(p.be[l])))
            mods += [ln, nn.Mish(), nn.Dropout(dropout)]
    return nn.Sequential(*mods).eval()


def torch_stored(p: Params, x, double=False):
    """compute_vectors' lines over torch's forward: F.normalize, then / (norm + 1e-7) in numpy."""
    import torch
    import torch.nn.functional as F
    seq = torch_sequential(p)
    t = torch.from_numpy(np.array(x, dtype=np.float32))
    if double:
        seq, t = seq.double(), t.double()
    with torch.no_grad():
        model = F.normalize(seq(t), p=2, dim=-1).numpy()
    stored = model.copy()
    stored /= np.linalg.norm(stored, axis=1, keepdims=True) + 1e-7
    return stored, model
