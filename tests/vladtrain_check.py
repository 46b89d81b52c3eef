"""Acceptance rules of the VLAD encoder's training step (include/imgrec_vladtrain.h) against a torch
float64 restatement.  Used by tests/test_vladtrain_cpu.py (the checker itself, torch's fp32 autograd
and defective steps) and tests/test_vladtrain_gpu.py (the HIP kernels).

The step (step_torch): vladenc_check.torch_sequential walked module by module, each Dropout replaced
by the mask that is passed in times 1 / (1 - p); F.normalize; torch.cdist of the batch and of the
codes (in float64 with compute_mode="donot_use_mm_for_euclid_dist"); loss_corr = 1 - Pearson of the
two triu(1).flatten() vectors (n^2 entries, the zeros included) over the sample_idx restriction;
loss_umap = kl_div(log_softmax(-D_z / T), softmax(-D_x / T), "batchmean"); loss = 2 corr + 0.25 umap;
autograd.  adam64 is torch.optim.Adam's arithmetic in numpy float64.

Acceptance.  Per case and per parameter tensor err = max|g - g64| / max|g64|; per loss the absolute
difference.  The tolerance is 4 x the same quantity of torch's own fp32 CPU autograd against the
float64 step, the larger over cdist's two compute modes, on that case's inputs and masks
(MEASURED, printed again by tests/test_vladtrain_cpu.py); 4 because two valid fp32 orders differ from
float64 independently (vladenc_check's convention).  Adam is checked on the candidate's OWN
gradients and previous state: every element of the new parameters and moments within 4 U relative
of adam64, U = 2^-24 (a float64 update rounded once is within U; fp32 arithmetic of torch's kind
within a few U of the update, far less relative to the parameter).

Inputs: rows of a unit-normalised Gaussian mixture (centres plus noise), like VLAD vectors: D_x
spreads over roughly 0.3 ... 1.4 where iid Gaussians would concentrate it.  Parameters are drawn as
vladenc_check.case_params draws them, the first layer scaled by sqrt(K) because the inputs are unit
vectors.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import vladenc_check as ec

U = ec.U
TOL_FACTOR = 4.0
ADAM_TOL = 4.0 * U
SEED = 7            # of the trainers' masks in the GPU suite


@dataclass(frozen=True)
class Case:
    name: str
    widths: tuple
    n: int
    seed: int
    dropout: float = 0.1
    k: int = 0              # > 0: that many unsorted sample indices
    dup: tuple = ()         # (i, j): row j is a copy of row i


CASES = [
    Case("tiny", (40, 24, 12, 8), 5, 11),                      # everything under one tile
    Case("odd", (1000, 37, 19, 5), 67, 12),                    # K % 32 != 0; a weight-gradient depth B % 4 != 0
    Case("ref_small", (1024, 669, 317, 128), 130, 13),         # crosses the 128-row tile; three feature tiles
    Case("ref_full", (32768, 669, 317, 128), 33, 14),          # the 147-split forward; dW_0 at 256 row tiles
    Case("subsample", (1024, 669, 317, 128), 130, 13, k=64),   # ref_small with 64 unsorted indices
    Case("dups", (40, 24, 12, 8), 6, 11, dropout=0.0, dup=(0, 3)),   # identical rows: D = 0 exactly
    Case("one_layer", (70, 3), 6, 16, dropout=0.0),            # no LayerNorm, no dropout site
    Case("deep8", (50, 20, 18, 16, 14, 12, 10, 9, 6), 9, 17),  # VLADENC_MAX_LAYERS layers: the depth limit
]
CASE = {c.name: c for c in CASES}

# err of torch's fp32 CPU autograd against step_torch in float64 (the larger of cdist's two modes):
# the three losses (absolute), then per parameter tensor max|g - g64| / max|g64|
MEASURED = {
    "tiny": {"loss": 1.59e-06, "corr": 1.66e-07, "umap": 7.71e-06, "W0": 1.04e-05, "b0": 2.14e-05, "g0": 4e-06, "be0": 1.7e-05, "W1": 6.24e-06, "b1": 1.88e-05, "g1": 7.07e-06, "be1": 1.43e-05, "W2": 7.49e-06, "b2": 2.66e-05},
    "odd": {"loss": 2.02e-07, "corr": 8.21e-08, "umap": 1.56e-07, "W0": 3.9e-06, "b0": 5.11e-06, "g0": 4.21e-06, "be0": 5.15e-06, "W1": 4.91e-06, "b1": 6.02e-06, "g1": 2.94e-06, "be1": 6.79e-06, "W2": 2.58e-06, "b2": 5.74e-06},
    "ref_small": {"loss": 2.03e-07, "corr": 1.01e-07, "umap": 1.56e-08, "W0": 6.61e-07, "b0": 7.93e-07, "g0": 8.71e-07, "be0": 9.29e-07, "W1": 7.31e-07, "b1": 8.72e-07, "g1": 1.23e-06, "be1": 9e-07, "W2": 7.66e-07, "b2": 1.73e-06},
    "ref_full": {"loss": 2.69e-07, "corr": 8.25e-08, "umap": 4.15e-07, "W0": 5.86e-06, "b0": 1.14e-05, "g0": 6.2e-06, "be0": 1.29e-05, "W1": 4.29e-06, "b1": 1.18e-05, "g1": 7.38e-06, "be1": 1.27e-05, "W2": 8.75e-06, "b2": 1.9e-05},
    "subsample": {"loss": 1.29e-07, "corr": 6.47e-08, "umap": 1.56e-08, "W0": 1.18e-06, "b0": 2.04e-06, "g0": 2.24e-06, "be0": 2.25e-06, "W1": 1.25e-06, "b1": 2.16e-06, "g1": 3.8e-06, "be1": 2.59e-06, "W2": 2.72e-06, "b2": 6.54e-06},
    "dups": {"loss": 5.22e-07, "corr": 8.75e-08, "umap": 1.39e-06, "W0": 1.88e-06, "b0": 1.31e-06, "g0": 1.03e-06, "be0": 1.25e-06, "W1": 1.63e-06, "b1": 1.96e-06, "g1": 2.24e-06, "be1": 2.26e-06, "W2": 2.8e-06, "b2": 1.62e-06},
    "one_layer": {"loss": 4.82e-07, "corr": 8.5e-08, "umap": 1.24e-06, "W0": 3.55e-06, "b0": 1.08e-05},
    "deep8": {"loss": 8.36e-08, "corr": 4.4e-08, "umap": 1.78e-07, "W0": 4.24e-06, "b0": 4.44e-06, "g0": 2.34e-06, "be0": 4.43e-06, "W1": 4.87e-06, "b1": 4.42e-06, "g1": 6.71e-06, "be1": 3.93e-06, "W2": 6.33e-06, "b2": 4.32e-06, "g2": 4.43e-06, "be2": 4.5e-06, "W3": 8.61e-06, "b3": 5.79e-06, "g3": 5.53e-06, "be3": 6.7e-06, "W4": 7.71e-06, "b4": 7.58e-06, "g4": 4.7e-06, "be4": 6.69e-06, "W5": 8.56e-06, "b5": 1.13e-05, "g5": 8.22e-06, "be5": 1.05e-05, "W6": 5.26e-06, "b6": 9.2e-06, "g6": 6.12e-06, "be6": 8.28e-06, "W7": 8.1e-06, "b7": 1.29e-05},
}
LOSS_KEYS = ("loss", "corr", "umap")


def tensor_keys(widths):
    nl = len(widths) - 1
    keys = []
    for l in range(nl):
        keys += [f"W{l}", f"b{l}"]
        if l < nl - 1:
            keys += [f"g{l}", f"be{l}"]
    return keys


@lru_cache(maxsize=None)
def case_params(name) -> ec.Params:
    cs = CASE[name]
    rng = np.random.default_rng(cs.seed)
    W, b, g, be = [], [], [], []
    nl = len(cs.widths) - 1
    for l in range(nl):
        K, N = cs.widths[l], cs.widths[l + 1]
        W.append(rng.standard_normal((N, K), dtype=np.float32) * np.float32((np.sqrt(K) if l == 0 else 1.0) / np.sqrt(K)))
        b.append((0.1 * rng.standard_normal(N)).astype(np.float32))
        if l < nl - 1:
            g.append((1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32))
            be.append((0.1 * rng.standard_normal(N)).astype(np.float32))
    for a in (*W, *b, *g, *be):
        a.setflags(write=False)
    return ec.Params(tuple(W), tuple(b), tuple(g), tuple(be))


@lru_cache(maxsize=None)
def case_input(name) -> np.ndarray:
    """(n, K) float32, read-only: unit rows of a Gaussian mixture of 4 centres."""
    cs = CASE[name]
    rng = np.random.default_rng(1000 + cs.seed)
    K = cs.widths[0]
    centres = rng.standard_normal((4, K))
    x = centres[rng.integers(0, 4, cs.n)] + 0.7 * rng.standard_normal((cs.n, K))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = x.astype(np.float32)
    if cs.dup:
        x[cs.dup[1]] = x[cs.dup[0]]
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def case_sample(name):
    cs = CASE[name]
    if not cs.k:
        return None
    idx = np.random.default_rng(2000 + cs.seed).permutation(cs.n)[:cs.k].astype(np.int32)
    idx.setflags(write=False)
    return idx


def host_masks(cs: Case, seed=SEED, step=0):
    """The documented hash's keep masks of a case, one (n, N_l) uint8 array per hidden layer."""
    from image_recommender_amd.vlad_trainer import dropout_keep
    return [dropout_keep(seed, step, l, cs.n, cs.widths[l + 1], cs.dropout) for l in range(len(cs.widths) - 2)]


# ---- the step in torch ------------------------------------------------------------------------------
def _defective_functions():
    import torch

    class DropNoScaleBwd(torch.autograd.Function):          # the scale missing in the backward
        @staticmethod
        def forward(ctx, a, m, s):
            ctx.save_for_backward(m)
            return a * m * s

        @staticmethod
        def backward(ctx, g):
            (m,) = ctx.saved_tensors
            return g * m, None, None

    class LNUnbiasedBwd(torch.autograd.Function):           # the backward's variance over N - 1
        @staticmethod
        def forward(ctx, y, gamma, beta, eps):
            mu = y.mean(1, keepdim=True)
            d = y - mu
            var = (d * d).mean(1, keepdim=True)
            ctx.save_for_backward(d, var, gamma)
            ctx.eps = eps
            return d / torch.sqrt(var + eps) * gamma + beta

        @staticmethod
        def backward(ctx, g):
            d, var, gamma = ctx.saved_tensors
            N = d.shape[1]
            r = 1.0 / torch.sqrt(var * N / (N - 1) + ctx.eps)
            v = d * r
            dv = g * gamma
            dy = r * (dv - dv.mean(1, keepdim=True) - v * (dv * v).mean(1, keepdim=True))
            return dy, (g * v).sum(0), g.sum(0), None

    return DropNoScaleBwd, LNUnbiasedBwd


def step_torch(p: ec.Params, x, masks, sample_idx=None, dropout=0.1, dtype="float64", cdist_mode=None, defect=None,
               corr_weight=2.0, umap_weight=0.25, temperature=1.5, override=None):
    """One forward and backward.  Returns {"loss", "corr", "umap", "z", "W0", "b0", "g0", "be0", ...} as
    float64 numpy.  `defect` switches on one wrong step (the CPU test's); `override` = {key: array}
    replaces parameters after the module is in `dtype` (a float64 trajectory's)."""
    import torch
    import torch.nn.functional as F
    from torch import nn
    dt = getattr(torch, dtype)
    if cdist_mode is None:
        cdist_mode = "donot_use_mm_for_euclid_dist"
    seq = ec.torch_sequential(p, dropout=dropout).to(dt)
    if override:
        lin0 = [m for m in seq if isinstance(m, nn.Linear)]
        lns0 = [m for m in seq if isinstance(m, nn.LayerNorm)]
        with torch.no_grad():
            for l, m in enumerate(lin0):
                m.weight.copy_(torch.from_numpy(np.asarray(override[f"W{l}"])))
                m.bias.copy_(torch.from_numpy(np.asarray(override[f"b{l}"])))
            for l, m in enumerate(lns0):
                m.weight.copy_(torch.from_numpy(np.asarray(override[f"g{l}"])))
                m.bias.copy_(torch.from_numpy(np.asarray(override[f"be{l}"])))
    for q in seq.parameters():
        q.requires_grad_(True)
    X = torch.from_numpy(np.array(x, dtype=np.float32)).to(dt)
    scale = 1.0 / (1.0 - dropout)
    DropNoScaleBwd, LNUnbiasedBwd = _defective_functions()
    a, site = X, 0
    for mod in seq:
        if isinstance(mod, nn.Dropout):
            m = torch.from_numpy(np.asarray(masks[site])).to(dt)
            site += 1
            if dropout > 0:
                a = DropNoScaleBwd.apply(a, m, scale) if defect == "dropout_scale" else a * m * scale
        elif isinstance(mod, nn.LayerNorm) and defect == "ln_variance":
            a = LNUnbiasedBwd.apply(a, mod.weight, mod.bias, mod.eps)
        else:
            a = mod(a)
    z = F.normalize(a, p=2, dim=-1)
    if defect == "no_transpose":
        z_in, z = z, z.detach().requires_grad_(True)
    D_x = torch.cdist(X, X, compute_mode=cdist_mode)
    D_z = torch.cdist(z, z, compute_mode=cdist_mode)
    if defect == "no_transpose":
        D_leaf = D_z.detach().requires_grad_(True)
        D_used = D_leaf
    else:
        D_used = D_z
    A, B = D_x, D_used
    if sample_idx is not None:
        idx = torch.from_numpy(np.asarray(sample_idx, dtype=np.int64))
        A, B = A[idx][:, idx], B[idx][:, idx]
    af, bf = A.triu(1).flatten(), B.triu(1).flatten()
    if defect == "pearson_pairs":
        iu = torch.triu_indices(A.shape[0], A.shape[0], 1)
        af, bf = A[iu[0], iu[1]], B[iu[0], iu[1]]
    ac, bc = af - af.mean(), bf - bf.mean()
    corr = (ac * bc).sum() / (ac.pow(2).sum().sqrt() * bc.pow(2).sum().sqrt() + 1e-8)
    loss_corr = 1 - corr
    T = 1.0 if defect == "temperature" else temperature
    loss_umap = F.kl_div(F.log_softmax(-D_used / T, dim=1), F.softmax(-D_x / T, dim=1),
                         reduction="sum" if defect == "kl_sum" else "batchmean")
    loss = corr_weight * loss_corr + umap_weight * loss_umap
    if defect == "no_transpose":
        loss.backward()
        G = D_leaf.grad                                     # dL/dD_z[i][j]; the transposed term left out
        zd = z.detach()
        diff = zd[:, None, :] - zd[None, :, :]
        Dd = D_z.detach()
        w = torch.where(Dd > 0, G / torch.where(Dd > 0, Dd, torch.ones_like(Dd)), torch.zeros_like(Dd))
        z_in.backward((w[:, :, None] * diff).sum(1))
    else:
        loss.backward()
    out = {"loss": float(loss.detach()), "corr": float(loss_corr.detach()), "umap": float(loss_umap.detach()),
           "z": z.detach().to(torch.float64).numpy()}
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    lns = [m for m in seq if isinstance(m, nn.LayerNorm)]
    for l, m in enumerate(lin):
        out[f"W{l}"] = m.weight.grad.to(torch.float64).numpy()
        out[f"b{l}"] = m.bias.grad.to(torch.float64).numpy()
    for l, m in enumerate(lns):
        out[f"g{l}"] = m.weight.grad.to(torch.float64).numpy()
        out[f"be{l}"] = m.bias.grad.to(torch.float64).numpy()
    return out


@lru_cache(maxsize=None)
def case_reference(name):
    """step_torch in float64 on the case's inputs with the host's masks at (SEED, step 0): computed
    once, shared, never modified."""
    cs = CASE[name]
    return step_torch(case_params(name), case_input(name), host_masks(cs), case_sample(name), dropout=cs.dropout)


def params_dict(p: ec.Params) -> dict:
    """A Params' arrays under step_torch's keys, float64."""
    out = {}
    for l in range(len(p.W)):
        out[f"W{l}"], out[f"b{l}"] = np.array(p.W[l], np.float64), np.array(p.b[l], np.float64)
    for l in range(len(p.g)):
        out[f"g{l}"], out[f"be{l}"] = np.array(p.g[l], np.float64), np.array(p.be[l], np.float64)
    return out


def trajectory64(name, steps, dropout=0.0, masks=None, **hyper):
    """The losses of `steps` float64 steps (step_torch + adam64) on the case's batch from its parameters."""
    cs = CASE[name]
    p, x = case_params(name), case_input(name)
    cur = params_dict(p)
    m = {k: np.zeros_like(v) for k, v in cur.items()}
    v = {k: np.zeros_like(a) for k, a in cur.items()}
    if masks is None:
        masks = [np.ones((cs.n, w), np.uint8) for w in cs.widths[1:-1]]
    out = []
    for t in range(1, steps + 1):
        r = step_torch(p, x, masks, case_sample(name), dropout=dropout, override=cur)
        out.append((r["loss"], r["corr"], r["umap"]))
        for k in cur:
            cur[k], m[k], v[k] = adam64(cur[k], r[k], m[k], v[k], t, **hyper)
    return out


def errors(widths, got, ref) -> dict:
    """The acceptance quantities of `got` (a dict as step_torch's) against `ref`."""
    e = {k: abs(float(got[k]) - float(ref[k])) for k in LOSS_KEYS}
    for k in tensor_keys(widths):
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        assert g.shape == r.shape, f"{k}: shape {g.shape}, expected {r.shape}"
        if not np.isfinite(g).all():
            e[k] = float("inf")
            continue
        e[k] = float(np.abs(g - r).max() / np.abs(r).max())
    return e


def torch_yardstick(name) -> dict:
    """errors() of torch's fp32 autograd, the larger of cdist's two compute modes."""
    cs = CASE[name]
    ref = case_reference(name)
    worst = {}
    for mode in ("use_mm_for_euclid_dist", "donot_use_mm_for_euclid_dist"):
        got = step_torch(case_params(name), case_input(name), host_masks(cs), case_sample(name), dropout=cs.dropout,
                         dtype="float32", cdist_mode=mode)
        for k, v in errors(cs.widths, got, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def tolerances(name) -> dict:
    return {k: TOL_FACTOR * v for k, v in MEASURED[name].items()}


def failures(name, got, keys=None) -> list:
    """The quantities of `got` above the case's tolerance, as (key, error, tolerance)."""
    cs = CASE[name]
    e, tol = errors(cs.widths, got, case_reference(name)), tolerances(name)
    return [(k, e[k], tol[k]) for k in (keys or e) if not e[k] <= tol[k]]


def check_step(name, got, keys=None) -> dict:
    bad = failures(name, got, keys)
    assert not bad, f"{name}: " + "; ".join(f"{k} off by {e:.3e}, tolerance {t:.3e}" for k, e, t in bad)
    return errors(CASE[name].widths, got, case_reference(name))


def as_step(res, z=None) -> dict:
    """VladEncoderTrainer.grads' dict in step_torch's keys."""
    out = dict(zip(LOSS_KEYS, res["losses"]))
    for l, w in enumerate(res["weights"]):
        out[f"W{l}"] = w
        out[f"b{l}"] = res["biases"][l]
    for l, g in enumerate(res["ln_weights"]):
        out[f"g{l}"] = g
        out[f"be{l}"] = res["ln_biases"][l]
    return out


# ---- Adam ---------------------------------------------------------------------------------------------
def adam64(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, defect=None):
    """torch.optim.Adam's update number t (1-based) of one tensor in float64: (p, m, v) after it."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    if defect == "adamw":
        p = p * (1.0 - lr * weight_decay)
    else:
        g = g + weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = (1.0, 1.0) if defect == "no_bias_correction" else (1.0 - b1 ** t, 1.0 - b2 ** t)
    return p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps), m, v


def adam_failures(prev, grads, new, t, **kw) -> list:
    """prev / new = (params, m, v), each a flat list of arrays; grads likewise.  The elements of
    `new` further than 4 U relative from adam64 of the candidate's own gradients and state."""
    bad = []
    for i, (p, g, m, v) in enumerate(zip(prev[0], grads, prev[1], prev[2])):
        ref = adam64(p, g, m, v, t, **kw)
        for what, r, got in zip(("p", "m", "v"), ref, (new[0][i], new[1][i], new[2][i])):
            err = np.abs(np.asarray(got, np.float64) - r)
            if not (err <= ADAM_TOL * np.abs(r)).all():
                bad.append((i, what, float((err / np.maximum(np.abs(r), 1e-300)).max())))
    return bad
