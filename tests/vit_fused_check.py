"""Checks of the fused ViT elementwise kernels (csrc/vit_fused.hip: add + LayerNorm, GELU,
QuickGELU, patchify, tokens) shared by the GPU test (tests/test_vit_elementwise_gpu.py) and by
its CPU proof (tests/test_vit_fused_check_cpu.py).  torch only; every function runs on the CPU or
the GPU.  Inputs come from a CPU generator with a fixed seed: the same bits on every machine.

Four things live here:

* float64 references with error bounds derived from the kernels' arithmetic
  (`layernorm_reference` / `layernorm_bound`, `gelu_reference` / `gelu_bound`,
  `quick_gelu_reference` / `quick_gelu_bound`), and the bit-exact fp32 references
  (`residual_reference`, `patchify_reference`, `tokens_reference`);
* the checkers built on them (`check_add_layernorm`, `activation_ratio`);
* the LayerNorm input suites (`ln_inputs`), two of which are exact probes;
* emulations of the kernels' arithmetic with switches for the mistakes such kernels typically
  have (`emulate_add_layernorm`, `emulate_gelu`, `emulate_quick_gelu`, `emulate_patchify`), which
  the CPU test uses to show that the checks can fail.

Every bound has the form |out - ref| <= half_ulp_bf16(ref) + slack: the one rounding to bf16 of the
kernel's fp32 result v, plus slack >= |v - ref|, the fp32 arithmetic error of a correct kernel.
u = 2^-24 is fp32's unit roundoff and g(k) = k u / (1 - k u) bounds k compounded roundings.  The
rounding acts on v, not on ref: where |ref| + slack reaches the next binade the half-spacing there
is twice as large, and slack carries that difference (`_bound`), so the form is rigorous.  Nothing
in a slack is taken from a kernel's output or fitted to what a GPU returned.

LayerNorm.  Per row of n = dim fp32 values v_i (the updated residual, which the reference takes
as given) with mu, var its exact mean and biased variance, A = mean|v|, r = 1 / sqrt(var + eps),
d_i = v_i - mu, the kernel computes (add_ln_kernel and add_ln_vec_kernel differ in order only):
  * s = sum v_i: per-lane chains of at most 16 additions, then 6 butterfly steps; any order of
    depth <= 22 gives |s^ - s| <= g(22) n A.  mean^ = s^ / n is one correctly rounded division
    (no fast-math flag), so |mean^ - mu| <= Em = g(23) A.  This is the cancellation: it does
    not shrink with the spread of the row;
  * d^_i = fl(v_i - mean^): |d^_i - d_i| <= e_i = Em + f_i, f_i = u (|v_i| + A + Em)
    (|v_i - mean^| <= |v_i| + A + Em);
  * q^ = sum d^_i^2 by fma chains of depth <= 16 and the 6 butterfly steps, all terms >= 0:
    relative g(22).  With d^_i = d_i + c + f'_i (c the common part, |c| <= Em, |f'_i| <= f_i) and
    sum d_i = 0: |mean d^^2 - var| <= dv = Em^2 + mean f^2 + 2 sqrt(var mean f^2) + 2 Em mean f
    (Cauchy-Schwarz on sum d_i f'_i; the cross term c sum d_i vanishes).  The division by n and
    the addition of eps round once each: the argument w = var + eps of the root carries the
    relative error dw = (dv + g(22) (var + dv) + 2 u (w + dv)) / w;
  * r^ = rsqrtf(w^): v_rsq_f32 is accurate to 1 ulp = 2^-23 relative, and (1 - dw)^(-1/2) - 1 <=
    dw / (2 (1 - dw)): relative rho = dw / (2 (1 - dw)) + 2^-23 (the check is void, bound = inf,
    where dw >= 1/2: a constant row against an eps far below fp32's resolution of its mean);
  * t^_i = fl(d^_i r^): |t^_i - d_i r| <= et_i = r (e_i + (|d_i| + e_i) (rho + u + rho u));
  * y_i = fma(t^_i, gamma_i, beta_i), one rounding of an exact t^ gamma + beta:
    slack_i = |gamma_i| et_i + u (|d_i r gamma_i| + |gamma_i| et_i + |beta_i|) + 2^-149
    (2^-149: fp32's own subnormal spacing, where the result underflows).
eps is the fp32 value the C ABI receives: the reference rounds it to fp32 first.
Two cases are exact instead: dim = 1 (s = v, v / 1 = v, v - v = 0) and the `zeros` and `pow2`
suites (every partial sum of equal powers of two is exact, so mean^ = v and d^ = 0): there
y == bf16(beta) bit for bit, whatever eps.

GELU (erf form): out = bf16(fl(fl(0.5 a) fl(1 + erff(fl(a c))))), c = fp32(1 / sqrt 2).
  * fl(0.5 a) is exact.  z^ = fl(a c) has relative error 2 u + u^2 (the constant's rounding and
    the product's); through erf'(z) = 2 / sqrt(pi) exp(-z^2) that moves erf by at most
    2.5 u |z| erf'(z) (the half u covers the second-order remainder, <= 2 u^2);
  * erff is allowed 4 ulp (device math libraries specify their fp32 erf at 2 to 4 ulp; the
    larger is taken): 8 u |erf(z)|;
  * fl(1 + E^) rounds once: u (1 + erf z + the two above).  For negative a the sum 1 + erf z
    cancels and these ABSOLUTE errors of about 9 u remain: Dw = 2.5 u |z| erf'(z) + 8 u |erf z|
    + u (1 + erf z + ...), an absolute term of about 4.5 * 2^-24 |a| in the result;
  * the final product rounds once: slack = 0.5 |a| Dw (1 + u) + u |ref| + 2^-149.
The float64 reference is 0.5 a erfc(-a / sqrt 2), which does not cancel.

QuickGELU: out = bf16(fl(a / fl(1 + exp2(fl(fl(-1.702f a) log2e_f))))), t = -1.702 a.
  * the exponent: two constants and two products round, relative 4 u, which is an absolute
    4 u |t| in natural-log units and so a RELATIVE error expm1(4 u |t|) of the exponential — it
    grows with |1.702 a| — and v_exp_f32 adds 1 ulp = 2 u: eE;
  * fl(1 + E^): relative es = eE E / (1 + E) + u (1 + eE E / (1 + E));
  * the correctly rounded division: |out / ref - 1| <= (1 + u) / (1 - es) - 1;
  * the floor.  fp32's smallest normal is 2^-126: an fp32 unit may flush what lies below it, so
    2^-126 absolute everywhere.  Where E = e^t >= 2^126 the exponential is within a factor 4 of
    fp32's largest finite value 2^128 (1 - 2^-24) and may overflow: out and ref have one sign,
    |ref| <= |a| 2^-126 and |out| <= |a| 2^-125 (1 + 2^-20), so |out - ref| <= |a| 2^-125 (1 + 2^-20)
    for 126 ln 2 <= t < 130 ln 2 (there |a| < 53); from t >= 130 ln 2 on the exponential has
    overflowed to inf for certain, out = -0 and the error is |ref| itself.
The value -inf: both formulas give -inf * 0.  The kernels are held to the bf16 rounding of
torch's own fp32 op on the CPU for that one input (F.gelu, h * sigmoid(1.702 h)): that is NaN.
NaN in gives NaN out, +inf gives +inf.

Patchify and tokens are bit-exact against the fp32 torch ops on the CPU: both sides perform the
same correctly rounded subtract and divide (or add) and one round-to-nearest-even to bf16.

The emulations follow the kernels operation by operation in fp32 (fma through float64: the
product of two fp32 is exact there).  The summation ORDER inside a wave is not emulated: per-lane
chains as in add_ln_kernel, then torch's sum over the 64 lanes in place of the butterfly.
"""
import math

import torch

from tests.vit_check import NAN_BITS

U = 2.0 ** -24
F32_NAN_BITS = 0x7FC0BEEF             # the quiet NaN the fp32 guards are pre-filled with
ERFF_ULP = 4.0
LOG2E_F = 1.4426950408889634          # rounded to fp32 where the emulation uses it
SQRT1_2 = 0.70710678118654752


def _g(k):
    return k * U / (1.0 - k * U)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % (2 ** 62)
    return torch.Generator(device="cpu").manual_seed(seed)


# ---- the bf16 grid -------------------------------------------------------------------------------
def half_ulp_bf16(r):
    """Half the spacing of the bf16 grid at the float64 value(s) r: 2^(floor(log2 |r|) - 8) for
    normal r, the constant 2^-134 below 2^-126 (bf16's subnormals are 2^-133 apart) and at 0."""
    r = torch.as_tensor(r, dtype=torch.float64)
    _, ex = torch.frexp(r.abs())                              # |r| = m 2^ex, m in [0.5, 1)
    e = torch.where(r == 0, torch.full_like(ex, -126), ex - 1).clamp(min=-126)
    return torch.ldexp(torch.ones_like(r), e - 8)


def _bound(ref, slack):
    """half_ulp_bf16(ref) + slack, slack widened by what the half-spacing gains where |ref| + slack
    lies in a higher binade than ref (the rounding acts on the fp32 value, not on ref)."""
    return slack + half_ulp_bf16(ref.abs() + slack)


def bits16(t):
    return t.contiguous().view(torch.int16)


def bits32(t):
    return t.contiguous().view(torch.int32)


def all_bf16_patterns():
    """All 65,536 bf16 bit patterns, pattern i at index i."""
    i = torch.arange(65536, dtype=torch.int32)
    return torch.where(i >= 32768, i - 65536, i).to(torch.int16).view(torch.bfloat16)


def _ratio(out, ref, bound):
    """|out - ref| / bound per element, 0 / 0 = 0, inf where out is not finite."""
    o = out.double()
    err = (o - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, math.inf))


def slack_used(out, ref, bound):
    """The largest share of the slack that an element needs: (|out - ref| - half_ulp_bf16(ref)) /
    (bound - half_ulp_bf16(ref)), at least 0.  error / bound sits at 1.000 wherever a value falls
    next to a rounding tie, whatever the slack; this figure says how near the fp32 part of the
    bound the arithmetic came.  A measurement for the changelog, never asserted."""
    hu = half_ulp_bf16(ref)
    o = out.double()
    ok = torch.isfinite(o) & torch.isfinite(bound)
    used = ((o - ref).abs() - hu) / (bound - hu)
    used = torch.where(ok, used, torch.zeros_like(used)).clamp(min=0.0)
    return float(used.max()) if used.numel() else 0.0


# ---- add + LayerNorm -----------------------------------------------------------------------------
LN_DIMS = (1, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 767, 768, 769, 1000, 1023, 1024)
LN_ROWS = (1, 3, 4, 5, 9)
LN_EPS = (1e-5, 1e-6, 1e-12)
LN_SUITES = ("spread", "offset", "tiny", "outlier", "zeros", "pow2")
LN_EXACT_SUITES = ("zeros", "pow2")


def ln_suites(dim):
    """The suites that exist at this dim (`pow2` at the power-of-two dims only)."""
    return tuple(s for s in LN_SUITES if s != "pow2" or dim & (dim - 1) == 0)


def ln_inputs(suite, rows, dim, seed):
    """(x fp32 (rows, dim), delta bf16 (rows, dim), gamma fp32 (dim), beta fp32 (dim)): random
    gamma and beta, a distinct delta per row, and x by suite:
      spread   0.5 + 3 N(0,1), delta N(0,1);
      offset   300 + 0.05 N(0,1) — a mean 6000 times the spread — delta 0.05 N(0,1);
      tiny     1e-3 N(0,1), delta 1e-3 N(0,1): the variance is below eps = 1e-5 and near 1e-6;
      outlier  N(0,1) with one element of 1e4 per row, delta N(0,1);
      zeros    x = 0 and delta = 0;
      pow2     x = delta = 2^(k - 1), a constant row (k = -3..3 by row) — with or without the
               delta the updated row is one power of two; power-of-two dims only."""
    g = _gen(LN_SUITES.index(suite), rows, dim, seed)
    gamma = torch.randn(dim, generator=g)
    beta = torch.randn(dim, generator=g)
    nx = torch.randn(rows, dim, generator=g)
    nd = torch.randn(rows, dim, generator=g)
    if suite == "spread":
        x, delta = 0.5 + 3.0 * nx, nd
    elif suite == "offset":
        x, delta = 300.0 + 0.05 * nx, 0.05 * nd
    elif suite == "tiny":
        x, delta = 1e-3 * nx, 1e-3 * nd
    elif suite == "outlier":
        x, delta = nx, nd
        col = torch.randint(0, dim, (rows,), generator=g)
        x[torch.arange(rows), col] = 1e4
    elif suite == "zeros":
        x, delta = torch.zeros(rows, dim), torch.zeros(rows, dim)
    elif suite == "pow2":
        if dim & (dim - 1):
            raise ValueError("the pow2 suite exists at power-of-two dims only")
        k = (torch.arange(rows) % 7 - 3).float()
        x = torch.exp2(k - 1)[:, None].expand(rows, dim).clone()
        delta = x.clone()
    else:
        raise ValueError(suite)
    return x.float().contiguous(), delta.bfloat16().contiguous(), gamma, beta


def residual_reference(x, delta):
    """The fp32 sum x + float(delta) on the CPU (delta None: x itself).  The kernel's update of x
    equals it bit for bit."""
    x = x.detach().cpu().float()
    return x.clone() if delta is None else x + delta.detach().cpu().float()


def _eps32(eps):
    return float(torch.tensor(eps, dtype=torch.float32))


def _ln_stats(x_new, eps):
    v = x_new.double()
    mu = v.mean(-1, keepdim=True)
    d = v - mu
    var = (d * d).mean(-1, keepdim=True)
    return v, d, var, var + _eps32(eps)


def layernorm_reference(x_new, gamma, beta, eps):
    """float64 LayerNorm (biased variance, eps as fp32) of the fp32 rows x_new."""
    _, d, _, w = _ln_stats(x_new, eps)
    return d / w.sqrt() * gamma.double() + beta.double()


def layernorm_bound(x_new, gamma, beta, eps):
    """half_ulp_bf16(ref) + slack per element (module docstring); inf where the relative error of
    var + eps cannot be bounded below 1/2."""
    v, d, var, w = _ln_stats(x_new, eps)
    gam, bet = gamma.double().abs(), beta.double().abs()
    a = v.abs().mean(-1, keepdim=True)
    em = _g(23) * a
    f = U * (v.abs() + a + em)
    e = em + f
    f2 = (f * f).mean(-1, keepdim=True)
    dv = em * em + f2 + 2.0 * (var * f2).sqrt() + 2.0 * em * f.mean(-1, keepdim=True)
    dw = (dv + _g(22) * (var + dv) + 2.0 * U * (w + dv)) / w
    ok = dw < 0.5
    rho = torch.where(ok, dw / (2.0 * (1.0 - dw)), torch.zeros_like(dw)) + 2.0 ** -23
    r = 1.0 / w.sqrt()
    et = r * (e + (d.abs() + e) * (rho + U + rho * U))
    slack = gam * et + U * ((d * r).abs() * gam + gam * et + bet) + 2.0 ** -149
    ref = d * r * gamma.double() + beta.double()
    bound = _bound(ref, slack)
    return torch.where(ok.expand_as(bound), bound, torch.full_like(bound, math.inf))


def check_add_layernorm(x_after, y, x_before, delta, gamma, beta, eps, suite=None):
    """All checks of one vit_add_layernorm_bf16 call, CPU tensors: the residual bit for bit
    (unchanged bit for bit when delta is None), y within layernorm_bound of the float64
    reference, and y == bf16(beta) bit for bit in the exact cases (dim = 1, `zeros`, `pow2`).
    Returns (the worst error / bound, slack_used)."""
    want_x = residual_reference(x_before, delta)
    nbad = int((bits32(x_after) != bits32(want_x)).sum())
    assert nbad == 0, f"residual: {nbad} of {want_x.numel()} fp32 values differ from x + float(delta)"
    ref = layernorm_reference(want_x, gamma, beta, eps)
    bound = layernorm_bound(want_x, gamma, beta, eps)
    ratio = _ratio(y, ref, bound)
    worst = float(ratio.max())
    assert worst <= 1.0, f"LayerNorm: error / bound = {worst:.4g} (suite {suite}, eps {eps})"
    if suite in LN_EXACT_SUITES or x_before.shape[-1] == 1:
        want = beta.bfloat16().expand_as(y)
        nbad = int((bits16(y) != bits16(want)).sum())
        assert nbad == 0, f"exact probe ({suite}): {nbad} outputs are not bf16(beta)"
    return worst, slack_used(y, ref, bound)


LN_MUTANTS = ("pad_dim", "drop_last_col", "unbiased_var", "eps_outside", "no_eps", "onepass_var",
              "swap_pair", "trunc_out", "gamma_by_lane", "delta_prev_row")


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _trunc_bf16(t):
    return (bits32(t.float()) >> 16).to(torch.int16).view(torch.bfloat16)


def _swap_pairs(n):
    """Index map exchanging 2i and 2i + 1 for every pair that lies below n."""
    i = torch.arange(n)
    return torch.where((i ^ 1) < n, i ^ 1, i)


def emulate_add_layernorm(x, delta, gamma, beta, eps, mutant=None):
    """add_ln_kernel's arithmetic on any device; returns (x_new fp32, y bf16).

    mutant: "pad_dim" — mean and variance divided by 64 * ceil(dim / 64); "drop_last_col" —
    column dim - 1 left out of the sums and not written (it keeps the guard pattern);
    "unbiased_var"; "eps_outside" — 1 / (sqrt(var) + eps); "no_eps"; "onepass_var" — E[x^2] -
    mean^2 in fp32; "swap_pair" — delta elements 2i and 2i + 1 exchanged, the wrong half of the
    packed word; "trunc_out" — truncation to bf16; "gamma_by_lane" — gamma[c % 64];
    "delta_prev_row" — row r takes the delta of row r - 1 (row 0 the last row's)."""
    assert mutant is None or mutant in LN_MUTANTS, mutant
    x = x.float()
    rows, dim = x.shape
    dev = x.device
    if delta is None:
        xn = x.clone()
    else:
        dl = delta.float()
        if mutant == "swap_pair":
            dl = dl[:, _swap_pairs(dim).to(dev)]
        if mutant == "delta_prev_row":
            dl = dl.roll(1, 0)
        xn = x + dl
    used = dim - 1 if mutant == "drop_last_col" else dim
    per = (dim + 63) // 64
    div = torch.tensor(float(64 * per if mutant == "pad_dim" else dim), dtype=torch.float32, device=dev)
    mask = (torch.arange(per * 64, device=dev) < used)

    def lanes(t):                                   # (rows, dim) -> (rows, per, 64), zero padded
        p = torch.zeros(rows, per * 64, dtype=torch.float32, device=dev)
        p[:, :dim] = t
        return (p * mask).view(rows, per, 64)

    v = lanes(xn)
    s = torch.zeros(rows, 64, dtype=torch.float32, device=dev)
    for i in range(per):
        s = s + v[:, i]
    mean = (s.sum(-1, keepdim=True) / div)
    d = (v.view(rows, -1) - mean) * mask
    dd = d.view(rows, per, 64)
    q = torch.zeros(rows, 64, dtype=torch.float32, device=dev)
    for i in range(per):
        q = _fma(dd[:, i], dd[:, i], q)
    var = q.sum(-1, keepdim=True) / div
    if mutant == "unbiased_var":
        var = q.sum(-1, keepdim=True) / torch.tensor(float(dim - 1), dtype=torch.float32, device=dev)
    if mutant == "onepass_var":
        s2 = torch.zeros(rows, 64, dtype=torch.float32, device=dev)
        for i in range(per):
            s2 = _fma(v[:, i], v[:, i], s2)
        var = s2.sum(-1, keepdim=True) / div - mean * mean
    e32 = torch.tensor(eps, dtype=torch.float32, device=dev)
    if mutant == "eps_outside":
        rstd = 1.0 / (var.sqrt() + e32)
    elif mutant == "no_eps":
        rstd = torch.rsqrt(var)
    else:
        rstd = torch.rsqrt(var + e32)
    gam = gamma.float()
    if mutant == "gamma_by_lane":
        gam = gam[torch.arange(dim, device=dev) % 64]
    yf = _fma((xn - mean) * rstd, gam, beta.float())
    y = _trunc_bf16(yf) if mutant == "trunc_out" else yf.bfloat16()
    if mutant == "drop_last_col":
        y = y.clone()
        bits16(y)[:, dim - 1] = NAN_BITS
    return xn, y


# ---- GELU and QuickGELU --------------------------------------------------------------------------
def gelu_reference(h):
    """float64 0.5 a erfc(-a / sqrt 2) (= 0.5 a (1 + erf(a / sqrt 2)) without the cancellation)."""
    a = h.double()
    return 0.5 * a * torch.special.erfc(-a * SQRT1_2)


def gelu_bound(h):
    a = h.double()
    z = a * SQRT1_2
    erf, erfcm = torch.erf(z), torch.special.erfc(-z)
    d_arg = 2.5 * U * z.abs() * (2.0 / math.sqrt(math.pi)) * torch.exp(-z * z)
    d_fn = ERFF_ULP * 2.0 * U * erf.abs()
    dw = d_arg + d_fn + U * (erfcm + d_arg + d_fn)
    ref = 0.5 * a * erfcm
    slack = 0.5 * a.abs() * dw * (1.0 + U) + U * ref.abs() + 2.0 ** -149
    return _bound(ref, slack)


def quick_gelu_reference(h):
    """float64 a / (1 + exp(-1.702 a))."""
    a = h.double()
    return a / (1.0 + torch.exp(-1.702 * a))


T_NEAR_OVERFLOW = 126.0 * math.log(2.0)
T_OVERFLOWED = 130.0 * math.log(2.0)


def quick_gelu_bound(h):
    a = h.double()
    t = -1.702 * a
    ref = quick_gelu_reference(h)
    e_e = torch.expm1((4.0 * U * (1.0 + 2.0 ** -20) * t.abs()).clamp(max=1.0)) * (1.0 + 2.0 * U) + 2.0 * U
    share = torch.sigmoid(t)                                  # E / (1 + E)
    e_s = e_e * share + U * (1.0 + e_e * share)
    rel = (1.0 + U) / (1.0 - e_s) - 1.0
    slack = ref.abs() * rel + 2.0 ** -126
    near = a.abs() * 2.0 ** -125 * (1.0 + 2.0 ** -20)
    big = 2.0 ** -126 + ref.abs() + torch.where(t < T_OVERFLOWED, near, torch.zeros_like(near))
    return _bound(ref, torch.where(t >= T_NEAR_OVERFLOW, big, slack))


def activation_ratio(out, h, kind):
    """Per element of the bf16 input h, how far the bf16 output is from what it may be, as error /
    bound for a finite input (kind "gelu" or "quick_gelu"); for the others 0 if the rule holds and
    inf if not: NaN -> NaN, +inf -> +inf, -inf -> the bf16 rounding of torch's fp32 op on the CPU
    (NaN).  One ratio per input element: nothing is left out."""
    ref, bound = {"gelu": (gelu_reference, gelu_bound),
                  "quick_gelu": (quick_gelu_reference, quick_gelu_bound)}[kind]
    a, o = h.double(), out.double()
    fin = torch.isfinite(a)
    safe = torch.where(fin, h, torch.zeros_like(h))
    ratio = _ratio(out, ref(safe), bound(safe))
    ninf = torch.tensor([-math.inf])
    rule = (torch.nn.functional.gelu(ninf) if kind == "gelu" else ninf * torch.sigmoid(1.702 * ninf))
    rule = rule.bfloat16().double().to(a.device)
    same = lambda x, y: (x == y) | (torch.isnan(x) & torch.isnan(y))
    good = torch.where(torch.isnan(a), torch.isnan(o),
                       torch.where(a > 0, o == math.inf, same(o, rule.expand_as(o))))
    special = torch.where(good, torch.zeros_like(ratio), torch.full_like(ratio, math.inf))
    ratio = torch.where(fin, ratio, special)
    assert ratio.numel() == h.numel()
    return ratio


def activation_slack_used(out, h, kind):
    """slack_used over the finite inputs of h."""
    ref, bound = {"gelu": (gelu_reference, gelu_bound),
                  "quick_gelu": (quick_gelu_reference, quick_gelu_bound)}[kind]
    fin = torch.isfinite(h.double())
    return slack_used(out[fin], ref(h[fin]), bound(h[fin]))


GELU_MUTANTS = ("tanh_form", "swap_pair", "trunc_out", "tail_skipped")
QUICK_GELU_MUTANTS = ("k17", "swap_pair", "trunc_out", "tail_skipped")
GELU_GROUP, QUICK_GELU_GROUP = 16, 8             # elements per thread of the vector branch


def _finish_activation(h, yf, mutant, group):
    y = _trunc_bf16(yf) if mutant == "trunc_out" else yf.bfloat16()
    n = h.numel()
    if mutant == "swap_pair":
        y = y[_swap_pairs(n).to(h.device)]
    if mutant == "tail_skipped" and n % group:
        y = torch.cat([y[:n - n % group], h[n - n % group:]])
    return y


def emulate_gelu(h, mutant=None):
    """gelu_kernel's arithmetic on a 1-d bf16 tensor.  mutant: "tanh_form" — 0.5 a (1 + tanh(
    sqrt(2 / pi) (a + 0.044715 a^3))); "swap_pair" — outputs 2i and 2i + 1 exchanged; "trunc_out";
    "tail_skipped" — the last n % 16 elements left as they were."""
    assert mutant is None or mutant in GELU_MUTANTS, mutant
    a = h.float()
    if mutant == "tanh_form":
        inner = torch.tensor(math.sqrt(2.0 / math.pi), dtype=torch.float32) * (a + 0.044715 * a * a * a)
        yf = (0.5 * a) * (1.0 + torch.tanh(inner))
    else:
        yf = (0.5 * a) * (1.0 + torch.erf(a * torch.tensor(SQRT1_2, dtype=torch.float32)))
    return _finish_activation(h, yf, mutant, GELU_GROUP)


def emulate_quick_gelu(h, mutant=None):
    """quick_gelu_kernel's arithmetic on a 1-d bf16 tensor.  mutant: "k17" — 1.7 for 1.702;
    "swap_pair"; "trunc_out"; "tail_skipped" — the last n % 8 elements left as they were."""
    assert mutant is None or mutant in QUICK_GELU_MUTANTS, mutant
    a = h.float()
    k = torch.tensor(-1.7 if mutant == "k17" else -1.702, dtype=torch.float32)
    e = torch.exp2((k * a) * torch.tensor(LOG2E_F, dtype=torch.float32))
    return _finish_activation(h, a / (1.0 + e), mutant, QUICK_GELU_GROUP)


# ---- patchify and tokens -------------------------------------------------------------------------
PATCHIFY_SHAPES = ((2, 16, 32, 8), (2, 32, 16, 8), (1, 32, 48, 16), (3, 48, 24, 24), (1, 32, 64, 32),
                   (1, 8, 8, 8))
TOKENS_SHAPES = ((3, 5, 12), (1, 0, 4), (2, 7, 260), (1, 1, 768))
TOWER_MEAN = (0.48145466, 0.4578275, 0.40821073)
TOWER_STD = (0.26862954, 0.26130258, 0.27577711)


def patchify_inputs(b, h, w, seed=0):
    """A distinct random image batch in [0, 1] and the tower's mean and std, fp32."""
    img = torch.rand(b, 3, h, w, generator=_gen(b, h, w, seed))
    return img, torch.tensor(TOWER_MEAN), torch.tensor(TOWER_STD)


def patchify_reference(img, mean, std, p):
    """bf16((img - mean[c]) / std[c]) as patches (b, (h/p)(w/p), 3 p p), each laid out (c, kh, kw):
    the fp32 torch ops on the CPU."""
    img = img.detach().cpu().float()
    b, c, h, w = img.shape
    x = ((img - mean.cpu().float().view(1, 3, 1, 1)) / std.cpu().float().view(1, 3, 1, 1)).bfloat16()
    x = x.reshape(b, c, h // p, p, w // p, p).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(b, (h // p) * (w // p), c * p * p).contiguous()


PATCHIFY_MUTANTS = ("swap_hw", "khkwc")


def emulate_patchify(img, mean, std, p, mutant=None):
    """patchify_kernel's index arithmetic, one gather per output element.  mutant: "swap_hw" — the
    patch-grid width taken from H (an address past the image wraps around here); "khkwc" — the
    patch laid out (kh, kw, c)."""
    assert mutant is None or mutant in PATCHIFY_MUTANTS, mutant
    img = img.float()
    b, _, hh, ww = img.shape
    gw = (hh if mutant == "swap_hw" else ww) // p
    npatch, pe = (hh // p) * (ww // p), 3 * p * p
    i = torch.arange(b * npatch * pe, device=img.device)
    e, bp = i % pe, i // pe
    pi, bi = bp % npatch, bp // npatch
    if mutant == "khkwc":
        c, kh, kw = e % 3, e // (3 * p), (e // 3) % p
    else:
        c, kh, kw = e // (p * p), (e // p) % p, e % p
    ph, pw = pi // gw, pi % gw
    src = ((bi * 3 + c) * hh + ph * p + kh) * ww + pw * p + kw
    val = (img.reshape(-1)[src % img.numel()] - mean.float().to(img.device)[c]) / std.float().to(img.device)[c]
    return val.bfloat16().view(b, npatch, pe)


def tokens_inputs(b, npatch, dim, seed=0):
    g = _gen(b, npatch, dim, seed)
    pe = torch.randn(b, npatch, dim, generator=g).bfloat16()
    return pe, torch.randn(1, 1, dim, generator=g), torch.randn(1, npatch + 1, dim, generator=g)


def tokens_reference(pe, cls, pos):
    """cat(cls, float(pe)) + pos, the fp32 torch ops on the CPU: (b, npatch + 1, dim) fp32."""
    pe, cls, pos = pe.detach().cpu(), cls.detach().cpu().float(), pos.detach().cpu().float()
    return torch.cat([cls.expand(pe.shape[0], -1, -1), pe.float()], 1) + pos
