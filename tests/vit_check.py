"""Checks of vit_attention_bf16 (csrc/vit_attn.hip) shared by the GPU tests
(tests/test_vit_attn_gpu.py, tests/test_vit_fused_gpu.py) and by their CPU proof
(tests/test_vit_check_cpu.py).  torch only; every function runs on the CPU or the GPU.

Three things live here:

* the float64 reference of softmax(q k^T * scale) v and the error bound derived from the kernel's
  arithmetic (`attention_reference`, `attention_bound`, `worst_ratio`);
* three exact probes — inputs on which the right answer is known to the bit or to one bf16
  rounding, so that a mistake of one key cannot hide in a tolerance (`probe_constant_v`,
  `probe_indicator_v`, `probe_one_hot` and their `check_*`);
* an emulation of the kernel's arithmetic with switches for the mistakes such a kernel typically
  has (`emulate_attention`), which the CPU test uses to show that the probes can fail.

The bound.  From bf16 q, k, v the kernel computes, per query row,
    out = bf16( (sum_j bf16(p_j) v_j) * (1 / sum_j p_j) ),  p_j = exp2(s_j * scale_log2 - m)
with fp32 scores s_j, m = max_j s_j * scale_log2, fp32 sums.  Against ref = P v (P the exact
softmax, float64) and A = P |v|:
  * the output's rounding to bf16 (8 significant bits, unit roundoff 2^-8):   2^-8 |ref| (to first
    order; the second-order part is inside the slack of the next term, which over-counts: the
    mean rounding error of P is half its worst case);
  * the rounding of every p_j to bf16, |bf16(p_j) - p_j| <= 2^-8 p_j, summed against |v_j| and
    divided by the unrounded sum:                                             2^-8 A;
  * fp32: the exponent s_j * scale_log2 - m carries an absolute error of about 2^-23 smax
    (smax = max_j |s_j * scale| of the row), which is a relative error of p_j; exp2, the
    reciprocal and the two sums add a few 2^-24 relative:                     2^-22 (1 + smax) A.
So |out - ref| <= 2^-8 (|ref| + A) + 2^-22 (1 + smax) A, per element, with nothing taken from the
kernel's own output.
"""
import math

import torch

HD = 64
NAN_BITS = 0x7FC0                     # the bf16 quiet NaN the output buffers are pre-filled with
LOG2E = 1.4426950408889634


# ---- layout ------------------------------------------------------------------------------------
def pack_qkv(q, k, v):
    """(b, heads, n, 64) q, k, v -> the qkv Linear's output layout (b, n, 3 * heads * 64) bf16."""
    b, h, n, d = q.shape
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4)          # (b, n, 3, h, d)
    return qkv.reshape(b, n, 3 * h * d).to(torch.bfloat16).contiguous()


def unpack_qkv(qkv, heads):
    """(b, n, 3 * heads * 64) -> q, k, v as (b, heads, n, 64) views of the same values."""
    b, n, _ = qkv.shape
    return qkv.view(b, n, 3, heads, HD).permute(2, 0, 3, 1, 4).unbind(0)


def unpack_out(out, heads):
    """(b, n, heads * 64) -> (b, heads, n, 64)."""
    b, n, _ = out.shape
    return out.view(b, n, heads, HD).permute(0, 2, 1, 3)


# ---- C1: float64 reference and the derived bound -------------------------------------------------
def attention_reference(qkv, heads, scale):
    """(ref, A, smax) in float64, each in out's layout (b, n, heads * 64) (smax broadcast over the
    64 dims of its head): ref = P v, A = P |v|, smax = max_j |q . k_j * scale| of the query row."""
    q, k, v = (t.double() for t in unpack_qkv(qkv, heads))
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(s, dim=-1)
    ref, a = p @ v, p @ v.abs()
    smax = s.abs().amax(dim=-1, keepdim=True).expand_as(ref)
    b, _, n, _ = ref.shape
    lay = lambda t: t.permute(0, 2, 1, 3).reshape(b, n, heads * HD)
    return lay(ref), lay(a), lay(smax)


def attention_bound(ref, a, smax):
    return 2.0 ** -8 * (ref.abs() + a) + 2.0 ** -22 * (1.0 + smax) * a


def worst_ratio(out, qkv, heads, scale):
    """max |out - ref| / bound over all elements (0 / 0 counts as 0: an exact zero is within a
    zero bound); NaN or inf in out gives inf."""
    ref, a, smax = attention_reference(qkv, heads, scale)
    err = (out.double() - ref).abs()
    bound = attention_bound(ref, a, smax)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(out.double()), ratio, torch.full_like(ratio, math.inf))
    return float(ratio.max())


def random_qkv(b, n, heads, seed, scale=1.5, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(b, n, 3 * heads * HD, generator=g) * scale).bfloat16().to(device)


# ---- C2: exact probes ----------------------------------------------------------------------------
PROBE_NTOK = (1, 15, 16, 17, 31, 33, 100, 197, 208, 255, 256)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def probe_constant_v(b, n, heads, seed=0):
    """q = 0, random k, v = 1: uniform attention over ones.  out == 1.0 exactly: every p_j is 1,
    the sum is n, and n * fl(1 / n) rounds to 1 in bf16.  A padded key in the denominator gives
    n / (n + pads) <= 256 / 257 < 1 - 2^-9, which never rounds to 1."""
    k = _randn((b, heads, n, HD), seed) * 1.5
    return pack_qkv(torch.zeros_like(k), k, torch.ones_like(k))


def check_constant_v(out):
    assert torch.equal(out.float(), torch.ones_like(out, dtype=torch.float32)), \
        f"constant-V probe: {int((out.float() != 1).sum())} outputs are not 1.0"


def probe_indicator_v(b, n, heads, seed=0):
    """q = 0, random k, v[j] = e_(j mod 64): out[:, c] is the share of keys with j mod 64 == c."""
    k = _randn((b, heads, n, HD), seed) * 1.5
    v = torch.zeros_like(k)
    j = torch.arange(n)
    v[:, :, j, j % HD] = 1.0
    return pack_qkv(torch.zeros_like(k), k, v)


def check_indicator_v(out, n):
    """Within 2^-8 relative of count_c / n (one bf16 rounding of count_c * fl(1 / n), <= 2^-9 +
    2^-23).  A dropped or doubled key moves a count of at most 4 (ntok <= 256) by 1: a fifth of
    its share at the least."""
    count = torch.bincount(torch.arange(n) % HD, minlength=HD).double().to(out.device)
    want = count / n
    err = (out.double().reshape(*out.shape[:-1], -1, HD) - want).abs()       # (b, n, heads, 64)
    bad = ~(err <= 2.0 ** -8 * want)                         # NaN counts as bad
    assert not bool(bad.any()), f"indicator-V probe: {int(bad.sum())} shares off count / ntok"


def one_hot_keys(n, seed=0):
    """n rows of +-1 (64 dims) whose pairwise dot products are all <= 32: drawn one at a time, a
    row that comes closer to an earlier one is drawn again (about 4 sigma: rare)."""
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    rows = torch.empty(0, HD)
    while rows.shape[0] < n:
        r = (torch.randint(0, 2, (HD,), generator=g) * 2 - 1).float()
        if rows.shape[0] == 0 or float((rows @ r).max()) <= 32:
            rows = torch.cat([rows, r[None]], 0)
    return rows


def probe_one_hot(b, n, heads, seed=0):
    """k rows of +-1 with pairwise dots <= 32, q[i] = 8 k[perm[i]], random bf16 v; returns (qkv,
    perm) with perm (b, heads, n).  At scale 1/8 the logit of key perm[i] is 64 and every other
    at most 32, so the other probabilities are below e^-32 < 1.3e-14 and the output is v[perm[i]]
    bit for bit (255 such keys move a sum by < 2^-38 relative; bf16 keeps 2^-9)."""
    g = torch.Generator(device="cpu").manual_seed(2000 + seed)
    k = torch.stack([one_hot_keys(n, seed + i) for i in range(b * heads)]).view(b, heads, n, HD)
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(b * heads)]).view(b, heads, n)
    q = 8.0 * torch.gather(k, 2, perm[..., None].expand(-1, -1, -1, HD))
    v = (torch.randn(b, heads, n, HD, generator=g) * 1.5).bfloat16().float()
    return pack_qkv(q, k, v), perm


def check_one_hot(out, qkv, perm, heads):
    v = unpack_qkv(qkv, heads)[2]
    want = torch.gather(v, 2, perm.to(v.device)[..., None].expand(-1, -1, -1, HD))
    got = unpack_out(out, heads)
    same = got.contiguous().view(torch.int16) == want.contiguous().view(torch.int16)
    assert bool(same.all()), f"one-hot probe: {int((~same).sum())} outputs differ from v[perm]"


# ---- C3: the kernel's arithmetic, with mutants -----------------------------------------------------
MUTANTS = ("pad", "drop_first", "drop_mid", "drop_last", "swap_v")


def emulate_attention(qkv, heads, scale, mutant=None):
    """vit_attn.hip's arithmetic on any device: fp32 scores, m = max s * scale_log2, p = exp2(fma(s,
    scale_log2, -m)), fp32 row sum, bf16 p into an fp32 P V, times fl(1 / sum), rounded to bf16.
    The accumulation ORDER inside the MFMAs is not emulated (it moves a sum by fp32 ulps).

    mutant: "pad" — one zero-padded key (score 0, v = 0) is counted by the max and the sum, what an
    off-by-one in `kpad + i < ntok` does; "drop_first" / "drop_mid" / "drop_last" — key 0, ntok // 2
    or ntok - 1 is masked out; "swap_v" — V rows r and r ^ 1 are exchanged (every pair that lies
    below ntok), what a wrong row in the transposed V read does."""
    q, k, v = (t.float() for t in unpack_qkv(qkv, heads))
    b, h, n, _ = q.shape
    if mutant == "pad":
        k = torch.cat([k, torch.zeros_like(k[:, :, :1])], 2)
        v = torch.cat([v, torch.zeros_like(v[:, :, :1])], 2)
    elif mutant == "swap_v":
        r = torch.arange(n)
        src = torch.where((r ^ 1) < n, r ^ 1, r)
        v = v[:, :, src]
    s = q @ k.transpose(-1, -2)                                        # fp32
    if mutant in ("drop_first", "drop_mid", "drop_last"):
        j = {"drop_first": 0, "drop_mid": n // 2, "drop_last": n - 1}[mutant]
        s[..., j] = -math.inf
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    m = s.amax(dim=-1, keepdim=True) * sl2                             # fp32 product
    e = (s.double() * sl2.double() - m.double()).float()               # the fma: one rounding
    p = torch.exp2(e)
    inv = 1.0 / p.sum(dim=-1, keepdim=True)
    o = p.bfloat16().float() @ v
    out = (o * inv).bfloat16()
    return out.permute(0, 2, 1, 3).reshape(b, n, h * HD)
