"""vit_attention_bf16 (include/imgrec_vit.h, csrc/vit_attn.hip) through the C ABI against the
float64 softmax(q k^T * scale) v of the same bf16 operands, within the bound derived from the
kernel's arithmetic (tests/vit_check.py: 2^-8 (|ref| + P|v|) + 2^-22 (1 + smax) P|v|), at every
one of the 16 attn_kernel<NKB> instantiations; and on three exact probes, where one key too many,
one too few or a wrong V row cannot hide in a tolerance.  tests/test_vit_check_cpu.py shows on an
emulation of the kernel's arithmetic that each of these checks can fail.

Every call writes into a buffer pre-filled with the bf16 NaN 0x7FC0 that is 256 elements longer
than the output: afterwards the body is finite (every row was written) and the tail untouched.
"""
import ctypes as C

import pytest
import torch

from tests import vit_check as vc

pytestmark = pytest.mark.gpu

TAIL = 256


def _attention(qkv, heads, scale=0.125):
    """vit_attention_bf16 on a GPU qkv (b, n, 3 * heads * 64) -> out (b, n, heads * 64)."""
    from image_recommender_amd import _lib
    b, n, c3 = qkv.shape
    numel = b * n * c3 // 3
    buf = torch.full((numel + TAIL,), vc.NAN_BITS, dtype=torch.int16, device="cuda")
    rc = _lib.load().vit_attention_bf16(C.c_void_p(qkv.data_ptr()), b, n, heads, vc.HD, C.c_float(scale),
                                        C.c_void_p(buf.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((buf[numel:] == vc.NAN_BITS).all()), "the kernel wrote past the end of out"
    out = buf[:numel].view(torch.bfloat16).view(b, n, c3 // 3)
    assert bool(torch.isfinite(out.float()).all()), "an output row was not written"
    return out


def _ratio(b, n, heads, seed, scale_in=1.5, scale=0.125):
    qkv = vc.random_qkv(b, n, heads, seed, scale_in, device="cuda")
    return vc.worst_ratio(_attention(qkv, heads, scale), qkv, heads, scale)


def test_attention_every_instantiation_within_derived_bound(gpu):
    """All 16 attn_kernel<NKB>: the first, the last-but-one and the last token count each serves
    (16 NKB - 15: a single live key in the last block; 16 NKB - 1: one padded key; 16 NKB: none)."""
    for nkb in range(1, 17):
        worst = 0.0
        for n in (16 * nkb - 15, 16 * nkb - 1, 16 * nkb):
            r = _ratio(2, n, 3, seed=100 * nkb + n)
            assert r <= 1.0, (nkb, n, r)
            worst = max(worst, r)
        print(f"[vit_attn] NKB = {nkb:2d}: worst error / bound {worst:.3f}")


def test_attention_more_workgroups_than_resident(gpu):
    """96 images x 12 heads = 1152 workgroups of 4 waves at 3 waves per SIMD: more than the
    device holds at once, so later workgroups reuse LDS and registers of earlier ones."""
    r = _ratio(96, 197, 12, seed=5)
    print(f"[vit_attn] (96, 197, 12): worst error / bound {r:.3f}")
    assert r <= 1.0, r


def test_attention_large_logits(gpu):
    """Inputs at scale 6: logits around +-150, where exp2 overflows without the max subtraction
    and the fp32 error of the exponent (the bound's third term) is at its largest."""
    r = _ratio(2, 197, 3, seed=6, scale_in=6.0)
    print(f"[vit_attn] input scale 6: worst error / bound {r:.3f}")
    assert r <= 1.0, r


def test_attention_other_scale(gpu):
    """scale is an argument of the C ABI, not a constant of the kernel."""
    for n in (50, 197):
        r = _ratio(2, n, 3, seed=7 + n, scale_in=2.0, scale=0.05)
        print(f"[vit_attn] scale 0.05, ntok {n}: worst error / bound {r:.3f}")
        assert r <= 1.0, r


@pytest.mark.parametrize("n", vc.PROBE_NTOK)
def test_attention_exact_probes(gpu, n):
    """Constant V: out == 1.0 exactly (a padded key in the denominator gives <= 256 / 257).
    Indicator V: out[:, c] within one bf16 rounding of count_c / ntok (a dropped or doubled key
    moves a count of at most 4 by 1).  One-hot attention: out == v[perm] bit for bit (the Q-K
    pairing, the swizzled LDS rows and the transposed V read, for every row)."""
    b, heads = 2, 3
    vc.check_constant_v(_attention(vc.probe_constant_v(b, n, heads, seed=n).cuda(), heads))
    vc.check_indicator_v(_attention(vc.probe_indicator_v(b, n, heads, seed=n).cuda(), heads), n)
    qkv, perm = vc.probe_one_hot(b, n, heads, seed=n)
    qkv = qkv.cuda()
    vc.check_one_hot(_attention(qkv, heads), qkv, perm, heads)
