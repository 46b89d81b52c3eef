"""CPU proof that the attention checks of tests/vit_check.py can fail: an emulation of
vit_attn.hip's arithmetic passes the derived bound (C1) and the three exact probes (C2) at every
token count 1..256, and the same emulation with one planted mistake — a padded key in the
denominator, a dropped key, two exchanged V rows — is rejected by at least one probe at every
token count.  Also the C ABI surface of the split-count entry points.  No GPU compute.
"""
import re
from pathlib import Path

import pytest
import torch

from image_recommender_amd import _lib
from tests import vit_check as vc

ROOT = Path(__file__).resolve().parents[1]
SCALE = 0.125
ALL_NTOK = range(1, 257)


def test_split_abi_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "imgrec_vit.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ("vit_linear_bf16_split", "vit_linear_splits"):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared in imgrec_vit.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported by the library"
    # argument validation comes before any device call
    assert lib.vit_linear_splits(0, 256) == -1 and lib.vit_linear_splits(10, 200) == -1
    assert lib.vit_linear_bf16_split(None, None, None, 10, 64, 256, 0, 1, None, None) == -1


def _probes(n):
    """name -> (qkv, checker of an output) for the three probes at ntok = n, one image, one head."""
    cq = vc.probe_constant_v(1, n, 1, seed=n)
    iq = vc.probe_indicator_v(1, n, 1, seed=n)
    oq, perm = vc.probe_one_hot(1, n, 1, seed=n)
    return {"constant": (cq, vc.check_constant_v),
            "indicator": (iq, lambda out: vc.check_indicator_v(out, n)),
            "one_hot": (oq, lambda out: vc.check_one_hot(out, oq, perm, 1))}


def _rejected(check, out):
    try:
        check(out)
    except AssertionError:
        return True
    return False


@pytest.fixture(scope="module")
def probes():
    return {n: _probes(n) for n in ALL_NTOK}


def test_one_hot_keys_keep_their_gap():
    """The construction the one-hot probe rests on: pairwise dots <= 32 among the +-1 key rows, so
    the logit gap at scale 1/8 is >= 8 * (64 - 32) / 8 = 32."""
    for n in (2, 197, 256):
        k = vc.one_hot_keys(n, seed=n)
        dots = k @ k.T - 64 * torch.eye(n)
        assert k.shape == (n, 64) and bool((k.abs() == 1).all()) and float(dots.max()) <= 32


def test_emulation_passes_the_derived_bound():
    """C1 on the unmutated emulation, every ntok, input scales 1.5 and 6 (logits around +-150):
    error / bound <= 1.  This says the bound is attainable by the kernel's arithmetic; it measures
    the emulation, not the kernel."""
    worst = 0.0
    for n in ALL_NTOK:
        for scale_in in (1.5, 6.0):
            qkv = vc.random_qkv(2, n, 3, seed=7 * n + int(scale_in), scale=scale_in)
            out = vc.emulate_attention(qkv, 3, SCALE)
            r = vc.worst_ratio(out, qkv, 3, SCALE)
            assert r <= 1.0, (n, scale_in, r)
            worst = max(worst, r)
    print(f"[vit_check] emulation's worst error / bound over ntok 1..256: {worst:.3f}")
    assert worst > 0.25          # a bound nothing comes near would check nothing


def test_bound_rejects_a_wrong_key_count_only_when_it_is_large():
    """What the issue observed and why C2 exists: at ntok = 197 one padded key in the denominator
    stays inside the derived bound on random inputs (so no random-input tolerance sees it), while
    at ntok = 2 the same mistake is far outside."""
    qkv = vc.random_qkv(2, 197, 3, seed=1)
    assert vc.worst_ratio(vc.emulate_attention(qkv, 3, SCALE, "pad"), qkv, 3, SCALE) <= 1.0
    qkv = vc.random_qkv(2, 2, 3, seed=1)
    assert vc.worst_ratio(vc.emulate_attention(qkv, 3, SCALE, "pad"), qkv, 3, SCALE) > 1.0


def test_emulation_passes_every_probe(probes):
    for n in ALL_NTOK:
        for name, (qkv, check) in probes[n].items():
            out = vc.emulate_attention(qkv, 1, SCALE)
            assert not _rejected(check, out), (n, name)
            assert vc.worst_ratio(out, qkv, 1, SCALE) <= 1.0, (n, name)


def test_probes_hold_with_several_images_and_heads():
    """The probes and their checkers in the shape the GPU test uses them (2 images, 3 heads)."""
    for n in (17, 197):
        vc.check_constant_v(vc.emulate_attention(vc.probe_constant_v(2, n, 3, seed=n), 3, SCALE))
        vc.check_indicator_v(vc.emulate_attention(vc.probe_indicator_v(2, n, 3, seed=n), 3, SCALE), n)
        qkv, perm = vc.probe_one_hot(2, n, 3, seed=n)
        vc.check_one_hot(vc.emulate_attention(qkv, 3, SCALE), qkv, perm, 3)
        with pytest.raises(AssertionError):
            vc.check_one_hot(vc.emulate_attention(qkv, 3, SCALE, "swap_v"), qkv, perm, 3)


@pytest.mark.parametrize("mutant", vc.MUTANTS)
def test_every_mutant_is_rejected_by_a_probe(probes, mutant):
    """Per ntok, which probes reject the mutant; at least one must.  The constant probe is the one
    for a padded key, the indicator probe for a dropped key.  Uniform attention (q = 0) is blind to
    a V-row exchange by construction — the sum over rows does not depend on their order — so that
    mutant is left to the one-hot probe, which pins every row; at ntok = 1 there is no second row
    to exchange and the mutant is the identity."""
    seen = {name: 0 for name in ("constant", "indicator", "one_hot")}
    for n in ALL_NTOK:
        if mutant == "swap_v" and n == 1:
            continue
        hits = [name for name, (qkv, check) in probes[n].items()
                if _rejected(check, vc.emulate_attention(qkv, 1, SCALE, mutant))]
        assert hits, (mutant, n)
        for name in hits:
            seen[name] += 1
    print(f"[vit_check] {mutant}: rejected by {seen}")
    if mutant == "pad":
        assert seen["constant"] == 256
    if mutant.startswith("drop"):
        assert seen["indicator"] == 256
    if mutant == "swap_v":
        assert seen["one_hot"] == 255 and seen["constant"] == 0 and seen["indicator"] == 0
