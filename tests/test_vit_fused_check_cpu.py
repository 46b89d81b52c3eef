"""CPU proof that the checks of tests/vit_fused_check.py can fail, and pass when they should: the
emulation of vit_fused.hip's arithmetic stays inside every derived bound and exact probe (add +
LayerNorm at every dim of the GPU test in every suite at every eps; GELU and QuickGELU on all
65,536 bf16 bit patterns), and the same emulation with one planted mistake is rejected at every dim
where the mistake changes the arithmetic.  Also the argument contracts of the five entry points that
return before any launch.  No GPU compute.
"""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from image_recommender_amd import _lib
from tests import vit_fused_check as fc

ROOT = Path(__file__).resolve().parents[1]
ROWS = 5
SEEDS = (0, 1)


def _ln_case(suite, dim, seed, eps, with_delta, mutant=None, rows=ROWS):
    """Run the emulation on one suite and hand everything to the checker the GPU test uses."""
    x, delta, gamma, beta = fc.ln_inputs(suite, rows, dim, seed)
    dl = delta if with_delta else None
    xn, y = fc.emulate_add_layernorm(x, dl, gamma, beta, eps, mutant)
    return fc.check_add_layernorm(xn, y, x, dl, gamma, beta, eps, suite), (xn, y)


def _ln_rejected(suite, dim, seed, eps, mutant):
    try:
        _ln_case(suite, dim, seed, eps, True, mutant)
    except AssertionError:
        return True
    return False


def test_half_ulp_bf16_is_the_grid():
    """Against the grid itself: the distance from a bf16 value to its upper neighbour is twice
    half_ulp_bf16 of it, for normals, subnormals and zero."""
    pat = fc.all_bf16_patterns()[:0x7F7F]                     # the non-negative finite values but the last
    nxt = fc.all_bf16_patterns()[1:0x7F80]
    gap = nxt.double() - pat.double()
    assert torch.equal(gap, 2.0 * fc.half_ulp_bf16(pat.double()))
    assert float(fc.half_ulp_bf16(0.0)) == 2.0 ** -134 and float(fc.half_ulp_bf16(-1.5)) == 2.0 ** -8
    assert float(fc.half_ulp_bf16(2.0 ** -127)) == 2.0 ** -134 and float(fc.half_ulp_bf16(255.9)) == 2.0 ** -1


def test_layernorm_emulation_passes_every_check():
    """Every dim, suite and eps, with and without the delta: error / bound <= 1 and the exact
    probes hold.  This says the derived bound is attainable; it measures the emulation."""
    worst, where, used, used_at = 0.0, None, 0.0, None
    for dim in fc.LN_DIMS:
        for suite in fc.ln_suites(dim):
            for eps in fc.LN_EPS:
                for with_delta in (True, False):
                    (r, su), _ = _ln_case(suite, dim, 0, eps, with_delta)
                    if r > worst:
                        worst, where = r, (dim, suite, eps, with_delta)
                    if su > used:
                        used, used_at = su, (dim, suite, eps, with_delta)
    print(f"[vit_fused_check] add_layernorm emulation: worst error / bound {worst:.3f} at {where}; "
          f"largest share of the slack used {used:.3f} at {used_at}")
    assert 0.25 < worst <= 1.0          # a bound nothing comes near would check nothing


def _identity(mutant, dim):
    """Where a mutant does not change what is computed (asserted below, not assumed)."""
    return {"pad_dim": dim % 64 == 0,             # 64 * ceil(dim / 64) == dim
            "gamma_by_lane": dim <= 64,            # c % 64 == c
            "swap_pair": dim == 1,                 # no second element to exchange with
            "eps_outside": dim == 1,               # v - mean is exactly 0: rstd never matters
            "onepass_var": dim == 1}.get(mutant, False)


@pytest.mark.parametrize("mutant", fc.LN_MUTANTS)
def test_every_layernorm_mutant_is_rejected(mutant):
    """At every dim where the mutant changes the arithmetic at least one suite at one eps rejects
    it; where it changes nothing (pad_dim at multiples of 64, ...) its output is the clean one bit
    for bit.  The dims contain both kinds."""
    hits, same = {}, []
    for dim in fc.LN_DIMS:
        if _identity(mutant, dim):
            for suite in fc.ln_suites(dim):
                _, (xa, ya) = _ln_case(suite, dim, 0, 1e-5, True)
                _, (xb, yb) = _ln_case(suite, dim, 0, 1e-5, True, mutant)
                assert torch.equal(fc.bits32(xa), fc.bits32(xb)) and torch.equal(fc.bits16(ya), fc.bits16(yb))
            same.append(dim)
            continue
        found = [(s, e) for sd in SEEDS for s in fc.ln_suites(dim) for e in fc.LN_EPS
                 if _ln_rejected(s, dim, sd, e, mutant)]
        assert found, f"{mutant} passes every suite at dim {dim}"
        for s, _ in found:
            hits[s] = hits.get(s, 0) + 1
        if dim > 1 and mutant in ("eps_outside", "no_eps"):     # why the tiny suite exists
            assert {("tiny", 1e-5), ("tiny", 1e-6)} <= set(found), (mutant, dim)
        if mutant == "onepass_var":                             # and the offset suite
            assert {s for s, _ in found} == {"offset"}, (mutant, dim)
    print(f"[vit_fused_check] {mutant}: rejected by {hits}; identity at dims {same}")
    if mutant == "pad_dim":
        assert same == [d for d in fc.LN_DIMS if d % 64 == 0] and len(same) < len(fc.LN_DIMS)


@pytest.mark.parametrize("kind", ["gelu", "quick_gelu"])
def test_activation_emulation_passes_on_every_bf16_pattern(kind):
    emu = fc.emulate_gelu if kind == "gelu" else fc.emulate_quick_gelu
    h = fc.all_bf16_patterns()
    ratio = fc.activation_ratio(emu(h), h, kind)
    assert ratio.numel() == 65536
    worst = float(ratio.max())
    at = int(ratio.argmax())
    print(f"[vit_fused_check] {kind} emulation: worst error / bound {worst:.3f} at pattern {at:#06x}; "
          f"largest share of the slack used {fc.activation_slack_used(emu(h), h, kind):.3f}")
    assert 0.25 < worst <= 1.0


@pytest.mark.parametrize("kind,mutant", [("gelu", m) for m in fc.GELU_MUTANTS] +
                         [("quick_gelu", m) for m in fc.QUICK_GELU_MUTANTS])
def test_every_activation_mutant_is_rejected(kind, mutant):
    """The exhaustive sweep rejects every mutant (tail_skipped at a length with a tail: 65,531
    patterns, rotated so that the tail holds values near 2 and not NaNs).  tanh_form and k17 differ from the right formula by less than a bf16 half-ulp
    at most inputs and are caught because the bound is the half-ulp of ref, not 2^-8 |ref|: some
    values land on the other side of a rounding boundary."""
    emu = fc.emulate_gelu if kind == "gelu" else fc.emulate_quick_gelu
    h = fc.all_bf16_patterns()
    if mutant == "tail_skipped":
        h = h.roll(-0x4000)[:65531].contiguous()
    ratio = fc.activation_ratio(emu(h, mutant), h, kind)
    nbad = int((ratio > 1.0).sum())
    print(f"[vit_fused_check] {kind} {mutant}: {nbad} of {h.numel()} patterns rejected")
    assert nbad > 0
    if mutant == "tail_skipped":
        group = fc.GELU_GROUP if kind == "gelu" else fc.QUICK_GELU_GROUP
        assert not bool((ratio[:h.numel() - h.numel() % group] > 1.0).any())


def test_patchify_emulation_and_mutants():
    """The emulation equals the reference at every shape of the GPU test; khkwc is rejected at
    every shape; swap_hw passes at a square image and is rejected at H != W — the reason for the
    shapes."""
    for b, hh, ww, p in fc.PATCHIFY_SHAPES:
        img, mean, std = fc.patchify_inputs(b, hh, ww)
        ref = fc.patchify_reference(img, mean, std, p)
        same = lambda m: torch.equal(fc.bits16(fc.emulate_patchify(img, mean, std, p, m)), fc.bits16(ref))
        assert same(None), (b, hh, ww, p)
        assert same("khkwc") == (False), (b, hh, ww, p)
        assert same("swap_hw") == (hh == ww), (b, hh, ww, p)
    assert any(hh == ww for _, hh, ww, _ in fc.PATCHIFY_SHAPES)
    assert {p for _, hh, ww, p in fc.PATCHIFY_SHAPES if hh != ww} == {8, 16, 24, 32}
    img, mean, std = fc.patchify_inputs(3, 224, 224)          # the one shape of the older test
    assert torch.equal(fc.emulate_patchify(img, mean, std, 16, "swap_hw"),
                       fc.patchify_reference(img, mean, std, 16))


# ---- argument contracts that return before any launch --------------------------------------------
P = C.c_void_p(0x10000)                # never dereferenced: every call below returns first
ODD = C.c_void_p(0x10008)              # 8-B aligned, not 16-B
ODD2 = C.c_void_p(0x10002)


def test_elementwise_abi_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "imgrec_vit.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ("vit_add_layernorm_bf16", "vit_gelu_bf16", "vit_quick_gelu_bf16",
                 "vit_patchify_bf16", "vit_tokens_f32"):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared in imgrec_vit.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported by the library"


def test_add_layernorm_contract():
    ln = _lib.load().vit_add_layernorm_bf16
    eps = C.c_float(1e-5)
    assert ln(P, P, P, P, P, -1, 768, eps, None) == -1
    for dim in (0, 1025, -4):
        assert ln(P, P, P, P, P, 4, dim, eps, None) == -1
    for null in (0, 2, 3, 4):                                   # x, gamma, beta, y (delta may be NULL)
        args = [P] * 5
        args[null] = None
        assert ln(*args, 4, 768, eps, None) == -1, null
    assert ln(P, P, P, P, P, 0, 768, eps, None) == 0
    assert ln(P, None, P, P, P, 0, 1, eps, None) == 0


@pytest.mark.parametrize("name", ["vit_gelu_bf16", "vit_quick_gelu_bf16"])
def test_activation_contract(name):
    act = getattr(_lib.load(), name)
    assert act(P, -1, None) == -1
    assert act(None, 16, None) == -1
    assert act(ODD, 16, None) == -1 and act(ODD2, 1, None) == -1      # not 16-B aligned
    assert act(P, 0, None) == 0 and act(None, 0, None) == 0


def test_patchify_contract():
    pf = _lib.load().vit_patchify_bf16
    for patch in (0, 12, -8):
        assert pf(P, 1, 48, 48, patch, P, P, P, None) == -1, patch
    assert pf(P, 1, 40, 32, 16, P, P, P, None) == -1                  # height % patch
    assert pf(P, 1, 32, 40, 16, P, P, P, None) == -1                  # width % patch
    assert pf(P, -1, 32, 32, 16, P, P, P, None) == -1
    for null in (0, 5, 6, 7):                                         # img, mean, std, out
        args = [P, 1, 32, 32, 16, P, P, P]
        args[null] = None
        assert pf(*args, None) == -1, null
    assert pf(ODD, 1, 32, 32, 16, P, P, P, None) == -1                # img not 16-B aligned
    assert pf(P, 1, 32, 32, 16, P, P, ODD, None) == -1                # out not 16-B aligned
    assert pf(P, 0, 32, 32, 16, P, P, P, None) == 0


def test_tokens_contract():
    tk = _lib.load().vit_tokens_f32
    for dim in (0, 6, -4):
        assert tk(P, P, P, 1, 4, dim, P, None) == -1, dim
    assert tk(P, P, P, 1, -1, 8, P, None) == -1
    assert tk(P, P, P, -1, 4, 8, P, None) == -1
    for null in (0, 1, 2, 6):                                         # patch_emb, cls, pos, out
        args = [P, P, P, 1, 4, 8, P]
        args[null] = None
        assert tk(*args, None) == -1, null
    for odd in (1, 2, 6):                                             # fp32 pointers: 16-B
        args = [P, P, P, 1, 4, 8, P]
        args[odd] = ODD
        assert tk(*args, None) == -1, odd
    assert tk(ODD2, P, P, 1, 4, 8, P, None) == -1                     # patch_emb: 8-B
    assert tk(P, P, P, 0, 4, 8, P, None) == 0
