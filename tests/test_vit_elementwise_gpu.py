"""The fused ViT elementwise kernels (csrc/vit_fused.hip) through their C ABI, against the float64
and bit-exact references of tests/vit_fused_check.py (whose CPU proof is
tests/test_vit_fused_check_cpu.py).  Every output and in-place buffer lies between two guards of
64 elements pre-filled with a NaN pattern, which must come back unchanged as raw integers; inputs
come from a seeded CPU generator and references are computed on the CPU.

Which case reaches which kernel:

  add_ln_kernel<4>       dim 1, 63, 64, 65, 255; dim 256 with one pointer misaligned
  add_ln_kernel<8>       dim 257, 300 (also with every pointer misaligned), 511; dim 512 misaligned
  add_ln_kernel<12>      dim 513, 767; dim 768 misaligned
  add_ln_kernel<16>      dim 769, 1000, 1023; dim 1024 misaligned
  add_ln_vec_kernel<1>   dim 256, all pointers 16-B aligned
  add_ln_vec_kernel<2>   dim 512, aligned
  add_ln_vec_kernel<3>   dim 768, aligned
  add_ln_vec_kernel<4>   dim 1024, aligned
  gelu_kernel            vector branch: the 65,536-pattern buffer, n >= 16 of the length edges;
                         tail branch: the 4,370 launches of 15 patterns each, n % 16 != 0
  quick_gelu_kernel      vector branch: the 65,536-pattern buffer, n >= 8 of the length edges;
                         tail branch: the 9,363 launches of 7 patterns each, n % 8 != 0
  patchify_kernel        H != W at p = 8 (both orientations), 16, 24, 32; one patch (8 x 8, p = 8)
  tokens_kernel          npatch = 0 (cls rows only), dim 12 and 260 (no multiple of 256), dim 768
"""
import ctypes as C
import functools

import pytest
import torch

from tests import vit_fused_check as fc
from tests.vit_check import NAN_BITS

pytestmark = pytest.mark.gpu

GUARD = 64


class Guarded:
    """A GPU buffer [guard | off spare elements | data | guard], every element pre-filled with the
    NaN pattern of its type; `data` (a CPU tensor) is copied in, or the region is left as pattern
    for a pure output.  off = 1 puts the data one element past a 16-byte boundary."""

    def __init__(self, data=None, shape=None, dtype=None, off=0):
        if data is not None:
            shape, dtype = tuple(data.shape), data.dtype
        self.shape, self.dtype, self.off = tuple(shape), dtype, off
        self.n = 1
        for s in self.shape:
            self.n *= s
        self.idt, self.pattern = ((torch.int32, fc.F32_NAN_BITS) if dtype == torch.float32
                                  else (torch.int16, NAN_BITS))
        self.lo = GUARD + off
        self.raw = torch.full((self.lo + self.n + GUARD,), self.pattern, dtype=self.idt, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        if data is not None and self.n:
            self.raw[self.lo:self.lo + self.n].copy_(data.contiguous().view(self.idt).reshape(-1))
        self.addr = self.raw.data_ptr() + self.lo * self.raw.element_size()
        assert (self.addr % 16 == 0) == (off == 0)

    @property
    def ptr(self):
        return C.c_void_p(self.addr)

    def download(self):
        """(data region as a CPU tensor of the buffer's type and shape, guards intact?)."""
        r = self.raw.cpu()
        body = r[self.lo:self.lo + self.n].clone().view(self.dtype).view(self.shape)
        intact = bool((r[:self.lo] == self.pattern).all()) and bool((r[self.lo + self.n:] == self.pattern).all())
        return body, intact


@pytest.fixture(scope="module")
def lib(gpu):
    from image_recommender_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _ln_inputs(suite, rows, dim):
    return fc.ln_inputs(suite, rows, dim, 0)


def _ln_call(lib, suite, rows, dim, eps, with_delta, mis):
    """One vit_add_layernorm_bf16 call with the pointer named by `mis` (or "all", or None) one
    element off its alignment, and every check on what comes back.  Returns error / bound."""
    x, delta, gamma, beta = _ln_inputs(suite, rows, dim)
    off = lambda name: 1 if mis in (name, "all") else 0
    xb, gb, bb = Guarded(x, off=off("x")), Guarded(gamma, off=off("gamma")), Guarded(beta, off=off("beta"))
    db = Guarded(delta, off=off("delta")) if with_delta else None
    yb = Guarded(shape=(rows, dim), dtype=torch.bfloat16, off=off("y"))
    x_before, _ = xb.download()
    rc = lib.vit_add_layernorm_bf16(xb.ptr, db.ptr if with_delta else None, gb.ptr, bb.ptr, yb.ptr,
                                    rows, dim, C.c_float(eps), None)
    torch.cuda.synchronize()
    assert rc == 0
    what = (suite, rows, dim, eps, with_delta, mis)
    x_after, x_guards = xb.download()
    y, y_guards = yb.download()
    assert x_guards and y_guards, f"guard overwritten: {what}"
    for b in (gb, bb) + ((db,) if with_delta else ()):
        body, intact = b.download()
        assert intact, f"input guard overwritten: {what}"
    dl = delta if with_delta else None
    if not with_delta:
        assert torch.equal(fc.bits32(x_after), fc.bits32(x)), f"x changed without a delta: {what}"
    try:
        return fc.check_add_layernorm(x_after, y, x_before, dl, gamma, beta, eps, suite)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def _ln_sweep(lib, dim, mis):
    """rows x delta x suite at one dim and placement, eps rotating so that every suite meets every
    eps (rows index + suite index mod 3 over 5 rows)."""
    worst, used, met = 0.0, 0.0, set()
    for ri, rows in enumerate(fc.LN_ROWS):
        for with_delta in (True, False):
            if mis == "delta" and not with_delta:
                continue                                   # a NULL delta is not a misalignment
            for si, suite in enumerate(fc.ln_suites(dim)):
                eps = fc.LN_EPS[(ri + si) % 3]
                met.add((suite, eps))
                r, su = _ln_call(lib, suite, rows, dim, eps, with_delta, mis)
                worst, used = max(worst, r), max(used, su)
    assert met == {(s, e) for s in fc.ln_suites(dim) for e in fc.LN_EPS}
    return worst, used


@pytest.mark.parametrize("dim", fc.LN_DIMS)
def test_add_layernorm(lib, dim):
    """Aligned pointers at every dim (the vec kernel at 256, 512, 768, 1024; the strided one
    elsewhere); at the multiples of 256 also each single misalignment that sends the call to the
    strided kernel, and at dim 300 every pointer misaligned at once."""
    places = [None]
    if dim % 256 == 0:
        places += ["x", "gamma", "beta", "delta", "y"]
    if dim == 300:
        places += ["all"]
    for mis in places:
        worst, used = _ln_sweep(lib, dim, mis)
        print(f"[vit_elementwise] add_layernorm dim {dim} misaligned {mis}: worst error / bound {worst:.3f}, "
              f"share of the slack used {used:.3f}")


ACTS = {"gelu": ("vit_gelu_bf16", fc.GELU_GROUP), "quick_gelu": ("vit_quick_gelu_bf16", fc.QUICK_GELU_GROUP)}


def _act_check(out, h, kind, what):
    ratio = fc.activation_ratio(out, h, kind)
    assert ratio.numel() == h.numel()
    worst = float(ratio.max()) if h.numel() else 0.0
    bad = int((ratio > 1.0).sum())
    assert bad == 0, (f"{kind} {what}: {bad} of {h.numel()} outside the bound, worst error / bound {worst:.4g} "
                      f"at input pattern {int(fc.bits16(h).reshape(-1)[int(ratio.argmax())]) & 0xFFFF:#06x}")
    return worst, fc.activation_slack_used(out, h, kind)


@pytest.mark.parametrize("kind", sorted(ACTS))
def test_activation_all_bf16_patterns(lib, kind):
    """All 65,536 bit patterns twice: as one buffer (every pattern in the vector branch), and in
    groups of 15 (7 for QuickGELU) patterns, one launch per group, so that every pattern also goes
    through the scalar tail; the slot after each group is a guard."""
    name, group = ACTS[kind]
    fn = getattr(lib, name)
    h = fc.all_bf16_patterns()
    buf = Guarded(h)
    assert fn(buf.ptr, h.numel(), None) == 0
    torch.cuda.synchronize()
    out, intact = buf.download()
    assert intact, "guard overwritten (vector placement)"
    w_vec = _act_check(out, h, kind, "vector branch")

    per = group - 1
    ngroups = -(-h.numel() // per)
    staged = torch.full((ngroups * per,), NAN_BITS, dtype=torch.int16)
    staged[:h.numel()] = fc.bits16(h)
    slots = torch.full((ngroups, group), NAN_BITS, dtype=torch.int16)
    slots[:, :per] = staged.view(ngroups, per)
    is_data = torch.zeros(ngroups, group, dtype=torch.bool)
    is_data[:, :per] = True
    is_data.view(-1)[(ngroups - 1) * group + (h.numel() - (ngroups - 1) * per):] = False
    buf = Guarded(slots.view(torch.bfloat16))
    for gi in range(ngroups):
        n = min(per, h.numel() - gi * per)
        rc = fn(C.c_void_p(buf.addr + gi * group * 2), n, None)
        assert rc == 0
    torch.cuda.synchronize()
    got, intact = buf.download()
    assert intact, "guard overwritten (tail placement)"
    got = fc.bits16(got)
    assert bool((got[~is_data] == NAN_BITS).all()), "the slot behind a tail was written"
    out = got[is_data].view(torch.bfloat16)
    assert out.numel() == h.numel()
    w_tail = _act_check(out, h, kind, "tail branch")
    print(f"[vit_elementwise] {kind}: worst error / bound {w_vec[0]:.3f} (vector), {w_tail[0]:.3f} (tail), "
          f"share of the slack used {w_vec[1]:.3f}, {w_tail[1]:.3f}; {ngroups} tail launches")


ACT_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 4095, 4096, 4097)


@pytest.mark.parametrize("kind", sorted(ACTS))
def test_activation_length_edges(lib, kind):
    """The vector / tail switch and the workgroup edges (256 threads of 8 or 16 elements)."""
    fn = getattr(lib, ACTS[kind][0])
    worst, used = 0.0, 0.0
    for n in ACT_LENGTHS:
        h = (torch.randn(n, generator=fc._gen(n, len(kind))) * 4).bfloat16()
        buf = Guarded(h)
        assert fn(buf.ptr, n, None) == 0
        torch.cuda.synchronize()
        out, intact = buf.download()
        assert intact, f"{kind} n = {n}: guard overwritten"
        r, su = _act_check(out, h, kind, f"n = {n}")
        worst, used = max(worst, r), max(used, su)
    print(f"[vit_elementwise] {kind} length edges: worst error / bound {worst:.3f}, "
          f"share of the slack used {used:.3f}")


@pytest.mark.parametrize("b,h,w,p", fc.PATCHIFY_SHAPES)
def test_patchify(lib, b, h, w, p):
    img, mean, std = fc.patchify_inputs(b, h, w)
    ib, mb, sb = Guarded(img), Guarded(mean), Guarded(std)
    ob = Guarded(shape=(b, (h // p) * (w // p), 3 * p * p), dtype=torch.bfloat16)
    assert lib.vit_patchify_bf16(ib.ptr, b, h, w, p, mb.ptr, sb.ptr, ob.ptr, None) == 0
    torch.cuda.synchronize()
    out, intact = ob.download()
    assert intact, "guard overwritten"
    ref = fc.patchify_reference(ib.download()[0], mean, std, p)
    nbad = int((fc.bits16(out) != fc.bits16(ref)).sum())
    assert nbad == 0, f"{nbad} of {ref.numel()} patch elements differ"


@pytest.mark.parametrize("b,npatch,dim", fc.TOKENS_SHAPES)
def test_tokens(lib, b, npatch, dim):
    pe, cls, pos = fc.tokens_inputs(b, npatch, dim)
    pb, cb, sb = Guarded(pe), Guarded(cls), Guarded(pos)
    ob = Guarded(shape=(b, npatch + 1, dim), dtype=torch.float32)
    assert lib.vit_tokens_f32(pb.ptr, cb.ptr, sb.ptr, b, npatch, dim, ob.ptr, None) == 0
    torch.cuda.synchronize()
    out, intact = ob.download()
    assert intact, "guard overwritten"
    ref = fc.tokens_reference(pe, cls, pos)
    nbad = int((fc.bits32(out) != fc.bits32(ref)).sum())
    assert nbad == 0, f"{nbad} of {ref.numel()} token elements differ"
