"""vit_linear_bf16 (include/imgrec_vit.h, csrc/vit_gemm.hip) — the HIP GEMM behind every matrix
product of the DreamSim-architecture forward — against a plain PyTorch fp32 reference of the same
op, act(x W^T + b) on the same bf16 operands, and the forward built on it against the hipBLASLt
one (/root/reference/vector_scripts/create_dreamsim_vector.py:51-93 embeds with this
architecture; its values are parity-unpinned: no pretrained weights here).

Tolerance, stated: the output is one bf16 rounding of an fp32 sum, so |y - ref| <= 2^-8 |ref|
(round to nearest: half an ulp of 2^-7 relative) + 2^-20 sum_i |x_i w_i| (fp32 accumulation-order
slack of a K <= 3072 dot product; the rigorous gamma_K is ~2e-4 of that sum, the observed ~1e-6)
+ the activation's own fp32 evaluation (erff / __expf: a few ulps, inside the first term).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = {"none": lambda t: t, "gelu": lambda t: torch.nn.functional.gelu(t),
        "quick_gelu": lambda t: t * torch.sigmoid(1.702 * t),
        "gelu_tanh": lambda t: torch.nn.functional.gelu(t, approximate="tanh")}


def _linear(m, k, n, act="none", bias=True, seed=0, scale=1.0, bf16_bias=False):
    """(y, fp32 reference, sum |x_i w_i|); bf16_bias: the reference adds the bias rounded to bf16
    (what _lin's F.linear fallback adds)."""
    from types import SimpleNamespace

    from image_recommender_amd.vector_scripts.create_dreamsim_vector import _hlin
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.randn(m, k, device="cuda", generator=g) * scale).bfloat16()
    w = (torch.randn(n, k, device="cuda", generator=g) / k ** 0.5).bfloat16()
    b = torch.randn(n, device="cuda", generator=g) if bias else None
    mod = SimpleNamespace(w_lp=w.contiguous(), b_lp=b.bfloat16() if bias else None,
                          b_f32=b.contiguous() if bias else None)
    y = _hlin(mod, x, act)
    torch.cuda.synchronize()
    ref = x.float() @ w.float().T + ((b.bfloat16().float() if bf16_bias else b) if bias else 0.0)
    ref = ACTS[act](ref)
    absum = x.float().abs() @ w.float().abs().T
    return y, ref, absum


def _within(y, ref, absum):
    err = (y.float() - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + absum * 2.0 ** -20 + 1e-30
    worst = float((err / bound).max())
    assert worst <= 1.0, worst
    return worst


@pytest.mark.parametrize("m,k,n", [(197 * 2, 768, 2304), (197, 768, 768), (512, 768, 3072),
                                   (394, 3072, 768), (1, 768, 256), (7, 64, 256), (8 * 197, 768, 768),
                                   (5000, 128, 512), (256 * 3 + 1, 256, 512)])
def test_linear_matches_fp32_reference(gpu, m, k, n):
    """Shapes of the forward (qkv / proj / fc1 / fc2 at 1-8 images), a single row, tails of a
    256-row tile (m = 197, 769: rows past M staged from row M - 1 and never stored), more token
    tiles than splits (m = 5000)."""
    y, ref, absum = _linear(m, k, n, seed=m + k + n)
    assert y.shape == (m, n) and y.dtype == torch.bfloat16
    _within(y, ref, absum)


@pytest.mark.parametrize("act", ["gelu", "quick_gelu", "gelu_tanh"])
def test_linear_activation_epilogue(gpu, act):
    """fc1's activation in the epilogue (fp32, before the bf16 rounding): nn.GELU's erf form
    (DINO / OpenCLIP), CLIP's QuickGELU, the tanh form."""
    y, ref, absum = _linear(197 * 3, 768, 3072, act, seed=7, scale=2.0)
    _within(y, ref, absum)


def test_linear_without_bias_and_refusals(gpu):
    """No bias (the CLIP / OpenCLIP patch projections); shapes the kernel does not take are
    refused by the C ABI (k % 64, n % 256, misaligned) and served by _lin in _hlin."""
    import ctypes as C

    from image_recommender_amd import _lib
    y, ref, absum = _linear(300, 768, 768, bias=False, seed=3)
    _within(y, ref, absum)
    lib = _lib.load()
    x = torch.zeros(10, 96, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(256, 96, dtype=torch.bfloat16, device="cuda")
    out = torch.empty(10, 256, dtype=torch.bfloat16, device="cuda")
    assert lib.vit_linear_bf16(C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), None, 10, 96,
                               256, 0, C.c_void_p(out.data_ptr()), None) == -1
    y2, ref2, absum2 = _linear(10, 96, 200, seed=4, bf16_bias=True)   # k % 64, n % 256: _lin path
    _within(y2, ref2, absum2)
    # fc1's fused activation on a fallback shape: _lin, then the activation in fp32
    # on the bf16-rounded pre-activation; stated bound: that rounding (2^-9 |pre|) through the
    # activation's slope (< 1.13 for GELU) plus the output's own bf16 rounding
    for act in ("gelu_tanh", "gelu", "quick_gelu"):
        y3, ref3, absum3 = _linear(10, 96, 200, act, seed=5, bf16_bias=True)
        pre = _linear(10, 96, 200, "none", seed=5, bf16_bias=True)[1]
        err = (y3.float() - ref3).abs()
        bound = ref3.abs() * 2.0 ** -8 + pre.abs() * 1.2 * 2.0 ** -8 + absum3 * 2.0 ** -20 + 1e-30
        assert float((err / bound).max()) <= 1.0, act


def test_forward_on_hip_gemm_matches_hipblaslt(gpu):
    """The fused forward with every GEMM on vit_linear_bf16 against the same forward on
    hipBLASLt (same weights, 6 images, 4 blocks per tower): cosine > 0.999 per image."""
    from image_recommender_amd.vector_scripts.create_dreamsim_vector import build_ensemble
    x = torch.rand((6, 3, 224, 224), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    lt = build_ensemble(seed=0, depth=4).cuda().eval().prepare_inference(torch.bfloat16, fused=True,
                                                                         hip_gemm=False)
    hg = build_ensemble(seed=0, depth=4).cuda().eval().prepare_inference(torch.bfloat16, fused=True)
    assert all(t.hip_gemm for t in hg.towers) and not any(t.hip_gemm for t in lt.towers)
    with torch.no_grad():
        a = torch.nn.functional.normalize(lt.embed(x).float(), dim=-1)
        b = torch.nn.functional.normalize(hg.embed(x).float(), dim=-1)
    cos = (a * b).sum(-1)
    assert float(cos.min()) > 0.999, cos


# ---- the multi-tile paths ------------------------------------------------------------------------
# vit_gemm_kernel gives a workgroup the token tiles split, split + nsplit, ...; between two tiles
# of one workgroup it waits with vmcnt(16) instead of vmcnt(0) after a full tile, issues the
# weight waves' deferred DMA early and carries the issue cursor over.  The automatic split count
# (vit_gemm_splits) gives a workgroup a second tile only when ntile > CUs / (n / 256), so the tests
# below set the split count themselves (vit_linear_bf16_split) or choose m from the CU count.
#
# They call the C ABI directly, into an output of m + 256 rows pre-filled with the bf16 NaN 0x7FC0:
# rows >= m must stay bitwise untouched (rows past M are staged from row M - 1, never stored) and
# rows < m must all be finite (every block of the XCD map wrote its output).
_ACT_ID = {"none": 0, "gelu": 1, "gelu_tanh": 2, "quick_gelu": 3}
_NAN_BITS = 0x7FC0
_GUARD = 256


def _operands(m, k, n, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.randn(m, k, device="cuda", generator=g) * scale).bfloat16()
    w = (torch.randn(n, k, device="cuda", generator=g) / k ** 0.5).bfloat16()
    b = torch.randn(n, device="cuda", generator=g)
    return x, w, b


def _run(x, w, b, act="none", nsplit=None):
    """vit_linear_bf16_split (nsplit None: vit_linear_bf16) on the current stream into a guarded
    buffer; the (m, n) result after the guard and finiteness checks."""
    import ctypes as C

    from image_recommender_amd import _lib
    lib = _lib.load()
    (m, k), n = x.shape, w.shape[0]
    buf = torch.full((m + _GUARD, n), _NAN_BITS, dtype=torch.int16, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if nsplit is None:
        rc = lib.vit_linear_bf16(p(x), p(w), p(b), m, k, n, _ACT_ID[act], p(buf), st)
    else:
        rc = lib.vit_linear_bf16_split(p(x), p(w), p(b), m, k, n, _ACT_ID[act], nsplit, p(buf), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((buf[m:] == _NAN_BITS).all()), "a row past m was stored"
    y = buf[:m].view(torch.bfloat16)
    assert bool(torch.isfinite(y.float()).all()), "an output block was not written"
    return y


def _reference(x, w, b, act="none"):
    ref = ACTS[act](x.float() @ w.float().T + b)
    return ref, x.float().abs() @ w.float().abs().T


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# (m, k, n, the split counts): what each row reaches is in the test's docstring
SPLIT_ROWS = [(845, 128, 256, (1,)), (845, 64, 256, (1,)), (1024, 768, 512, (1, 2, 4)),
              (845, 768, 768, (1, 2)), (1281, 192, 1280, (1, 3)), (1666, 256, 2048, (1, 4, 7)),
              (600, 3072, 768, (1, 3)), (197, 768, 768, (1,))]
SPLIT_ACTS = [(r, "none") for r in range(len(SPLIT_ROWS))] + \
             [(r, a) for r in (0, 5) for a in ("gelu", "quick_gelu", "gelu_tanh")]


@pytest.mark.parametrize("row,act", SPLIT_ACTS)
def test_linear_forced_splits(gpu, row, act):
    """More than one token tile per workgroup, by a forced split count, against the fp32
    reference (the file's bound, unchanged), bitwise equal to vit_linear_bf16 and across the split
    counts (every output element comes from one workgroup in a fixed K order).
      0: 845 x 128 -> 256, nsplit 1: 4 tiles in one workgroup, full, full, full, 77 rows (two live
         64-row quads);
      1: k = 64, nst = 1: a tile's first stage is its last, the vmcnt(16) wait and the early weight
         issue meet;
      2: 1024 x 768 -> 512, nsplit 1, 2, 4: only full tiles, ending on a full tile;
      3: 845 x 768 -> 768, nsplit 1, 2: nqb = 3; the partial tile is the second tile of split 1;
      4: 1281 x 192 -> 1280, nsplit 1, 3: nqb = 5 so G = 5, 15 workgroups (no multiple of 8), the
         last tile is one row;
      5: 1666 x 256 -> 2048, nsplit 1, 4, 7: nqb = 8 so G = 4, 7 tiles with unequal counts, a
         130-row tail (three live quads);
      6: 600 x 3072 -> 768, nsplit 1, 3: 48 stages per tile;
      7: 197 x 768 -> 768, nsplit 1: the baseline, one partial tile.
    Rows 0 and 5 run with every activation too: the epilogue sits between the two tiles' memory
    operations."""
    m, k, n, splits = SPLIT_ROWS[row]
    x, w, b = _operands(m, k, n, seed=m + k + n, scale=2.0 if act != "none" else 1.0)
    ref, absum = _reference(x, w, b, act)
    auto = _run(x, w, b, act)
    # nsplit 1 walks every tile in one workgroup: cnt >= 2 in all rows but the baseline
    assert splits[0] == 1 and ((m + 255) // 256 >= 2 or row == 7)
    for nsplit in splits:
        y = _run(x, w, b, act, nsplit)
        worst = _within(y, ref, absum)
        print(f"[vit_gemm] row {row} ({m}, {k}, {n}) {act} nsplit {nsplit}: error / bound {worst:.3f}")
        assert _same_bits(y, auto), f"nsplit {nsplit} differs from vit_linear_bf16"


def test_linear_split_count_is_validated(gpu):
    """nsplit = 0 is the automatic choice; 1 <= nsplit <= ceil(m / 256) otherwise."""
    import ctypes as C

    from image_recommender_amd import _lib
    lib = _lib.load()
    x, w, b = _operands(600, 64, 256, seed=1)
    assert _same_bits(_run(x, w, b, nsplit=0), _run(x, w, b))
    buf = torch.full((600, 256), _NAN_BITS, dtype=torch.int16, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    for bad in (-1, 4, 1 << 20):
        assert lib.vit_linear_bf16_split(p(x), p(w), p(b), 600, 64, 256, 0, bad, p(buf), None) == -1
    torch.cuda.synchronize()
    assert bool((buf == _NAN_BITS).all())
    assert lib.vit_linear_splits(600, 256) == 3 and lib.vit_linear_splits(600, 100) == -1


def _auto_m(tiles_per_cu_group):
    """m whose automatic split leaves a workgroup more than one tile at n = 3072 (12 feature
    blocks: CUs // 12 workgroups per block), with a 77-row tail."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 256 * (tiles_per_cu_group * (cus // 12) + 1) + 77


def _auto_tiles(m, n):
    from image_recommender_amd import _lib
    nsplit = _lib.load().vit_linear_splits(m, n)
    ntile = (m + 255) // 256
    assert 1 <= nsplit <= ntile
    return -(-ntile // nsplit)


# tiles-per-group factor, k, the fewest tiles per workgroup the case must reach: 5709 rows on 256
# CUs (2 tiles), 11,085 (3 tiles), 16,461 (4 tiles)
AUTO_CASES = [(1, 64, 2), (1, 768, 2), (2, 64, 2), (2, 768, 2), (3, 768, 3)]


@pytest.mark.parametrize("factor,k,least", AUTO_CASES)
def test_linear_automatic_split_multi_tile(gpu, factor, k, least):
    """The automatic split count, at shapes where it gives a workgroup two, three and four tiles:
    the test asserts that of vit_linear_splits itself, then checks the output."""
    m, n = _auto_m(factor), 3072
    per = _auto_tiles(m, n)
    assert per >= least, (m, per)
    x, w, b = _operands(m, k, n, seed=m + k)
    worst = _within(_run(x, w, b), *_reference(x, w, b))
    print(f"[vit_gemm] automatic, ({m}, {k}, {n}), {per} tiles per workgroup: error / bound {worst:.3f}")


@pytest.mark.parametrize("k,act", [(64, "none"), (768, "gelu")])
def test_linear_non_temporal_stores(gpu, k, act):
    """The NT = true instantiations (m n 2 > 512 MiB) at the smallest m that selects them for
    n = 3072, m = 87,382 = 341 * 256 + 86: k = 64, and fc1 itself (k = 768, GELU).  All rows are
    compared; the fp32 reference is computed in chunks of 8192 rows.  Large because no smaller
    shape takes the path."""
    import time
    m, n = 87382, 3072
    assert m * n * 2 > 512 << 20 >= (m - 1) * n * 2
    assert _auto_tiles(m, n) >= 2
    x, w, b = _operands(m, k, n, seed=k, scale=2.0 if act != "none" else 1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = _run(x, w, b, act)
    worst = 0.0
    for r0 in range(0, m, 8192):
        ref, absum = _reference(x[r0:r0 + 8192], w, b, act)
        worst = max(worst, _within(y[r0:r0 + 8192], ref, absum))
    torch.cuda.synchronize()
    print(f"[vit_gemm] non-temporal ({m}, {k}, {n}) {act}: error / bound {worst:.3f}, "
          f"{1e3 * (time.perf_counter() - t0):.0f} ms for the call and the check")


@pytest.mark.parametrize("m,k,n,nsplit", [(845, 3072, 256, 1), (-1, 768, 3072, None),
                                          (-2, 768, 3072, None)])
def test_linear_exact_integers(gpu, m, k, n, nsplit):
    """x integers in [-4, 4], w in [-2, 2], bias in [-8, 8], no activation: every partial sum is
    an integer below 2^24, so the fp32 result is exact in any accumulation order and the output is
    the bf16 rounding of the exact product — zero tolerance.  m = -f stands for the automatic
    multi-tile shape _auto_m(f)."""
    if m < 0:
        m = _auto_m(-m)
        assert _auto_tiles(m, n) >= 2
    g = torch.Generator(device="cuda").manual_seed(k)
    x = torch.randint(-4, 5, (m, k), device="cuda", generator=g).bfloat16()
    w = torch.randint(-2, 3, (n, k), device="cuda", generator=g).bfloat16()
    b = torch.randint(-8, 9, (n,), device="cuda", generator=g).float()
    y = _run(x, w, b, nsplit=nsplit)
    ref = x.double() @ w.double().T + b.double()
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(y, ref.float().bfloat16())


def test_linear_repeatable_and_stream_independent(gpu):
    """The automatic multi-tile case three times on the current stream and once on another one:
    bitwise identical."""
    m, k, n = _auto_m(2), 768, 3072
    assert _auto_tiles(m, n) >= 2
    x, w, b = _operands(m, k, n, seed=11)
    first = _run(x, w, b)
    for _ in range(2):
        assert _same_bits(_run(x, w, b), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _run(x, w, b)
    torch.cuda.current_stream().wait_stream(side)
    assert _same_bits(other, first)
    _within(first, *_reference(x, w, b))
