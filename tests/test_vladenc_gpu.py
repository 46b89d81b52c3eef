"""HIP tests of the VLAD encoder's forward pass (include/imgrec_vladenc.h, csrc/vladenc.hip,
image_recommender_amd.vlad_encoder) against the rules of tests/vladenc_check.py.

Every case (vladenc_check.CASES: the reference's widths at a depth of 1024 and at the real 32768,
odd widths below one tile, a single layer, five layers, one-hot inputs at the last column and at a
split boundary) goes through vladenc_forward_device at each of its batch sizes with NaN-poisoned
outputs, twice, and the two runs must be byte-equal.  Then: batch invariance byte for byte (rows
alone, the reversed batch, three chunk sizes), the optional `hidden`, the flag, n = 0, the four ways
to call, the descriptor-to-vector pipeline, two streams and two handles on the shared workspace.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import vladenc_check as ec

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in ec.CASES]


@pytest.fixture(scope="module")
def encoders(gpu):
    """A VladEncoder per case, made on first use."""
    from image_recommender_amd.vlad_encoder import VladEncoder
    cache = {}

    def get(name):
        if name not in cache:
            p = ec.case_params(name)
            cache[name] = VladEncoder(p.W, p.b, p.g, p.be, ln_eps=p.eps)
        return cache[name]
    yield get
    for e in cache.values():
        e.close()


def gpu_forward(enc, x, model_output=False, want_hidden=True, chunk_rows=0, stream=None):
    """vladenc_forward_device on a numpy input: (out, hidden) as numpy (hidden None without
    `want_hidden`).  The outputs start as NaN, so an element the call leaves unwritten fails the
    checks; without `want_hidden` the poisoned buffer must come back untouched."""
    import torch
    from image_recommender_amd import _lib
    lib = _lib.load()
    n = x.shape[0]
    dev = torch.device("cuda")
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(dev) if n else torch.empty((1, enc.in_dim), device=dev)
    out = torch.full((max(n, 1), enc.out_dim), float("nan"), dtype=torch.float32, device=dev)
    hid = torch.full((max(n, 1), max(enc.hidden_dim, 1)), float("nan"), dtype=torch.float32, device=dev)
    old = os.environ.get("IMGREC_VLADENC_CHUNK_ROWS")
    if chunk_rows:
        os.environ["IMGREC_VLADENC_CHUNK_ROWS"] = str(chunk_rows)       # read when the call starts
    try:
        st = (stream or torch.cuda.current_stream()).cuda_stream
        _lib.check(lib.vladenc_forward_device(
            enc._handle(), C.c_void_p(xd.data_ptr()), n, _lib.VLADENC_MODEL_OUTPUT if model_output else 0,
            C.c_void_p(out.data_ptr()), C.c_void_p(hid.data_ptr()) if want_hidden else None, C.c_void_p(st or None)),
            "vladenc_forward_device")
        torch.cuda.synchronize()
    finally:
        if chunk_rows:
            if old is None:
                os.environ.pop("IMGREC_VLADENC_CHUNK_ROWS", None)
            else:
                os.environ["IMGREC_VLADENC_CHUNK_ROWS"] = old
    assert torch.isnan(out[n:]).all() and torch.isnan(hid[n:]).all(), "written past the batch"
    if not want_hidden:
        assert torch.isnan(hid).all(), "hidden was written although NULL was passed"
        return out.cpu().numpy()[:n], None
    assert enc.hidden_dim > 0 or torch.isnan(hid).all()
    return out.cpu().numpy()[:n], hid.cpu().numpy()[:n, :enc.hidden_dim]


@pytest.fixture(scope="module")
def runs(gpu, encoders):
    """(stored, model, hidden) of every (case, batch size), computed once on first use."""
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            x = ec.case_input(name, n)
            stored, hidden = gpu_forward(encoders(name), x)
            model, hidden2 = gpu_forward(encoders(name), x, model_output=True)
            assert hidden.tobytes() == hidden2.tobytes()
            cache[name, n] = (stored, model, hidden)
        return cache[name, n]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_case(gpu, encoders, runs, name):
    p = ec.case_params(name)
    for n in ec.CASE[name].batches:
        x = ec.case_input(name, n)
        stored, model, hidden = runs(name, n)
        assert stored.shape == model.shape == (n, p.widths[-1]) and hidden.shape == (n, sum(p.hidden_widths))
        print(f"{name} n={n}: ", end="")
        ratio, e2e = ec.check_all(name, p, x, stored, model, hidden)
        print(f"hidden error at most {ratio:.4f} of its bound, end to end {e2e:.3e} (tolerance {ec.E2E_TOL[name]:.3e})")
        again, hidden_again = gpu_forward(encoders(name), x)
        assert again.tobytes() == stored.tobytes() and hidden_again.tobytes() == hidden.tobytes()


def test_batch_invariance(gpu, encoders, runs):
    enc = encoders("ref_small")
    x = ec.case_input("ref_small", 129)
    stored, model, hidden = runs("ref_small", 129)
    import torch
    from image_recommender_amd import _lib
    # every row alone: device-resident, one call per row into one poisoned buffer
    xd = torch.from_numpy(np.array(x)).cuda()
    out = torch.full((129, enc.out_dim), float("nan"), dtype=torch.float32, device="cuda")
    hid = torch.full((129, enc.hidden_dim), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for i in range(129):
        enc.forward_device(xd[i].data_ptr(), 1, out[i].data_ptr(), stream=st, hidden_ptr=hid[i].data_ptr())
    torch.cuda.synchronize()
    o, h = out.cpu().numpy(), hid.cpu().numpy()
    for i in range(129):
        assert o[i].tobytes() == stored[i].tobytes(), f"row {i} alone differs from its row of the batch"
        assert h[i].tobytes() == hidden[i].tobytes(), f"row {i} alone: hidden differs"
    r, rh = gpu_forward(enc, np.ascontiguousarray(x[::-1]))
    assert r[::-1].tobytes() == stored.tobytes() and rh[::-1].tobytes() == hidden.tobytes()
    for n in (1, 3):                                       # the narrow tile's batches are prefixes of the wide one's
        assert runs("ref_small", n)[0].tobytes() == stored[:n].tobytes()
        assert runs("ref_small", n)[2].tobytes() == hidden[:n].tobytes()
    assert _lib.VLADENC_CHUNK_ROWS == 128


@pytest.mark.parametrize("rows", [1, 64, 100])
def test_chunk_rows_change_nothing(gpu, encoders, runs, rows):
    x = ec.case_input("ref_small", 129)
    stored, model, hidden = runs("ref_small", 129)
    o, h = gpu_forward(encoders("ref_small"), x, chunk_rows=rows)
    assert o.tobytes() == stored.tobytes() and h.tobytes() == hidden.tobytes()
    m, _ = gpu_forward(encoders("ref_small"), x, chunk_rows=rows, model_output=True)
    assert m.tobytes() == model.tobytes()


def test_many_rows_cross_the_chunk_and_launch_boundaries(gpu, encoders):
    """Without the knob: 2100 rows of `odd` are two chunks (2048 rows in 16 row tiles, then 52), and
    200 rows of `ref_full` take the first layer in two launches
    (128 + 72 rows, its partial sums being the largest) and the later layers in one.  Rows cut out
    around each boundary and run as a batch of their own give the same bytes; the derived bounds hold."""
    from image_recommender_amd import _lib
    assert _lib.VLADENC_SUPER_ROWS == 2048
    rng = np.random.default_rng(31)
    for name, n, cuts in (("odd", 2100, (slice(2040, 2100), slice(0, 1), slice(2047, 2049))),
                          ("ref_full", 200, (slice(120, 136), slice(199, 200)))):
        p, enc = ec.case_params(name), encoders(name)
        x = rng.standard_normal((n, p.widths[0]), dtype=np.float32)
        if name == "ref_full":
            x /= np.linalg.norm(x, axis=1, keepdims=True)              # unit rows, as VLAD vectors are
        stored, hidden = gpu_forward(enc, x)
        model, _ = gpu_forward(enc, x, model_output=True)
        for cut in cuts:
            s, h = gpu_forward(enc, np.ascontiguousarray(x[cut]))
            assert s.tobytes() == stored[cut].tobytes() and h.tobytes() == hidden[cut].tobytes(), (name, cut)
        sub = slice(0, n) if name == "odd" else slice(120, 136)
        ec.check_linear(p, x[sub], hidden[sub])
        ec.check_output(p, x[sub], hidden[sub], model[sub], stored[sub])


def test_hidden_is_optional_and_the_flag_is_one_division(gpu, encoders, runs):
    for name in ("ref_small", "one_layer"):
        n = max(ec.CASE[name].batches)
        x = ec.case_input(name, n)
        stored, model, hidden = runs(name, n)
        assert gpu_forward(encoders(name), x, want_hidden=False)[0].tobytes() == stored.tobytes()
        assert gpu_forward(encoders(name), x, want_hidden=False, model_output=True)[0].tobytes() == model.tobytes()
        # the default is the model output divided by (its norm + 1e-7): float64, rounded once
        ref = ec.second64(model)
        assert (np.abs(stored.astype(np.float64) - ref) <= ec.U * (1 + 2.0 ** -20) * np.abs(ref)).all()
        assert (stored != model).any()
        np.testing.assert_allclose(np.linalg.norm(model.astype(np.float64), axis=1), 1.0, atol=2 * ec.U, rtol=0)


def test_no_rows(gpu, encoders):
    enc = encoders("ref_small")
    out, hid = gpu_forward(enc, np.zeros((0, enc.in_dim), np.float32))        # asserts nothing was written
    assert out.shape == (0, enc.out_dim) and hid.shape == (0, enc.hidden_dim)
    assert enc.forward(np.zeros((0, enc.in_dim), np.float32)).shape == (0, enc.out_dim)


def test_four_ways_to_call(gpu, encoders, runs):
    import torch
    from image_recommender_amd import _lib
    enc = encoders("odd")
    x = ec.case_input("odd", 129)
    stored, model, hidden = runs("odd", 129)
    a, ah = enc.forward(x, return_hidden=True)
    assert a.dtype == np.float32 and a.tobytes() == stored.tobytes() and ah.tobytes() == hidden.tobytes()
    assert enc.forward(x, model_output=True).tobytes() == model.tobytes()
    assert enc.forward(x[5]).tobytes() == stored[5].tobytes()                  # one vector
    xd = torch.from_numpy(np.array(x)).cuda()
    out = torch.full((129, enc.out_dim), float("nan"), dtype=torch.float32, device="cuda")
    enc.forward_device(xd.data_ptr(), 129, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == stored.tobytes()
    h = np.full_like(stored, np.nan)
    hh = np.full_like(hidden, np.nan)
    xc = np.ascontiguousarray(x)
    _lib.check(_lib.load().vladenc_forward(enc._handle(), xc.ctypes.data, 129, 0, h.ctypes.data, hh.ctypes.data),
               "vladenc_forward")
    assert h.tobytes() == stored.tobytes() and hh.tobytes() == hidden.tobytes()
    # (the raw device entry is what `runs` went through)
    w = (C.c_int * 9)()
    nl = C.c_int()
    _lib.check(_lib.load().vladenc_widths(enc._handle(), w, C.byref(nl)), "vladenc_widths")
    assert nl.value == 3 and tuple(w[:4]) == enc.widths


def test_pipeline_from_descriptors(gpu, encoders, runs):
    """encode_images keeps the VLAD vectors on the device; the host round trip gives the same bytes."""
    from image_recommender_amd.vlad import SoftVLAD
    from tests import vlad_check as vc
    cs = vc.CASE["sift"]
    x, off, c = vc.case_data("sift")
    descs = [x[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    sv = SoftVLAD(c, nn=cs.nn, sigma=cs.sigma)
    enc = encoders("ref_full")
    got = enc.encode_images(sv, descs)
    vlad = sv.encode(descs)
    want = enc.forward(vlad)
    assert got.dtype == np.float32 and got.shape == (8, 128) and got.tobytes() == want.tobytes()
    zero = enc.forward(np.zeros((1, 32768), np.float32))[0]
    empty = np.nonzero(np.diff(off) == 0)[0]
    assert empty.size == 2
    for i in empty:
        assert got[i].tobytes() == zero.tobytes()
    assert enc.encode_images(sv, (x, off), model_output=True).tobytes() == enc.forward(vlad, model_output=True).tobytes()
    assert enc.encode_images(sv, []).shape == (0, 128)
    # the GPU's VLAD vectors agree with the numpy ones the case is made of to fp32 rounding, so
    # the stored vectors agree end to end
    p = ec.case_params("ref_full")
    assert ec.end_to_end_error(p, vlad, got) <= ec.E2E_TOL["ref_full"]


def test_forward_device_alternating_on_two_streams(gpu, encoders):
    """Six calls alternating between two streams share the per-device workspace (split partial sums,
    hidden activations) through its stream hand-off (csrc/dev_workspace.h over csrc/stream_fence.h):
    each equals, byte for byte, the same call made alone.  Every call has an input of its own, so a
    call that overtook its predecessor's use of the workspace would show."""
    import torch
    enc = encoders("ref_small")
    calls, n = 6, 40
    rng = np.random.default_rng(77)
    xs = [torch.from_numpy(rng.standard_normal((n, enc.in_dim), dtype=np.float32)).cuda() for _ in range(calls)]
    one = torch.cuda.Stream()
    enc._handle()
    torch.cuda.synchronize()

    def run(streams, sync):
        outs = [torch.full((n, enc.out_dim), float("nan"), dtype=torch.float32, device="cuda") for _ in xs]
        torch.cuda.synchronize()
        for c, (x, out) in enumerate(zip(xs, outs)):
            enc.forward_device(x.data_ptr(), n, out.data_ptr(), stream=streams[c % len(streams)].cuda_stream)
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]

    alone = run([one], True)
    assert all(np.isfinite(a).all() for a in alone)
    assert len({a.tobytes() for a in alone}) == calls
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for got, want in zip(run([a, b], False), alone):
        assert got.tobytes() == want.tobytes()


def test_two_handles_share_the_workspace(gpu, encoders, runs):
    """Two encoders with different weights (and layer shapes), called alternately on one stream
    without a wait in between: neither sees the other's partial sums or activations."""
    import torch
    ea, eb = encoders("ref_small"), encoders("odd")
    xa, xb = ec.case_input("ref_small", 129), ec.case_input("odd", 129)
    want_a, want_b = runs("ref_small", 129)[0], runs("odd", 129)[0]
    xad, xbd = torch.from_numpy(np.array(xa)).cuda(), torch.from_numpy(np.array(xb)).cuda()
    outs = []
    st = torch.cuda.current_stream().cuda_stream
    for i in range(3):
        oa = torch.full((129, ea.out_dim), float("nan"), dtype=torch.float32, device="cuda")
        ob = torch.full((129, eb.out_dim), float("nan"), dtype=torch.float32, device="cuda")
        ea.forward_device(xad.data_ptr(), 129, oa.data_ptr(), stream=st)
        eb.forward_device(xbd.data_ptr(), 129, ob.data_ptr(), stream=st)
        outs.append((oa, ob))
    torch.cuda.synchronize()
    for oa, ob in outs:
        assert oa.cpu().numpy().tobytes() == want_a.tobytes() and ob.cpu().numpy().tobytes() == want_b.tobytes()
