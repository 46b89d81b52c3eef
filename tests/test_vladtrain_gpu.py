"""HIP tests of the VLAD encoder's training step (include/imgrec_vladtrain.h, csrc/vladtrain.hip,
image_recommender_amd.vlad_trainer) against the rules of tests/vladtrain_check.py.

Every case (vladtrain_check.CASES, the 8-layer depth limit among them) goes through `grads` with
poisoned outputs (the losses, z and the masks by the caller; the gradient vector by the library,
which fills it with NaN bytes before a grads call, so a slot no kernel writes is not finite), twice,
byte-equal:
losses and gradients against the float64 checker within 4 x torch's own fp32 error, the returned
masks against the host's regeneration of the documented hash.  Then: the p = 0 forward byte for
byte against VladEncoder, three Adam steps against adam64 on the device's own gradients, two
trainers / two streams / the chunk knob byte for byte, a 30-step fit, evaluate, save and load, the
descriptor pipeline, and the batch limits.
"""
import os

import numpy as np
import pytest

from tests import vladtrain_check as tc

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in tc.CASES]


def make_trainer(name, dropout=None, seed=tc.SEED, **kw):
    from image_recommender_amd.vlad_trainer import VladEncoderTrainer
    cs, p = tc.CASE[name], tc.case_params(name)
    return VladEncoderTrainer(widths=cs.widths, params=(p.W, p.b, p.g, p.be), seed=seed,
                              dropout=cs.dropout if dropout is None else dropout, **kw)


@pytest.fixture(scope="module")
def trainers(gpu):
    """A trainer per case (its dropout, seed SEED, step 0), made on first use; the tests that step
    make their own."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = make_trainer(name)
        return cache[name]
    yield get
    for t in cache.values():
        t.close()


def flat(state):
    return [a for part in state for a in part]


def state_bytes(tr):
    from image_recommender_amd import _lib
    return b"".join(a.tobytes() for which in (_lib.VLADTRAIN_PARAMS, _lib.VLADTRAIN_ADAM_M, _lib.VLADTRAIN_ADAM_V)
                    for a in flat(tr.get_state(which)))


@pytest.mark.parametrize("name", NAMES)
def test_grads_pass_the_checker_and_repeat_byte_for_byte(trainers, name):
    cs, tr = tc.CASE[name], trainers(name)
    x, idx = tc.case_input(name), tc.case_sample(name)
    a = tr.grads(x, sample_idx=idx, return_masks=True, return_z=True)
    b = tr.grads(x, sample_idx=idx, return_masks=True, return_z=True)
    for k in ("weights", "biases", "ln_weights", "ln_biases"):
        for u, v in zip(a[k], b[k]):
            assert np.isfinite(u).all() and u.tobytes() == v.tobytes(), k
    assert a["losses"] == b["losses"] and all(np.isfinite(a["losses"]))
    assert a["z"].tobytes() == b["z"].tobytes() and np.isfinite(a["z"]).all()
    assert a["masks"].tobytes() == b["masks"].tobytes()
    got = tc.as_step(a)
    ref, tol = tc.case_reference(name), tc.tolerances(name)
    e = tc.errors(cs.widths, got, ref)
    print(f"{name}: error (tolerance)")
    for k in e:
        print(f"    {k:5s} {e[k]:.3e} ({tol[k]:.3e})")
    tc.check_step(name, got)
    want = tc.host_masks(cs)
    if want:
        assert (a["masks"] == np.concatenate(want, axis=1)).all(), "the masks are not the documented hash"
        if cs.dropout > 0:
            assert 0.02 < 1.0 - a["masks"].mean() < 0.25
    else:
        assert a["masks"].shape == (cs.n, 0)
    assert np.abs(a["z"].astype(np.float64) - ref["z"]).max() < 1e-4
    assert tr.step_count == 0, "grads must not advance the step"


@pytest.mark.parametrize("name", ["tiny", "ref_small", "ref_full", "one_layer", "deep8"])
def test_training_forward_at_p0_is_the_encoders_bytes(gpu, name):
    from image_recommender_amd.vlad_encoder import VladEncoder
    p, x = tc.case_params(name), tc.case_input(name)
    tr = make_trainer(name, dropout=0.0)
    enc = VladEncoder(p.W, p.b, p.g, p.be)
    try:
        z = tr.grads(x, sample_idx=tc.case_sample(name), return_z=True)["z"]
        assert z.tobytes() == enc.forward(x, model_output=True).tobytes()
        assert tr.encoder().forward(x).tobytes() == enc.forward(x).tobytes()
    finally:
        tr.close()
        enc.close()


def test_grads_do_not_depend_on_what_the_gradient_vector_held(gpu):
    """Two trainers in the same state, one with a differing grads call in between: the same bytes, so
    nothing of an earlier result survives in a later one (at the depth limit, 8 layers)."""
    from image_recommender_amd import _lib
    name = "deep8"
    x = tc.case_input(name)
    other = np.ascontiguousarray(x[::-1])
    a, b = make_trainer(name), make_trainer(name)
    try:
        a.step(x)
        ga = a.grads(other)
        b.step(x)
        b.grads(x)                                   # a differing call in between
        gb = b.grads(other)
        for k in ("weights", "biases", "ln_weights", "ln_biases"):
            for u, v in zip(ga[k], gb[k]):
                assert np.isfinite(u).all() and u.tobytes() == v.tobytes(), k
        assert ga["losses"] == gb["losses"]
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name", ["ref_small", "deep8"])
def test_three_adam_steps_on_the_devices_own_gradients(gpu, name):
    from image_recommender_amd import _lib
    tr = make_trainer(name)
    x = tc.case_input(name)
    try:
        for t in (1, 2, 3):
            prev = tuple(flat(tr.get_state(w)) for w in (_lib.VLADTRAIN_PARAMS, _lib.VLADTRAIN_ADAM_M, _lib.VLADTRAIN_ADAM_V))
            g = tr.grads(x)
            grads = flat((g["weights"], g["biases"], g["ln_weights"], g["ln_biases"]))
            losses = tr.step(x)
            assert losses == g["losses"], "a step's losses are its grads call's"
            stepped = flat(tr.get_state(_lib.VLADTRAIN_GRADS))
            assert all(u.tobytes() == v.tobytes() for u, v in zip(grads, stepped)), "a step's gradients are grads'"
            new = tuple(flat(tr.get_state(w)) for w in (_lib.VLADTRAIN_PARAMS, _lib.VLADTRAIN_ADAM_M, _lib.VLADTRAIN_ADAM_V))
            bad = tc.adam_failures(prev, grads, new, t)
            assert bad == [], (t, bad[:5])
            assert tr.step_count == t
            assert any(u.tobytes() != v.tobytes() for u, v in zip(prev[0], new[0]))
    finally:
        tr.close()


def test_two_trainers_two_streams_and_the_chunk_knob_end_in_equal_bytes(gpu):
    import torch
    name = "ref_small"
    x = tc.case_input(name)
    xd = torch.from_numpy(np.array(x)).cuda()

    def run(how):
        tr = make_trainer(name)
        old = os.environ.get("IMGREC_VLADENC_CHUNK_ROWS")
        try:
            if how == "knob":
                os.environ["IMGREC_VLADENC_CHUNK_ROWS"] = "50"          # read when a call starts
            losses = []
            if how == "stream":
                st = torch.cuda.Stream()
                st.wait_stream(torch.cuda.current_stream())
                for _ in range(5):
                    losses.append(tr.step_device(xd.data_ptr(), x.shape[0], stream=st.cuda_stream))
            else:
                for _ in range(5):
                    losses.append(tr.step(x))
            return losses, state_bytes(tr), tr.state_dict()
        finally:
            if how == "knob":
                if old is None:
                    os.environ.pop("IMGREC_VLADENC_CHUNK_ROWS", None)
                else:
                    os.environ["IMGREC_VLADENC_CHUNK_ROWS"] = old
            tr.close()
    base = run("host")
    assert len(set(base[0])) == 5, "five steps, five different losses"
    for how in ("host", "stream", "knob"):
        got = run(how)
        assert got[0] == base[0], how
        assert got[1] == base[1], how
        assert all((got[2][k] == base[2][k]).all() for k in base[2]), how


def test_fit_lowers_the_correlation_loss_and_follows_the_float64_trajectory(gpu):
    name = "tiny"
    x = tc.case_input(name)
    tr = make_trainer(name, dropout=0.0)
    lines = []
    try:
        hist = tr.fit(iter([x] * 30 + []), epochs=32, log=lines.append)
    finally:
        tr.close()
    assert len(hist) == 30 and len(lines) == 32 and lines[-1] == "No data found in epoch"
    assert lines[0] == f"Epoch   1/32 - loss={hist[0][0]:.5f}, corr={hist[0][1]:.5f}, umap={hist[0][2]:.5f}"
    print("corr:", " ".join(f"{h[1]:.4f}" for h in hist))
    assert hist[-1][1] < hist[0][1]
    want = tc.trajectory64(name, 3)
    tol = tc.tolerances(name)
    for t in range(3):
        for k, got, ref in zip(tc.LOSS_KEYS, hist[t], want[t]):
            print(f"step {t + 1} {k}: {abs(got - ref):.3e} ({tol[k]:.3e})")
            assert abs(got - ref) <= tol[k], (t, k, got, ref)


@pytest.mark.parametrize("name", ["dups", "one_layer", "subsample", "deep8"])
def test_evaluate_is_the_losses_of_grads_at_p0(gpu, name):
    tr = make_trainer(name, dropout=0.0)
    dropped = make_trainer(name, dropout=0.5) if tc.CASE[name].widths[1:-1] else None
    try:
        x, idx = tc.case_input(name), tc.case_sample(name)
        want = tr.grads(x, sample_idx=idx)["losses"]
        assert tr.evaluate(x, sample_idx=idx) == want
        if dropped is not None:
            assert dropped.evaluate(x, sample_idx=idx) == want, "eval mode has no dropout"
            assert dropped.grads(x, sample_idx=idx)["losses"] != want
        if idx is not None:
            assert tr.evaluate(x, sample_idx=np.sort(idx)) == want, "the order of the sample does not matter"
            assert tr.evaluate(x)[2] == want[2] and tr.evaluate(x)[1] != want[1], "umap is over the whole batch"
    finally:
        tr.close()
        if dropped is not None:
            dropped.close()


def test_save_then_load_gives_the_encoders_bytes(gpu, tmp_path):
    from image_recommender_amd.vlad_encoder import VladEncoder
    name = "odd"
    x = tc.case_input(name)
    tr = make_trainer(name)
    try:
        for _ in range(2):
            tr.step(x)
        tr.save(tmp_path / "sift_vlad_encoder.pt")
        a, b = VladEncoder.load(tmp_path / "sift_vlad_encoder.pt"), tr.encoder()
        p = tc.case_params(name)
        assert any((u != v).any() for u, v in zip(a._W, p.W)), "the saved weights are the trained ones"
        assert a.forward(x).tobytes() == b.forward(x).tobytes()
        a.close()
        b.close()
    finally:
        tr.close()


def test_fit_images_equals_the_host_round_trip(gpu):
    from image_recommender_amd.vlad import SoftVLAD
    from tests import vlad_check as vc
    cs = vc.CASE["sift"]
    x, off, c = vc.case_data("sift")
    descs = [x[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    sv = SoftVLAD(c, nn=cs.nn, sigma=cs.sigma)
    assert sv.dim == 32768 and len(descs) >= 2
    a, b = make_trainer("ref_full"), make_trainer("ref_full")
    try:
        ha = a.fit_images(sv, [descs, descs], epochs=2, log=None)
        vlad = sv.encode(descs)
        hb = b.fit([vlad, vlad], epochs=2, log=None)
        assert ha == hb and len(ha) == 2 and a.step_count == 2
        assert state_bytes(a) == state_bytes(b)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("I,J,K", [(37, 1000, 67), (130, 131, 1024), (5, 3, 2)])
def test_product_alone(gpu, I, J, K):
    """vladtrain_product_device, the GEMM every gradient runs on: unsplit with a ragged depth, split,
    under one tile; against float64 within the fp32 bound of any summation order; twice, byte-equal."""
    import ctypes as C
    import torch
    from image_recommender_amd import _lib
    from tests.vladenc_check import U
    rng = np.random.default_rng(I + J + K)
    A, B = rng.standard_normal((I, K), dtype=np.float32), rng.standard_normal((J, K), dtype=np.float32)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    outs = []
    for _ in range(2):
        Cd = torch.full((I + 1, J), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().vladtrain_product_device(
            C.c_void_p(Ad.data_ptr()), I, C.c_void_p(Bd.data_ptr()), J, K, C.c_void_p(Cd.data_ptr()),
            C.c_void_p(torch.cuda.current_stream().cuda_stream or None)), "vladtrain_product_device")
        torch.cuda.synchronize()
        assert torch.isnan(Cd[I]).all(), "written past the output"
        outs.append(Cd[:I].cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    want = A.astype(np.float64) @ B.astype(np.float64).T
    bound = (K + 1) * U * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T)
    assert (np.abs(outs[0] - want) <= bound).all()


def test_batches_outside_the_limits_are_rejected_cleanly(trainers):
    import ctypes as C
    from image_recommender_amd import _lib
    tr = trainers("tiny")
    lib, h = _lib.load(), tr._handle()
    x = np.zeros((4097, 40), np.float32)
    losses = np.zeros(3, np.float32)
    before = state_bytes(tr)
    for n in (1, 4097, 0, -1):
        rc = lib.vladtrain_step(h, C.c_void_p(x.ctypes.data), n, None, 0, C.c_void_p(losses.ctypes.data))
        assert rc == _lib.KNN_EINVAL and "n must be" in _lib.last_error()
    idx = np.array([0, 1, 1], np.int32)
    rc = lib.vladtrain_step(h, C.c_void_p(x.ctypes.data), 5, C.c_void_p(idx.ctypes.data), 3, C.c_void_p(losses.ctypes.data))
    assert rc == _lib.KNN_EINVAL and "twice" in _lib.last_error()
    idx[2] = 5
    rc = lib.vladtrain_eval(h, C.c_void_p(x.ctypes.data), 5, C.c_void_p(idx.ctypes.data), 3, C.c_void_p(losses.ctypes.data))
    assert rc == _lib.KNN_EINVAL and "not a row" in _lib.last_error()
    with pytest.raises(ValueError):
        tr.step(x[:1])
    with pytest.raises(ValueError):
        tr.step(x)
    assert tr.step_count == 0 and state_bytes(tr) == before
    assert np.isfinite(tr.evaluate(tc.case_input("tiny"))).all()
