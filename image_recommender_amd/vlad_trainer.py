"""Training of the SIFT-VLAD MLP encoder (include/imgrec_vladtrain.h, csrc/vladtrain.hip).

The reference cannot store a SIFT vector before ``load_train_encoder_on_sample`` has trained
``SIFTVLADEncoder`` (``vector_scripts/create_sift_vector.py:345-414``): 400 steps of
``2.0 * loss_corr + 0.25 * loss_umap`` over the pairwise distances of a batch of VLAD vectors and of
their codes, with Adam.  ``VladEncoderTrainer`` runs that step in HIP kernels: the forward with
dropout, both losses, the backward and Adam, exact fp32 products and float64 reductions in a fixed
order, so two runs from the same seed end in the same bytes.

    vlad = SoftVLAD(np.load("sift_codebook.npy"))
    trainer = VladEncoderTrainer()                                  # the reference's widths and settings
    trainer.fit_images(vlad, descriptor_batches, epochs=400)        # VLAD vectors never leave the device
    trainer.save("sift_vlad_encoder.pt")                            # VladEncoder.load / torch load_state_dict
    enc = trainer.encoder()

===============================================  =====================================================
reference                                        here
===============================================  =====================================================
``SIFTVLADEncoder(...)`` + ``optim.Adam(...)``   ``VladEncoderTrainer(widths, dropout, lr, ...)``
one pass of the loop body (``:393-404``)         ``step(X)`` / ``step_device(x_ptr, n, stream)``
``randperm(n)[:1024]`` inside ``loss_corr``      ``sample_idx`` drawn from (seed, step), or passed in
the epoch loop and its log line                  ``fit(batches, epochs=400)``
``compute_vectors`` + ``np.stack`` per epoch     ``fit_images(vlad, descriptor_batches)``
``torch.save(model.state_dict(), path)``         ``save(path)`` (the same keys)
``autoencoder/encoder_test.py``'s correlation    ``evaluate(X)``
===============================================  =====================================================

There is no NumPy fallback: without the native library every call raises.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import (KnnError, VLADENC_MAX_IN, VLADENC_MAX_LAYERS, VLADENC_MAX_WIDTH, VLADTRAIN_ADAM_M,
                   VLADTRAIN_ADAM_V, VLADTRAIN_GRADS, VLADTRAIN_MAX_BATCH, VLADTRAIN_MAX_BATCH_FLOATS,
                   VLADTRAIN_PARAMS)
from .vlad_encoder import VladEncoder, _ptr, _ptr_array

__all__ = ["VladEncoderTrainer", "dropout_keep", "KnnError"]

_M64 = (1 << 64) - 1


def _mix(v: np.ndarray) -> np.ndarray:
    v = v ^ (v >> np.uint64(30))
    v = v * np.uint64(0xbf58476d1ce4e5b9)
    v = v ^ (v >> np.uint64(27))
    v = v * np.uint64(0x94d049bb133111eb)
    return v ^ (v >> np.uint64(31))


def dropout_keep(seed: int, step: int, layer: int, rows: int, features: int, p: float) -> np.ndarray:
    """The ``(rows, features)`` keep mask (uint8, 1 = kept) of hidden layer `layer` at `step`: the
    counter-based hash that include/imgrec_vladtrain.h documents, on the host."""
    with np.errstate(over="ignore"):
        a = _mix(np.array([(int(seed) + 0x9e3779b97f4a7c15 * (int(step) + 1)) & _M64], np.uint64))
        row = np.arange(rows, dtype=np.uint64) | np.uint64(int(layer) << 32)
        b = _mix(a ^ row)
        c = _mix(b[:, None] + np.arange(features, dtype=np.uint64)[None, :])
    return ((c >> np.uint64(40)) >= np.uint64(math.floor(float(p) * 2.0 ** 24))).astype(np.uint8)


class VladEncoderTrainer:
    """A trainer of ``Linear -> LayerNorm -> Mish -> Dropout -> ... -> Linear`` with ``widths[l]`` inputs
    and ``widths[l + 1]`` outputs per layer.  Without ``params`` the initial parameters follow
    ``nn.Linear``'s and ``nn.LayerNorm``'s default distributions (U(+-1 / sqrt(in)), ones, zeros), drawn
    with numpy from ``seed``; ``params = (weights, biases, ln_weights, ln_biases)`` as ``VladEncoder``'s.
    ``seed`` also keys the dropout masks and the ``sample_k`` subsample."""

    def __init__(self, widths=(32768, 669, 317, 128), dropout: float = 0.1, lr: float = 1e-3,
                 weight_decay: float = 1e-5, betas=(0.9, 0.999), eps: float = 1e-8, corr_weight: float = 2.0,
                 umap_weight: float = 0.25, temperature: float = 1.5, sample_k: int = 1024, seed: int = 0,
                 device: int = -1, ln_eps: float = 1e-5, params=None):
        widths = tuple(int(w) for w in widths)
        if not 2 <= len(widths) <= VLADENC_MAX_LAYERS + 1:
            raise ValueError(f"expected 2 to {VLADENC_MAX_LAYERS + 1} widths, got {len(widths)}")
        if min(widths) < 1 or widths[0] > VLADENC_MAX_IN or max(widths[1:]) > VLADENC_MAX_WIDTH:
            raise ValueError(f"widths out of range (input <= {VLADENC_MAX_IN}, others <= {VLADENC_MAX_WIDTH}): {widths}")
        betas = tuple(float(b) for b in betas)
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"betas must be two values in [0, 1) (got {betas})")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout must be in [0, 1) (got {dropout})")
        for name, v, positive in (("lr", lr, False), ("weight_decay", weight_decay, False), ("eps", eps, True),
                                  ("temperature", temperature, True), ("ln_eps", ln_eps, False)):
            v = float(v)
            if not math.isfinite(v) or v < 0.0 or (positive and v == 0.0):
                raise ValueError(f"{name} must be finite and {'> 0' if positive else '>= 0'} (got {v})")
        if not (math.isfinite(float(corr_weight)) and math.isfinite(float(umap_weight))):
            raise ValueError("the loss weights must be finite")
        if int(sample_k) < 2:
            raise ValueError(f"sample_k must be at least 2 (got {sample_k})")
        if int(seed) < 0:
            raise ValueError(f"seed must not be negative (got {seed})")
        self.widths = widths
        self.dropout, self.lr, self.weight_decay, self.betas, self.eps = float(dropout), float(lr), float(weight_decay), betas, float(eps)
        self.corr_weight, self.umap_weight, self.temperature = float(corr_weight), float(umap_weight), float(temperature)
        self.sample_k, self.seed, self.device, self.ln_eps = int(sample_k), int(seed), int(device), float(ln_eps)
        nl = len(widths) - 1
        if params is None:
            rng = np.random.default_rng(self.seed)
            W, b = [], []
            for l in range(nl):
                bound = 1.0 / math.sqrt(widths[l])
                W.append(rng.uniform(-bound, bound, (widths[l + 1], widths[l])).astype(np.float32))
                b.append(rng.uniform(-bound, bound, widths[l + 1]).astype(np.float32))
            g = [np.ones(widths[l + 1], np.float32) for l in range(nl - 1)]
            be = [np.zeros(widths[l + 1], np.float32) for l in range(nl - 1)]
        else:
            # VladEncoder's constructor is the shape and finiteness check
            enc = VladEncoder(*params, ln_eps=self.ln_eps)
            if enc.widths != widths:
                raise ValueError(f"the parameters have widths {enc.widths}, expected {widths}")
            W, b, g, be = enc._W, enc._b, enc._g, enc._be
        self._init = (W, b, g, be)
        self._h = None
        self._made_on = None         # the device index behind device = -1, known once the handle exists

    @classmethod
    def from_state_dict(cls, sd, **kwargs) -> "VladEncoderTrainer":
        """Continue from a torch module's ``state_dict`` (the reference's keys); fresh Adam moments."""
        enc = VladEncoder.from_state_dict(sd, ln_eps=kwargs.get("ln_eps", 1e-5))
        return cls(widths=enc.widths, params=(enc._W, enc._b, enc._g, enc._be), **kwargs)

    # ---- the native handle -------------------------------------------------------------------
    def _config(self) -> _lib.VladTrainConfig:
        return _lib.VladTrainConfig(self.dropout, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                    self.corr_weight, self.umap_weight, self.temperature, self.ln_eps, self.seed)

    def _handle(self) -> C.c_void_p:
        if self._h is None:
            lib = _lib.load()
            h = C.c_void_p()
            W, b, g, be = self._init
            widths = (C.c_int * len(self.widths))(*self.widths)
            cfg = self._config()
            _lib.check(lib.vladtrain_create(len(W), widths, _ptr_array(W), _ptr_array(b), _ptr_array(g), _ptr_array(be),
                                            C.byref(cfg), self.device, C.byref(h)), "vladtrain_create")
            self._h = h
            if self.device < 0:
                import torch
                self._made_on = torch.cuda.current_device()
        return self._h

    def close(self) -> None:
        if self._h is not None:
            _lib.load().vladtrain_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def in_dim(self) -> int:
        return self.widths[0]

    @property
    def out_dim(self) -> int:
        return self.widths[-1]

    @property
    def hidden_dim(self) -> int:
        return sum(self.widths[1:-1])

    @property
    def step_count(self) -> int:
        """Steps taken so far."""
        if self._h is None:
            return 0
        s = C.c_int64()
        _lib.check(_lib.load().vladtrain_get_step(self._h, C.byref(s)), "vladtrain_get_step")
        return int(s.value)

    @step_count.setter
    def step_count(self, step: int) -> None:
        _lib.check(_lib.load().vladtrain_set_step(self._handle(), int(step)), "vladtrain_set_step")

    # ---- state -------------------------------------------------------------------------------
    def _empty(self):
        nl = len(self.widths) - 1
        W = [np.empty((self.widths[l + 1], self.widths[l]), np.float32) for l in range(nl)]
        b = [np.empty(self.widths[l + 1], np.float32) for l in range(nl)]
        g = [np.empty(self.widths[l + 1], np.float32) for l in range(nl - 1)]
        be = [np.empty(self.widths[l + 1], np.float32) for l in range(nl - 1)]
        return W, b, g, be

    def get_state(self, which: int = VLADTRAIN_PARAMS):
        """``(weights, biases, ln_weights, ln_biases)`` of the parameters, an Adam moment
        (``VLADTRAIN_ADAM_M`` / ``_V``) or the last gradients (``VLADTRAIN_GRADS``), as numpy copies."""
        if self._h is None and which == VLADTRAIN_PARAMS:
            return tuple([a.copy() for a in t] for t in self._init)
        W, b, g, be = self._empty()
        _lib.check(_lib.load().vladtrain_get_state(self._handle(), int(which), _ptr_array(W), _ptr_array(b), _ptr_array(g),
                                                   _ptr_array(be)), "vladtrain_get_state")
        return W, b, g, be

    def set_state(self, which: int, state) -> None:
        W, b, g, be = self._empty()
        for dst, src in zip((W, b, g, be), state):
            if len(dst) != len(src):
                raise ValueError(f"expected {len(dst)} arrays, got {len(src)}")
            for d, s in zip(dst, src):
                s = np.asarray(s)
                if s.shape != d.shape:
                    raise ValueError(f"expected shape {d.shape}, got {s.shape}")
                d[...] = s
        _lib.check(_lib.load().vladtrain_set_state(self._handle(), int(which), _ptr_array(W), _ptr_array(b), _ptr_array(g),
                                                   _ptr_array(be)), "vladtrain_set_state")

    def state_dict(self) -> "OrderedDict":
        """The parameters under the reference's keys: ``encoder.{4 l}.weight/bias`` for Linear l,
        ``encoder.{4 l + 1}.weight/bias`` for its LayerNorm; torch tensors."""
        import torch
        W, b, g, be = self.get_state(VLADTRAIN_PARAMS)
        sd = OrderedDict()
        for l in range(len(W)):
            sd[f"encoder.{4 * l}.weight"] = torch.from_numpy(W[l])
            sd[f"encoder.{4 * l}.bias"] = torch.from_numpy(b[l])
            if l < len(g):
                sd[f"encoder.{4 * l + 1}.weight"] = torch.from_numpy(g[l])
                sd[f"encoder.{4 * l + 1}.bias"] = torch.from_numpy(be[l])
        return sd

    def save(self, path) -> None:
        """``torch.save(state_dict(), path)``: a ``sift_vlad_encoder.pt`` for ``VladEncoder.load`` and for
        the reference's ``load_state_dict``."""
        import torch
        torch.save(self.state_dict(), path)

    def encoder(self) -> VladEncoder:
        """A ``VladEncoder`` of the current weights."""
        W, b, g, be = self.get_state(VLADTRAIN_PARAMS)
        return VladEncoder(W, b, g, be, ln_eps=self.ln_eps, device=self.device)

    # ---- one batch ---------------------------------------------------------------------------
    def draw_sample(self, n: int, step: int | None = None):
        """The ``sample_k`` rows ``loss_corr`` is restricted to when ``n > sample_k`` (the reference's
        ``randperm(n)[:sample_k]``), a function of (seed, step); ``None`` for a smaller batch."""
        if n <= self.sample_k:
            return None
        step = self.step_count if step is None else int(step)
        return np.random.default_rng([self.seed, step]).permutation(n)[:self.sample_k].astype(np.int32)

    def _sample_args(self, n, sample_idx):
        if sample_idx is None:
            sample_idx = self.draw_sample(n)
        if sample_idx is None:
            return None, None, 0
        idx = np.ascontiguousarray(sample_idx, dtype=np.int32).ravel()
        return idx, _ptr(idx), int(idx.size)

    def _batch(self, X):
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.in_dim:
            raise ValueError(f"X: expected (n, {self.in_dim}), got shape {X.shape}")
        self._check_n(int(X.shape[0]))
        return np.ascontiguousarray(X, dtype=np.float32)

    def _check_n(self, n):
        if not 2 <= n <= VLADTRAIN_MAX_BATCH or n * self.in_dim > VLADTRAIN_MAX_BATCH_FLOATS:
            raise ValueError(f"a batch has 2 to {VLADTRAIN_MAX_BATCH} rows and at most {VLADTRAIN_MAX_BATCH_FLOATS} "
                             f"values (got {n} rows of {self.in_dim})")

    def step(self, X, sample_idx=None):
        """One training step on the host batch ``X`` ``(n, in_dim)``.  Returns ``(loss, corr, umap)``."""
        X = self._batch(X)
        idx, ip, k = self._sample_args(X.shape[0], sample_idx)
        losses = np.empty(3, np.float32)
        _lib.check(_lib.load().vladtrain_step(self._handle(), _ptr(X), X.shape[0], ip, k, _ptr(losses)), "vladtrain_step")
        return tuple(float(v) for v in losses)

    def step_device(self, x_ptr: int, n: int, stream: int = 0, sample_idx=None, losses_ptr: int = 0):
        """One step over device-resident rows on `stream`.  With ``losses_ptr`` (device float[3]) the
        call never waits and returns None; otherwise it waits for the step and returns
        ``(loss, corr, umap)``."""
        n = int(n)
        self._check_n(n)
        if not x_ptr:
            raise ValueError("step_device: x_ptr must not be 0")
        idx, ip, k = self._sample_args(n, sample_idx)
        lib = _lib.load()
        if losses_ptr:
            _lib.check(lib.vladtrain_step_device(self._handle(), C.c_void_p(x_ptr), n, ip, k, C.c_void_p(stream or None),
                                                 C.c_void_p(losses_ptr)), "vladtrain_step_device")
            return None
        import torch
        h = self._handle()
        with torch.cuda.device(self._torch_device(torch)):
            ld = torch.empty(3, dtype=torch.float32, device="cuda")
            _lib.check(lib.vladtrain_step_device(h, C.c_void_p(x_ptr), n, ip, k, C.c_void_p(stream or None),
                                                 C.c_void_p(ld.data_ptr())), "vladtrain_step_device")
            torch.cuda.synchronize()
            return tuple(float(v) for v in ld.cpu().numpy())

    def grads(self, X, sample_idx=None, return_masks: bool = False, return_z: bool = False) -> dict:
        """The step's losses and every parameter's gradient at the current step counter, without the
        update: ``{"losses": (loss, corr, umap), "weights", "biases", "ln_weights", "ln_biases"}`` and, on
        request, ``"masks"`` ``(n, hidden_dim)`` uint8 (1 = kept) and ``"z"`` ``(n, out_dim)``, the model output."""
        X = self._batch(X)
        n = X.shape[0]
        idx, ip, k = self._sample_args(n, sample_idx)
        losses = np.full(3, np.nan, np.float32)
        z = np.full((n, self.out_dim), np.nan, np.float32) if return_z else None
        masks = np.full((n, self.hidden_dim), 255, np.uint8) if return_masks else None
        _lib.check(_lib.load().vladtrain_grads(
            self._handle(), _ptr(X), n, ip, k, _ptr(losses), _ptr(z) if return_z else None,
            _ptr(masks) if return_masks and masks.size else None), "vladtrain_grads")
        W, b, g, be = self.get_state(VLADTRAIN_GRADS)
        out = {"losses": tuple(float(v) for v in losses), "weights": W, "biases": b, "ln_weights": g, "ln_biases": be}
        if return_masks:
            out["masks"] = masks
        if return_z:
            out["z"] = z
        return out

    def evaluate(self, X, sample_idx=None):
        """``(loss, corr, umap)`` of a batch in eval mode: no dropout, no update."""
        X = self._batch(X)
        idx, ip, k = self._sample_args(X.shape[0], sample_idx)
        losses = np.empty(3, np.float32)
        _lib.check(_lib.load().vladtrain_eval(self._handle(), _ptr(X), X.shape[0], ip, k, _ptr(losses)), "vladtrain_eval")
        return tuple(float(v) for v in losses)

    def _torch_device(self, torch) -> int:
        """The index of the device the handle lives on: `device`, or for -1 the one that was current
        when the handle was made."""
        if self.device >= 0:
            return self.device
        if self._made_on is None:
            self._handle()
        return self._made_on

    # ---- the reference's loop ------------------------------------------------------------------
    def fit(self, batches, epochs: int = 400, log=print) -> list:
        """The reference's loop: one batch of `batches` per epoch (numpy ``(n, in_dim)``, or a CUDA torch
        tensor, which is stepped where it lies); an exhausted iterator skips the epoch; one log line
        per epoch in the reference's format.  Returns the ``(loss, corr, umap)`` of every step taken."""
        it = iter(batches)
        history = []
        for epoch in range(int(epochs)):
            try:
                X = next(it)
            except StopIteration:
                if log:
                    log("No data found in epoch")
                continue
            if hasattr(X, "data_ptr") and getattr(X, "is_cuda", False):
                import torch
                if X.dim() != 2 or X.shape[1] != self.in_dim or X.dtype != torch.float32 or not X.is_contiguous():
                    raise ValueError(f"a device batch must be a contiguous float32 (n, {self.in_dim}) tensor")
                dev = self._torch_device(torch)
                if X.device.index != dev:
                    raise ValueError(f"a device batch lies on cuda:{X.device.index}, the trainer runs on cuda:{dev}")
                with torch.cuda.device(dev):         # the stream is the trainer's device's
                    res = self.step_device(X.data_ptr(), int(X.shape[0]), stream=torch.cuda.current_stream().cuda_stream)
            else:
                res = self.step(X)
            history.append(res)
            if log:
                log(f"Epoch {epoch + 1:3}/{epochs} - loss={res[0]:.5f}, corr={res[1]:.5f}, umap={res[2]:.5f}")
        return history

    def vlad_batches(self, vlad, descriptor_batches):
        """Per element of `descriptor_batches` (per-image descriptor arrays, as ``SoftVLAD.encode`` takes)
        the ``(nimg, vlad.dim)`` VLAD vectors as a CUDA tensor, from ``vlad.encode_device``."""
        if vlad.dim != self.in_dim:
            raise ValueError(f"the VLAD vectors have {vlad.dim} columns, the encoder takes {self.in_dim}")
        import torch
        for descs in descriptor_batches:
            x, off = vlad._ragged(descs)
            nimg = int(off.size - 1)
            with torch.cuda.device(self._torch_device(torch)):
                st = torch.cuda.current_stream()
                xd = torch.tensor(x, device="cuda") if x.shape[0] else torch.empty((1, vlad.d), dtype=torch.float32, device="cuda")
                od = torch.tensor(off, device="cuda")
                v = torch.empty((nimg, vlad.dim), dtype=torch.float32, device="cuda")
                vlad.encode_device(xd.data_ptr(), od.data_ptr(), nimg, int(x.shape[0]), v.data_ptr(), stream=st.cuda_stream)
            yield v

    def fit_images(self, vlad, descriptor_batches, epochs: int = 400, log=print) -> list:
        """``fit`` fed from ``SoftVLAD.encode_device``: the VLAD vectors stay on the device."""
        return self.fit(self.vlad_batches(vlad, descriptor_batches), epochs=epochs, log=log)
