"""The SIFT-VLAD MLP encoder's forward pass (include/imgrec_vladenc.h, csrc/vladenc.hip).

The reference pushes every image's 32768-d VLAD vector through ``SIFTVLADEncoder``
(``vector_scripts/create_sift_vector.py:59-77``: ``Linear(32768, 669) -> LayerNorm -> Mish ->
Linear(669, 317) -> LayerNorm -> Mish -> Linear(317, 128)``, then ``F.normalize``), and
``compute_vectors`` (``:514-521``) divides the result once more by its norm + 1e-7: that 128-d vector
is what it stores in ``sift_vectors`` and searches.  ``VladEncoder`` runs that forward pass in HIP
kernels (fp32 throughout, batch-invariant byte for byte); ``vlad_trainer.VladEncoderTrainer`` trains it.

    vlad = SoftVLAD(np.load("sift_codebook.npy"))
    enc = VladEncoder.load("sift_vlad_encoder.pt")
    vectors = enc.encode_images(vlad, [rootsift(d) for d in per_image_descriptors])   # (nimg, 128)

===============================================  =====================================================
reference                                        here
===============================================  =====================================================
``SIFTVLADEncoder`` + ``load_state_dict``        ``VladEncoder.load(path)`` / ``from_state_dict(sd)``
``encoder_model(X)`` (eval, no_grad)             ``forward(X, model_output=True)``
``compressed /= norm + 1e-7`` (stored vector)    ``forward(X)`` (the default)
VLAD on CPU workers, then ``.to(device)``        ``encode_images(vlad, descs)``: all on the device
``encoder_model.train()`` / the losses           ``vlad_trainer.VladEncoderTrainer`` (HIP kernels too)
===============================================  =====================================================

There is no NumPy fallback: without the native library every call raises.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import _lib
from ._lib import (KnnError, VLADENC_MAX_IN, VLADENC_MAX_LAYERS, VLADENC_MAX_WIDTH, VLADENC_MODEL_OUTPUT)

__all__ = ["VladEncoder", "KnnError"]

_KEY = re.compile(r"^(.*?)(\d+)\.(weight|bias)$")


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def _ptr_array(arrays) -> C.Array:
    return (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


class VladEncoder:
    """``weights[l]`` is ``(widths[l + 1], widths[l])`` (``nn.Linear``'s layout), ``biases[l]`` its bias;
    ``ln_weights[l]`` / ``ln_biases[l]`` the LayerNorm after every layer but the last, which Mish
    follows.  ``device`` is the HIP device (-1 = the current one at first use)."""

    def __init__(self, weights, biases, ln_weights, ln_biases, ln_eps: float = 1e-5, device: int = -1):
        weights, biases = list(weights), list(biases)
        ln_weights, ln_biases = list(ln_weights), list(ln_biases)
        nl = len(weights)
        if not 1 <= nl <= VLADENC_MAX_LAYERS:
            raise ValueError(f"expected 1 to {VLADENC_MAX_LAYERS} linear layers, got {nl}")
        if len(biases) != nl or len(ln_weights) != nl - 1 or len(ln_biases) != nl - 1:
            raise ValueError(f"{nl} layers need {nl} biases and {nl - 1} LayerNorm weights and biases "
                             f"(got {len(biases)}, {len(ln_weights)}, {len(ln_biases)})")

        def own(a, shape, what):
            a = np.asarray(a)
            if a.shape != shape:
                raise ValueError(f"{what}: expected shape {shape}, got {a.shape}")
            a = np.array(a, dtype=np.float32, order="C")
            if not np.isfinite(a).all():
                raise ValueError(f"{what}: not finite")
            return a

        self._W, self._b, self._g, self._be = [], [], [], []
        widths = []
        for l, w in enumerate(weights):
            w = np.asarray(w)
            if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] < 1:
                raise ValueError(f"weights[{l}]: expected an (out, in) array, got shape {w.shape}")
            if l == 0:
                widths.append(int(w.shape[1]))
            if w.shape[1] != widths[-1]:
                raise ValueError(f"weights[{l}]: {w.shape[1]} inputs after a layer of {widths[-1]} outputs")
            widths.append(int(w.shape[0]))
            self._W.append(own(w, w.shape, f"weights[{l}]"))
            self._b.append(own(biases[l], (widths[-1],), f"biases[{l}]"))
            if l < nl - 1:
                self._g.append(own(ln_weights[l], (widths[-1],), f"ln_weights[{l}]"))
                self._be.append(own(ln_biases[l], (widths[-1],), f"ln_biases[{l}]"))
        if widths[0] > VLADENC_MAX_IN:
            raise ValueError(f"input width {widths[0]} exceeds {VLADENC_MAX_IN}")
        if max(widths[1:]) > VLADENC_MAX_WIDTH:
            raise ValueError(f"a hidden or output width exceeds {VLADENC_MAX_WIDTH}: {widths}")
        self.widths = tuple(widths)
        self.ln_eps = float(ln_eps)
        if not (self.ln_eps >= 0.0 and np.isfinite(self.ln_eps)):
            raise ValueError(f"ln_eps must be finite and >= 0 (got {ln_eps})")
        self.device = int(device)
        self._h = None

    # ---- construction from torch -------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, ln_eps: float = 1e-5, device: int = -1) -> "VladEncoder":
        """From the ``state_dict`` of an ``nn.Sequential`` of Linear / LayerNorm / Mish / Dropout (the
        reference's ``encoder.0`` Linear, ``encoder.1`` LayerNorm, ``encoder.4``, ``.5``, ``.8``), walked by
        numeric index: a 2-D weight is a Linear, the 1-D weight after it that layer's LayerNorm."""
        mods: dict[int, dict] = {}
        prefix = None
        for key, val in sd.items():
            m = _KEY.match(key)
            if m is None:
                raise ValueError(f"state_dict key {key!r} is not <prefix><index>.weight or .bias")
            if prefix is None:
                prefix = m.group(1)
            if m.group(1) != prefix:
                raise ValueError(f"state_dict key {key!r} does not share the prefix {prefix!r}")
            a = val.detach().cpu().numpy() if hasattr(val, "detach") else np.asarray(val)
            mods.setdefault(int(m.group(2)), {})[m.group(3)] = a
        W, b, g, be = [], [], [], []
        for i in sorted(mods):
            mod, name = mods[i], f"{prefix}{i}"
            if "weight" not in mod:
                raise ValueError(f"state_dict key {name + '.bias'!r} has no {name + '.weight'!r}")
            w = mod["weight"]
            if w.ndim == 2:
                if len(g) < len(W):
                    raise ValueError(f"state_dict key {name + '.weight'!r}: a Linear follows a Linear without a LayerNorm")
                W.append(w)
                b.append(mod.get("bias", np.zeros(w.shape[0], np.float32)))
            elif w.ndim == 1:
                if len(g) != len(W) - 1:
                    raise ValueError(f"state_dict key {name + '.weight'!r}: a LayerNorm that follows no Linear")
                if "bias" not in mod:
                    raise ValueError(f"state_dict key {name + '.weight'!r}: a LayerNorm without a bias")
                g.append(w)
                be.append(mod["bias"])
            else:
                raise ValueError(f"state_dict key {name + '.weight'!r} has {w.ndim} dimensions")
        if not W:
            raise ValueError("state_dict holds no Linear layer")
        if len(g) != len(W) - 1:
            raise ValueError(f"state_dict key {prefix}{max(mods)}.weight: the last Linear must not be followed by a LayerNorm")
        return cls(W, b, g, be, ln_eps=ln_eps, device=device)

    @classmethod
    def load(cls, path, ln_eps: float = 1e-5, device: int = -1) -> "VladEncoder":
        """From a file written by ``torch.save(model.state_dict(), path)`` (``sift_vlad_encoder.pt``)."""
        import torch
        return cls.from_state_dict(torch.load(path, map_location="cpu", weights_only=True), ln_eps=ln_eps,
                                   device=device)

    # ---- properties --------------------------------------------------------------------------
    @property
    def in_dim(self) -> int:
        return self.widths[0]

    @property
    def out_dim(self) -> int:
        return self.widths[-1]

    @property
    def hidden_dim(self) -> int:
        """Columns of ``hidden``: the hidden widths' sum."""
        return sum(self.widths[1:-1])

    def _handle(self) -> C.c_void_p:
        """The native encoder, made on first use (the weights are uploaded once)."""
        if self._h is None:
            lib = _lib.load()
            h = C.c_void_p()
            widths = (C.c_int * len(self.widths))(*self.widths)
            _lib.check(lib.vladenc_create(
                len(self._W), widths, _ptr_array(self._W), _ptr_array(self._b), _ptr_array(self._g),
                _ptr_array(self._be), self.ln_eps, self.device, C.byref(h)), "vladenc_create")
            self._h = h
        return self._h

    def close(self) -> None:
        if self._h is not None:
            _lib.load().vladenc_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host arrays -------------------------------------------------------------------------
    def forward(self, x, model_output: bool = False, return_hidden: bool = False):
        """``x``: ``(n, in_dim)`` (or one vector).  Returns ``(n, out_dim)`` float32: the stored vector, or
        with ``model_output`` the model's own output (``F.normalize`` only).  With ``return_hidden`` also
        ``(n, hidden_dim)``: every hidden layer's post-Mish activation, concatenated."""
        x = np.asarray(x)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        if x.ndim != 2 or x.shape[1] != self.in_dim:
            raise ValueError(f"x: expected (n, {self.in_dim}), got shape {x.shape}")
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = int(x.shape[0])
        out = np.empty((n, self.out_dim), np.float32)
        hidden = np.empty((n, self.hidden_dim), np.float32) if return_hidden else None
        _lib.check(_lib.load().vladenc_forward(
            self._handle(), _ptr(x), n, VLADENC_MODEL_OUTPUT if model_output else 0, _ptr(out),
            _ptr(hidden) if return_hidden and hidden.size else None), "vladenc_forward")
        if one:
            out = out[0]
        return (out, hidden) if return_hidden else out

    # ---- device-resident ---------------------------------------------------------------------
    def forward_device(self, x_ptr: int, n: int, out_ptr: int, stream: int = 0, model_output: bool = False,
                       hidden_ptr: int = 0) -> None:
        """The forward pass over device-resident ``x`` (n x in_dim float32) into ``out`` (n x out_dim) and,
        if given, ``hidden`` (n x hidden_dim) on `stream`; never waits."""
        n = int(n)
        if n < 0:
            raise ValueError(f"n must not be negative (got {n})")
        if n > 0 and (not x_ptr or not out_ptr):
            raise ValueError("forward_device: x_ptr and out_ptr must not be 0")
        _lib.check(_lib.load().vladenc_forward_device(
            self._handle(), C.c_void_p(x_ptr or None), n, VLADENC_MODEL_OUTPUT if model_output else 0,
            C.c_void_p(out_ptr or None), C.c_void_p(hidden_ptr or None), C.c_void_p(stream or None)),
            "vladenc_forward_device")

    def encode_images(self, vlad, descs, model_output: bool = False) -> np.ndarray:
        """Descriptors to stored vectors: ``vlad.encode_device`` into a device buffer, then
        ``forward_device`` on the same stream; the ``vlad.dim``-d vectors never leave the device.
        ``descs`` as for ``SoftVLAD.encode``; an image without descriptors goes through as the zero VLAD
        vector, as in the reference.  Returns ``(nimg, out_dim)`` float32."""
        if vlad.dim != self.in_dim:
            raise ValueError(f"the VLAD vectors have {vlad.dim} columns, the encoder takes {self.in_dim}")
        x, off = vlad._ragged(descs)
        nimg = int(off.size - 1)
        if nimg == 0:
            return np.empty((0, self.out_dim), np.float32)
        import torch
        with torch.cuda.device(self.device if self.device >= 0 else torch.cuda.current_device()):
            st = torch.cuda.current_stream()
            xd = torch.tensor(x, device="cuda") if x.shape[0] else torch.empty((1, vlad.d), dtype=torch.float32, device="cuda")
            od = torch.tensor(off, device="cuda")
            v = torch.empty((nimg, vlad.dim), dtype=torch.float32, device="cuda")
            out = torch.empty((nimg, self.out_dim), dtype=torch.float32, device="cuda")
            vlad.encode_device(xd.data_ptr(), od.data_ptr(), nimg, int(x.shape[0]), v.data_ptr(), stream=st.cuda_stream)
            self.forward_device(v.data_ptr(), nimg, out.data_ptr(), stream=st.cuda_stream, model_output=model_output)
            return out.cpu().numpy()
