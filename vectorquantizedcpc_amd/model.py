"""Drop-in ``Encoder`` / ``VQEmbeddingEMA`` / ``CPCLoss`` for the reference's ``model.py`` (inference and scoring paths).

Same constructor (``Encoder(conf: ConfEncoder)``, ``model.py:17-34``), same
``state_dict()`` key set (``model.py:43-57``), same ``encode`` / ``forward`` signatures
(``model.py:59-86``).  The torch sub-modules below only HOLD the parameters (so
``load_state_dict(checkpoint["encoder"])``, ``.to(device)``, ``.eval()`` and the
``encoder.encoder[-1]`` forward hook of ``encode.py:34-40`` keep working); all arithmetic
runs in ``libvqcpc_hip.so`` through the C ABI of ``include/vqcpc.h``.
"""
import weakref
from dataclasses import dataclass
from itertools import chain
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib

MISSING = "???"   # stands where the reference uses omegaconf.MISSING (model.py:6)


@dataclass
class ConfEncoder:
    """``model.py:17-31``."""
    in_channels: int = MISSING
    channels: int = MISSING
    n_embeddings: int = MISSING
    z_dim: int = MISSING
    c_dim: int = MISSING


def _vq_eval(h, xf: Tensor, q: Optional[Tensor] = None, idx: Optional[Tensor] = None, stats: bool = True):
    """The eval VQ step (``model.py:103-134``, ``:147-153``) on the native handle ``h`` over rows xf (N, z_dim) fp32, contiguous:
    ``vqcpc_encoder_vq_encode`` -- unless the caller has ``q`` and ``idx`` of these rows already (``vqcpc_encoder_encode`` gives
    them) -- then, with ``stats``, ``vqcpc_encoder_forward_stats``.  -> (q, idx, z_st, [loss, perplexity]), the last two None
    without ``stats``.  The caller chooses the handle, and with it the moment a stale one is rebuilt."""
    lib, dev, N = _lib.load(), xf.device, xf.size(0)
    z_st = st = None
    with _lib.device_guard(dev):
        if q is None:
            q = torch.empty_like(xf)
            idx = torch.empty(N, dtype=torch.int64, device=dev)
            _lib.check(lib.vqcpc_encoder_vq_encode(h, xf.data_ptr(), N, q.data_ptr(), idx.data_ptr(), _lib.current_stream()))
        if stats:
            z_st, st = torch.empty_like(xf), torch.empty(2, device=dev)
            _lib.check(lib.vqcpc_encoder_forward_stats(h, xf.data_ptr(), q.data_ptr(), idx.data_ptr(), N, z_st.data_ptr(),
                                                       st[0:].data_ptr(), st[1:].data_ptr(), _lib.current_stream()))
    return q, idx, z_st, st


class VQEmbeddingEMA(nn.Module):
    """Codebook buffers (``model.py:89-101``) + the reference's public ``encode`` / ``forward`` (``model.py:103-155``) as thin
    wrappers over the owning ``Encoder``'s native handle (the same VQ kernel ``Encoder.encode`` runs).  In training mode
    ``forward`` also runs the EMA update of ``model.py:136-145`` (``vqcpc_encoder_vq_adapt``): no gradient is involved, the three
    buffers are updated IN PLACE (the reference rebinds them) and the native handle follows without being rebuilt.  The
    straight-through gradient of ``model.py:150`` is not provided here: ``Encoder.quantize(z_pre, differentiable=True)`` has it.
    """

    def __init__(self, n_embeddings, embedding_dim, commitment_cost=0.25, decay=0.999, epsilon=1e-5):
        super().__init__()
        self.commitment_cost, self.decay, self.epsilon = commitment_cost, decay, epsilon
        init_bound = 1 / 512
        embedding = torch.empty(n_embeddings, embedding_dim).uniform_(-init_bound, init_bound)
        self.register_buffer("embedding", embedding)
        self.register_buffer("ema_count", torch.zeros(n_embeddings))
        self.register_buffer("ema_weight", self.embedding.clone())
        self._owner = None                              # weakref to the Encoder that holds the native handle

    def __getstate__(self):                             # copy.deepcopy / pickle: the owner re-links itself
        d = self.__dict__.copy()
        d["_owner"] = None
        return d

    def _flat(self, x: Tensor):
        """The owning Encoder and x as contiguous fp32 rows (N, D) (``model.py:124``), after the checks every entry shares."""
        owner = self._owner() if self._owner is not None else None
        if owner is None:
            raise RuntimeError("VQEmbeddingEMA: the MI355X path serves the codebook through its owning Encoder "
                               "(construct it as Encoder(conf).codebook)")
        _lib.require_cuda(x, "x")
        _lib.require_same_device(x, self.embedding, "x")
        D = self.embedding.size(1)
        if x.dim() < 2 or x.size(-1) != D:
            raise RuntimeError(f"expected x of shape (Batch, Time, {D}), got {tuple(x.shape)}")
        return owner, x.detach().to(torch.float32).reshape(-1, D).contiguous()

    @torch.no_grad()
    def encode(self, x: Tensor):
        """``model.py:103-115``: (quantized, indices (Batch, Time))."""
        owner, xf = self._flat(x)
        q, idx, _, _ = _vq_eval(owner._native(), xf, stats=False)
        return q.view_as(x), idx.view(x.size(0), x.size(1))

    def forward(self, x: Tensor):
        """``model.py:117-155``: (x + (q - x), 0.25 * mse, perplexity), all three from the codebook as it is on entry.  In
        training mode the EMA update (``model.py:136-145``) follows, in place; no gradient flows either way."""
        if self.training:
            if torch.is_grad_enabled() and x.requires_grad:
                raise NotImplementedError("VQEmbeddingEMA: the straight-through gradient of training mode (model.py:150) is "
                                          "not implemented; the codebook update itself needs none -- call it under "
                                          "torch.no_grad() or on a detached x")
            with torch.no_grad():
                owner, xf = self._flat(x)
                z_st = torch.empty_like(xf)
                stats = owner._adapt_rows(xf, z_st)
            return z_st.view_as(x), stats[0], stats[1]
        with torch.no_grad():
            owner, xf = self._flat(x)
            _, _, z_st, stats = _vq_eval(owner._native(), xf)
        return z_st.view_as(x), stats[0], stats[1]


class Encoder(_lib.NativeModule):
    """Spec-Conv1d/k4s2-LN-ReLU-[FC-LN-ReLU]x4-FC-VQ + LSTM (``model.py:33-86``) on MI355X."""

    def __init__(self, conf: ConfEncoder):
        super().__init__()
        self.conf = conf
        self.conv = nn.Conv1d(conf.in_channels, conf.channels, 4, 2, 1, bias=False)
        block = lambda: [nn.Linear(conf.channels, conf.channels, bias=False), nn.LayerNorm(conf.channels), nn.ReLU(True)]
        self.encoder = nn.Sequential(nn.LayerNorm(conf.channels), nn.ReLU(True),
                                     *chain.from_iterable(block() for _ in range(4)),
                                     nn.Linear(conf.channels, conf.z_dim))
        self.codebook = VQEmbeddingEMA(conf.n_embeddings, conf.z_dim)
        self.codebook._owner = weakref.ref(self)
        self.rnn = nn.LSTM(conf.z_dim, conf.c_dim, batch_first=True)

    # ------------------------------------------------------------------ native handle (lifecycle: _lib.NativeModule)
    _NAME, _CREATE, _DESTROY, _SET_OPTION = "Encoder", "vqcpc_encoder_create", "vqcpc_encoder_destroy", "vqcpc_encoder_set_option"
    _WEIGHT_NAMES = (["conv.weight"] + [f"encoder.{n}.{k}" for n in (0, 3, 6, 9, 12) for k in ("weight", "bias")] +
                     [f"encoder.{n}.weight" for n in (2, 5, 8, 11)] + ["encoder.14.weight", "encoder.14.bias",
                      "codebook.embedding", "rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0"])

    def _weights(self, p):
        w = _lib.fill_front(_lib.EncoderWeights(), [p(n) for n in self._FRONT_NAMES])
        w.codebook = p("codebook.embedding")
        w.rnn_w_ih, w.rnn_w_hh = p("rnn.weight_ih_l0"), p("rnn.weight_hh_l0")
        w.rnn_b_ih, w.rnn_b_hh = p("rnn.bias_ih_l0"), p("rnn.bias_hh_l0")
        c = self.conf
        w.in_channels, w.channels, w.n_embeddings, w.z_dim, w.c_dim = (
            c.in_channels, c.channels, c.n_embeddings, c.z_dim, c.c_dim)
        return w

    def __setstate__(self, state):
        super().__setstate__(state)
        self.codebook._owner = weakref.ref(self)

    def last_schedule(self) -> int:
        """Schedule the front end of the last ``encode`` / ``stage`` call ran (``vqcpc_encoder_last_schedule``): 2 the six
        column-split launches, 1 the one-launch fused kernel, 0 the layered kernels; -1 before the first call."""
        return -1 if self._handle is None else int(_lib.load().vqcpc_encoder_last_schedule(self._handle))

    def workspace_bytes(self) -> int:
        """Device bytes of the native handle's grow-only work buffers (``vqcpc_encoder_workspace_bytes``): front-end activations,
        statistics and the work spaces of the codebook update, of the context gradients and of the front-end gradients -- the peak of
        the calls so far, weights not counted."""
        import ctypes
        n = ctypes.c_uint64()
        _lib.check(_lib.load().vqcpc_encoder_workspace_bytes(self._native(), ctypes.byref(n)))
        return int(n.value)

    def check(self):
        """Synchronise the current stream and raise ``RuntimeError`` if the resident context scan of the last ``encode``
        gave up on an in-kernel exchange (``vqcpc_encoder_check``): that call's ``c`` is incomplete, the handle has fallen
        back to one launch per time step, and repeating the call gives the right result."""
        if self._handle is None:
            return
        torch.cuda.current_stream().synchronize()
        _lib.check(_lib.load().vqcpc_encoder_check(self._handle))

    # ------------------------------------------------------------------ reference surface
    def _encode_native(self, mel: Tensor, want_c: bool, conv_mode: int = 0, want_pre: bool = False):
        _lib.require_cuda(mel, "mel")
        if mel.dim() != 3 or mel.size(1) != self.conf.in_channels:
            raise RuntimeError(f"expected mel of shape (B, {self.conf.in_channels}, T), got {tuple(mel.shape)}")
        if mel.size(2) < 2:
            raise RuntimeError("Conv1d(k=4, s=2, p=1) needs at least 2 mel frames")
        _lib.require_same_device(mel, self.conv.weight, "mel")
        if mel.dtype != torch.float32 or not mel.is_contiguous() or mel.requires_grad:
            mel = mel.detach().to(torch.float32).contiguous()
        B, _, T = mel.shape
        To = (T - 2) // 2 + 1                        # nn.Conv1d(k4, s2, p1) output length (model.py:43)
        h = self._native()
        dev = mel.device
        last = self.encoder._modules["14"]
        hooks = last._forward_hooks
        z = torch.empty(B, To, self.conf.z_dim, device=dev)
        z_pre = torch.empty_like(z) if (want_pre or hooks) else None       # pre-VQ rows only when somebody reads them
        idx = torch.empty(B, To, dtype=torch.int64, device=dev)
        c = torch.empty(B, To, self.conf.c_dim, device=dev) if want_c else None
        with _lib.device_guard(dev):
            _lib.check(_lib.load().vqcpc_encoder_encode(
                h, mel.data_ptr(), B, T, conv_mode, z.data_ptr(), c.data_ptr() if want_c else None,
                idx.data_ptr(), z_pre.data_ptr() if z_pre is not None else None, _lib.current_stream()))
        for hook in list(hooks.values()):                   # encode.py:34-40 captures the pre-VQ activations
            hook(last, (None,), z_pre)
        return z, c, idx, z_pre

    @torch.no_grad()
    def encode(self, mel: Tensor, conv_mode: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
        """``model.py:59-70``: (z, c, indices).  ``conv_mode``: see ``vqcpc.h`` (0 = as the reference)."""
        z, c, idx, _ = self._encode_native(mel, want_c=True, conv_mode=conv_mode)
        return z, c, idx

    @torch.no_grad()
    def encode_indices(self, mel: Tensor, conv_mode: int = 0) -> Tensor:
        """What ``convert.py:76`` keeps of ``encode``: the code indices (LSTM skipped)."""
        return self._encode_native(mel, want_c=False, conv_mode=conv_mode)[2]

    @torch.no_grad()
    def stage(self, mel: Tensor, stage: int, conv_mode: int = 0) -> Tensor:
        """Activations after one front-end stage (``vqcpc_encoder_stage``), rows (B, T/2, F)."""
        _lib.require_cuda(mel, "mel")
        _lib.require_same_device(mel, self.conv.weight, "mel")
        mel = mel.detach().to(torch.float32).contiguous()
        B, _, T = mel.shape
        F = self.conf.z_dim if stage == 10 else self.conf.channels
        out = torch.empty(B, (T - 2) // 2 + 1, F, device=mel.device)
        with _lib.device_guard(mel.device):
            _lib.check(_lib.load().vqcpc_encoder_stage(self._native(), mel.data_ptr(), B, T, conv_mode, stage,
                                                       out.data_ptr(), _lib.current_stream()))
        return out

    def _adapt_rows(self, xf: Tensor, z_st: Optional[Tensor] = None, idx: Optional[Tensor] = None, handle=None) -> Tensor:
        """One codebook update (``vqcpc_encoder_vq_adapt``) over the rows xf (N, z_dim) fp32, contiguous, on the module's device
        -> a 2-element device tensor (loss, perplexity) from the codebook as it was (and, into ``z_st`` (N, z_dim) / ``idx`` (N) int64
        if given, the straight-through rows and the code indices of that codebook).  The three buffers are written through
        their ``data_ptr()``: their ``_version`` stays, so the handle -- which the call itself brings up to date -- is not rebuilt."""
        cb = self.codebook
        for name in ("embedding", "ema_count", "ema_weight"):
            t = getattr(cb, name)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != xf.device:
                raise RuntimeError(f"codebook.{name} must be a contiguous float32 tensor on {xf.device} "
                                   f"(got {t.dtype}, contiguous={t.is_contiguous()}, {t.device})")
        if xf.size(0) < 1:
            raise RuntimeError("codebook update: no rows")
        h = handle if handle is not None else self._native()
        stats = torch.empty(2, device=xf.device)
        with _lib.device_guard(xf.device):
            _lib.check(_lib.load().vqcpc_encoder_vq_adapt(
                h, xf.data_ptr(), xf.size(0), float(cb.decay), float(cb.epsilon), cb.embedding.data_ptr(),
                cb.ema_count.data_ptr(), cb.ema_weight.data_ptr(), z_st.data_ptr() if z_st is not None else None,
                idx.data_ptr() if idx is not None else None,
                stats[0:].data_ptr(), stats[1:].data_ptr(), _lib.current_stream()))
        return stats

    @torch.no_grad()
    def adapt_codebook(self, mels: Tensor, n_frames: Optional[List[int]] = None, conv_mode: int = 0,
                       return_indices: bool = False):
        """Fit the codebook to a batch: the front end up to ``z_pre`` (stage 10), then the EMA update of ``model.py:136-145``
        over the valid rows -- what one training step of the reference does to the codebook, without the gradient step on the
        other weights.  mels (B, in_channels, T); ``n_frames``: valid OUTPUT frames per utterance (a host list, each in
        [0, T // 2]; default all), rows behind them are padding and take no part.  Returns ``(loss, perplexity)`` of the batch
        under the codebook as it was, 0-dim device tensors; nothing is synchronised.  Works in either mode.  ``conv_mode``: as
        ``encode``.  ``return_indices``: also return the code every valid row was assigned to under that codebook, (N,) int64 on
        the device, utterance after utterance."""
        z_pre = self.stage(mels, 10, conv_mode)
        B, To, D = z_pre.shape
        if n_frames is None:
            rows = z_pre.view(-1, D)
        else:
            n = [int(v) for v in n_frames]
            if len(n) != B or any(v < 0 or v > To for v in n):
                raise RuntimeError(f"n_frames must hold one count in [0, {To}] per utterance ({B}), got {n}")
            rows = z_pre.view(-1, D) if all(v == To for v in n) else torch.cat([z_pre[b, :v] for b, v in enumerate(n)])
        rows = rows.contiguous()
        idx = torch.empty(rows.size(0), dtype=torch.int64, device=rows.device) if return_indices else None
        stats = self._adapt_rows(rows, idx=idx)
        return (stats[0], stats[1], idx) if return_indices else (stats[0], stats[1])

    # ------------------------------------------------------------------ the context LSTM and its gradient
    _RNN_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

    def _rnn_weights(self, dev):
        ws = [getattr(self.rnn, n) for n in self._RNN_NAMES]
        for n, t in zip(self._RNN_NAMES, ws):
            if t.dtype != torch.float32 or t.device != dev:
                raise RuntimeError(f"rnn.{n} must be a float32 tensor on {dev} (got {t.dtype}, {t.device})")
        return ws

    def _context_fwd(self, z: Tensor, weights=None):
        """One ``vqcpc_encoder_context_fwd`` call on contiguous fp32 device tensors -> (c, saved).  ``weights``: the four LSTM
        tensors (contiguous), or None = the handle's copies."""
        import ctypes
        B, T, _ = z.shape
        dev = z.device
        h = self._sizes_handle(dev) if weights is not None else self._native()
        lib = _lib.load()
        n = ctypes.c_uint64()
        _lib.check(lib.vqcpc_encoder_context_saved_bytes(h, B, T, ctypes.byref(n)))
        c = torch.empty(B, T, self.conf.c_dim, device=dev)
        saved = torch.empty(int(n.value) // 4, device=dev)
        wp = [w.data_ptr() for w in weights] if weights is not None else [None] * 4
        with _lib.device_guard(dev):
            _lib.check(lib.vqcpc_encoder_context_fwd(h, z.data_ptr(), B, T, *wp, c.data_ptr(), saved.data_ptr(), _lib.current_stream()))
        return c, saved

    def _context_bwd(self, z: Tensor, c: Tensor, saved: Tensor, grad_c: Tensor, weights=None, want=(True, True, True, True)):
        """One ``vqcpc_encoder_context_bwd`` call.  want = (z, w_ih, w_hh, bias) booleans -> the four gradients or None."""
        B, T, _ = z.shape
        dev = z.device
        h = self._sizes_handle(dev) if weights is not None else self._native()
        H, D = self.conf.c_dim, self.conf.z_dim
        shapes = ((B, T, D), (4 * H, D), (4 * H, H), (4 * H,))
        grads = [torch.empty(sh, device=dev) if w else None for sh, w in zip(shapes, want)]
        ptr = lambda t: t.data_ptr() if t is not None else None
        wp = [weights[0].data_ptr(), weights[1].data_ptr()] if weights is not None else [None, None]
        with _lib.device_guard(dev):
            _lib.check(_lib.load().vqcpc_encoder_context_bwd(h, z.data_ptr(), B, T, *wp, c.data_ptr(), saved.data_ptr(),
                                                             grad_c.data_ptr(), *[ptr(g) for g in grads], _lib.current_stream()))
        return grads

    def context(self, z: Tensor, *, differentiable: bool = False) -> Tensor:
        """``self.rnn(z)[0]`` (``model.py:69`` / ``:85``): z (B, T, z_dim) on the module's device -> c (B, T, c_dim).

        differentiable=False (the default): ``vqcpc_encoder_context``, detached.  differentiable=True, grad mode on and ``z`` or any
        ``rnn`` parameter requiring grad: ``c`` carries a ``grad_fn``.  Its forward is ``vqcpc_encoder_context_fwd`` on the
        parameters as they are (an optimizer step costs no new handle) and keeps the gates and cell states; its backward is one
        ``vqcpc_encoder_context_bwd`` call (``csrc/context_grad.hip``: back-propagation through time, one launch per step, every
        sum in a fixed order) asking only for the gradients that are needed; ``bias_ih_l0`` and ``bias_hh_l0`` receive the same
        values.  The value has the bits of the default call.  Under ``torch.no_grad()`` the flag changes nothing."""
        _lib.require_cuda(z, "z")
        _lib.require_same_device(z, self.rnn.weight_ih_l0, "z")
        if z.dim() != 3 or z.size(2) != self.conf.z_dim or z.size(0) < 1 or z.size(1) < 1:
            raise RuntimeError(f"expected z of shape (B, T, {self.conf.z_dim}), got {tuple(z.shape)}")
        if differentiable and torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for p in self.rnn.parameters())):
            ws = self._rnn_weights(z.device)
            return _ContextGrad.apply(self, z.to(torch.float32), *ws)
        zf = z.detach().to(torch.float32).contiguous()
        B, T, _ = zf.shape
        c = torch.empty(B, T, self.conf.c_dim, device=zf.device)
        with _lib.device_guard(zf.device):
            _lib.check(_lib.load().vqcpc_encoder_context(self._native(), zf.data_ptr(), B, T, c.data_ptr(), _lib.current_stream()))
        return c

    # ------------------------------------------------------------------ the front end, the VQ step and their gradients
    _FRONT_NAMES = (["conv.weight"] + [f"encoder.{n}.weight" for n in (0, 3, 6, 9, 12)] + [f"encoder.{n}.bias" for n in (0, 3, 6, 9, 12)] +
                    [f"encoder.{n}.weight" for n in (2, 5, 8, 11)] + ["encoder.14.weight", "encoder.14.bias"])

    def _front_params(self, dev):
        """The front end's 17 parameters in the member order of ``vqcpc_encoder_front_weights``."""
        sub = lambda name: self.get_parameter(name)
        ws = [sub(n) for n in self._FRONT_NAMES]
        for n, t in zip(self._FRONT_NAMES, ws):
            if t.dtype != torch.float32 or t.device != dev:
                raise RuntimeError(f"{n} must be a float32 tensor on {dev} (got {t.dtype}, {t.device})")
        return ws

    @staticmethod
    def _front_struct(tensors):
        """17 tensors (or None) in ``_FRONT_NAMES`` order -> ``_lib.EncoderFrontTensors``."""
        return _lib.fill_front(_lib.EncoderFrontTensors(), [t.data_ptr() if t is not None else None for t in tensors])

    def _check_mels(self, mels: Tensor) -> Tensor:
        _lib.require_cuda(mels, "mel")
        if mels.dim() != 3 or mels.size(1) != self.conf.in_channels:
            raise RuntimeError(f"expected mel of shape (B, {self.conf.in_channels}, T), got {tuple(mels.shape)}")
        if mels.size(0) < 1 or mels.size(2) < 2:
            raise RuntimeError("Conv1d(k=4, s=2, p=1) needs at least one utterance of at least 2 mel frames")
        _lib.require_same_device(mels, self.conv.weight, "mel")
        return mels.detach().to(torch.float32).contiguous()

    def _front_fwd(self, mel: Tensor, weights=None, conv_mode: int = 0):
        """One ``vqcpc_encoder_front_fwd`` call on a contiguous fp32 device mel -> (z_pre, saved).  ``weights``: the 17 front-end
        tensors (contiguous, ``_FRONT_NAMES`` order), or None = the handle's copies."""
        import ctypes
        B, _, T = mel.shape
        dev = mel.device
        h = self._sizes_handle(dev) if weights is not None else self._native()
        lib = _lib.load()
        n = ctypes.c_uint64()
        _lib.check(lib.vqcpc_encoder_front_saved_bytes(h, B, T, ctypes.byref(n)))
        z_pre = torch.empty(B, (T - 2) // 2 + 1, self.conf.z_dim, device=dev)
        saved = torch.empty(int(n.value) // 4, device=dev)
        w = ctypes.byref(self._front_struct(weights)) if weights is not None else None
        with _lib.device_guard(dev):
            _lib.check(lib.vqcpc_encoder_front_fwd(h, mel.data_ptr(), B, T, conv_mode, w, z_pre.data_ptr(), saved.data_ptr(),
                                                   _lib.current_stream()))
        return z_pre, saved

    def _front_bwd(self, mel: Tensor, saved: Tensor, grad_z_pre: Tensor, weights=None, want=(True,) * 17, conv_mode: int = 0):
        """One ``vqcpc_encoder_front_bwd`` call.  want: 17 booleans in ``_FRONT_NAMES`` order -> the 17 gradients or None."""
        import ctypes
        B, _, T = mel.shape
        dev = mel.device
        h = self._sizes_handle(dev) if weights is not None else self._native()
        shapes = [self.get_parameter(n).shape for n in self._FRONT_NAMES]
        grads = [torch.empty(sh, device=dev) if w else None for sh, w in zip(shapes, want)]
        w = ctypes.byref(self._front_struct(weights)) if weights is not None else None
        with _lib.device_guard(dev):
            _lib.check(_lib.load().vqcpc_encoder_front_bwd(h, mel.data_ptr(), B, T, conv_mode, w, saved.data_ptr(), grad_z_pre.data_ptr(),
                                                           ctypes.byref(self._front_struct(grads)), _lib.current_stream()))
        return grads

    def front_end(self, mels: Tensor, *, differentiable: bool = False, conv_mode: int = 0) -> Tensor:
        """``self.encoder(self.conv(mels).transpose(1, 2))`` (``model.py:65-67`` / ``:78-80``): mels (B, in_channels, T) ->
        z_pre (B, T // 2, z_dim), the rows before the VQ.

        differentiable=False (the default): ``stage(mels, 10)``, detached.  differentiable=True, grad mode on and a front-end
        parameter requiring grad: ``z_pre`` carries a ``grad_fn``.  Its forward is one ``vqcpc_encoder_front_fwd`` on the parameters
        as they are (an optimizer step costs no new handle) and keeps the rows the backward reads again; its backward is one
        ``vqcpc_encoder_front_bwd`` call (``csrc/front_grad.hip``: every sum in a fixed order) asking only for the gradients autograd
        needs.  The mel receives no gradient.  The value has the bits of the default call.  Under ``torch.no_grad()`` the flag
        changes nothing."""
        mel = self._check_mels(mels)
        if differentiable and torch.is_grad_enabled():
            ws = self._front_params(mel.device)
            if any(p.requires_grad for p in ws):
                return _FrontGrad.apply(self, mel, conv_mode, *ws)
        return self.stage(mel, 10, conv_mode)

    def _codebook_handle(self, dev):
        """The handle for a call that reads only the CODEBOOK from the handle's copies (``quantize``): a live handle on ``dev`` whose
        codebook is current serves, also one whose other copies an optimizer step has made stale -- a fit of the front end costs no
        new handle per step.  (``vqcpc_encoder_vq_adapt`` keeps the handle's codebook and the buffer in step.)"""
        h = self._live_handle(dev)
        e = self.codebook.embedding
        if h is not None and self._handle_key[2 + self._WEIGHT_NAMES.index("codebook.embedding")] == (e.data_ptr(), e._version):
            return h
        return self._native()

    def _quantize_rows(self, xf: Tensor, adapt: bool, want_q: bool):
        """The VQ step over rows xf (N, z_dim) fp32 contiguous -> (z_st, stats = [loss, perplexity], idx, q or None): the codebook
        as it is on entry decides all four; with ``adapt`` the EMA update follows (``vqcpc_encoder_vq_adapt``)."""
        h = self._codebook_handle(xf.device)
        q = idx = z_st = stats = None
        if want_q or not adapt:
            q, idx, z_st, stats = _vq_eval(h, xf, stats=not adapt)
        if adapt:
            z_st = torch.empty_like(xf)
            if idx is None:
                idx = torch.empty(xf.size(0), dtype=torch.int64, device=xf.device)
            stats = self._adapt_rows(xf, z_st, idx, handle=h)
        return z_st, stats, idx, q

    def quantize(self, z_pre: Tensor, *, differentiable: bool = False, adapt: bool = False):
        """``self.codebook(z_pre)`` (``model.py:117-155``): z_pre (B, T, z_dim) -> (z_st, vq_loss, perplexity, indices (B, T)),
        all four from the codebook as it is on entry.

        adapt=False: the eval branch (``vqcpc_encoder_vq_encode`` + ``vqcpc_encoder_forward_stats``).  adapt=True: the reference's
        training branch, ``vqcpc_encoder_vq_adapt`` -- the EMA update of ``model.py:136-145`` follows, in place.
        differentiable=True, grad mode on and ``z_pre`` requiring grad: ``z_st`` and ``vq_loss`` carry a ``grad_fn`` whose backward is
        one ``vqcpc_encoder_vq_bwd`` call, the straight-through estimator plus the commitment loss of ``model.py:147-150``; the
        values are those of the default call.  ``VQEmbeddingEMA.forward`` stays as it is."""
        _lib.require_cuda(z_pre, "z_pre")
        _lib.require_same_device(z_pre, self.codebook.embedding, "z_pre")
        D = self.conf.z_dim
        if z_pre.dim() != 3 or z_pre.size(2) != D or z_pre.numel() == 0:
            raise RuntimeError(f"expected z_pre of shape (B, T, {D}), got {tuple(z_pre.shape)}")
        if differentiable and torch.is_grad_enabled() and z_pre.requires_grad:
            return _VQGrad.apply(self, z_pre.to(torch.float32), bool(adapt))
        with torch.no_grad():
            z_st, stats, idx, _ = self._quantize_rows(z_pre.detach().to(torch.float32).reshape(-1, D).contiguous(), bool(adapt), False)
        return z_st.view_as(z_pre), stats[0], stats[1], idx.view(z_pre.shape[:2])

    def forward_differentiable(self, mels: Tensor, *, adapt_codebook: bool = True):
        """``model.py:72-86`` in training mode: (z, c, vq_loss, perplexity) with a ``grad_fn`` wherever a parameter requires grad --
        ``front_end``, ``quantize`` and ``context``, each ``differentiable=True``.  ``adapt_codebook``: run the EMA update as the
        reference's training branch does (the gradients are the same either way: they come from the codebook as it was).  Works in
        either mode; ``forward`` itself stays the inference path."""
        z_pre = self.front_end(mels, differentiable=True)
        z, vq_loss, perplexity, _ = self.quantize(z_pre, differentiable=True, adapt=adapt_codebook)
        c = self.context(z, differentiable=True)
        return z, c, vq_loss, perplexity

    def forward(self, mels: Tensor):
        """``model.py:72-86`` in eval mode: (z, c, vq_loss, perplexity)."""
        if self.training:
            raise NotImplementedError("vectorquantizedcpc_amd.Encoder implements the inference path; "
                                      "call .eval() (the EMA/straight-through training branch, model.py:136-145, is out of scope)")
        with torch.no_grad():
            zq, _, idx, z_pre = self._encode_native(mels, want_c=False, want_pre=True)
            B, Tz, D = zq.shape
            h = self._native()
            _, _, z_st, stats = _vq_eval(h, z_pre.view(-1, D), zq.view(-1, D), idx.view(-1))
            c = torch.empty(B, Tz, self.conf.c_dim, device=zq.device)
            with _lib.device_guard(zq.device):
                _lib.check(_lib.load().vqcpc_encoder_context(h, z_st.data_ptr(), B, Tz, c.data_ptr(), _lib.current_stream()))
        return z_st.view_as(zq), c, stats[0], stats[1]


@dataclass
class ConfCPC:
    """``model.py:158-165``."""
    n_prediction_steps: int = MISSING
    n_speakers_per_batch: int = MISSING
    n_utterances_per_speaker: int = MISSING
    n_negatives: int = MISSING
    z_dim: int = MISSING
    c_dim: int = MISSING


class CPCLoss(_lib.NativeModule):
    """``CPCLoss`` (``model.py:167-316``) on MI355X: the InfoNCE loss and per-step prediction accuracies in one fused HIP
    launch per batch, and -- on request -- its gradient.

    ``forward(z, c)`` is checkpoint SCORING: the value of the objective, detached.  ``forward(z, c, differentiable=True)`` under
    grad mode returns a loss that ``backward()`` can be called on: ``vqcpc_cpc_grad`` (``csrc/cpc_grad.hip``) computes the loss
    and the gradients with respect to ``z``, ``c`` and the first K predictors in one call, every sum in a fixed order, so equal
    inputs give equal bits.  That is what ``driver.fit_predictors`` refits the predictors with on a frozen encoder, and what
    ``driver.fit_context`` hands to ``Encoder.context(z, differentiable=True)`` to refit the context LSTM with them; in
    ``driver.fit_encoder`` ``dz`` goes on through ``Encoder.quantize`` and ``Encoder.front_end`` down to ``conv.weight``.  The
    optimizer is torch's by default; ``optim.Adam`` makes the update one ``vqcpc_adam_step`` call.

    All ``n_prediction_steps`` predictors are held (the reference's 24 ``state_dict()`` keys, so
    ``load_state_dict(checkpoint["cpc"])`` works unchanged); like the reference only the first half is ever used
    (``model.py:181``), and only that half ever receives a gradient.  The one deliberate difference is where the negatives
    come from: the reference draws them from torch's global CPU generator, this class from a counter-based protocol keyed by
    ``(seed, stream_id)`` (``synth.cpc_negatives``), or from the caller (``negatives=``) for draw-for-draw comparisons."""

    def __init__(self, conf: ConfCPC):
        super().__init__()
        self.conf = conf
        self.n_speakers_per_batch = conf.n_speakers_per_batch
        self.n_utterances_per_speaker = conf.n_utterances_per_speaker
        self.n_prediction_steps = conf.n_prediction_steps // 2
        self.n_negatives = conf.n_negatives
        self.z_dim = conf.z_dim
        self.c_dim = conf.c_dim
        self.predictors = nn.ModuleList([nn.Linear(conf.c_dim, conf.z_dim) for _ in range(conf.n_prediction_steps)])

    # ------------------------------------------------------------------ native handle (lifecycle: _lib.NativeModule;
    # refresh() is needed only after a write through ``.data``, the handle holds COPIES of the predictors)
    _NAME, _CREATE, _DESTROY = "CPCLoss", "vqcpc_cpc_create", "vqcpc_cpc_destroy"

    def _weight_names(self):
        if self.n_prediction_steps < 1:
            raise RuntimeError("CPCLoss: n_prediction_steps // 2 must be at least 1")
        return [f"predictors.{i}.{p}" for i in range(self.n_prediction_steps) for p in ("weight", "bias")]

    def _weights(self, p):
        w = _lib.CPCWeights()
        if self.n_prediction_steps > 16:
            raise RuntimeError(f"CPCLoss: at most 16 prediction steps are scored, got {self.n_prediction_steps}")
        for i in range(self.n_prediction_steps):
            w.weight[i], w.bias[i] = p(f"predictors.{i}.weight"), p(f"predictors.{i}.bias")
        w.n_steps, w.n_speakers, w.n_utterances = self.n_prediction_steps, self.n_speakers_per_batch, self.n_utterances_per_speaker
        w.n_negatives, w.z_dim, w.c_dim = self.n_negatives, self.z_dim, self.c_dim
        return w

    # ------------------------------------------------------------------ reference surface
    def _check_negatives(self, negatives, length: int, device):
        K, S, U, G = self.n_prediction_steps, self.n_speakers_per_batch, self.n_utterances_per_speaker, self.n_negatives
        utt, seq = negatives
        for name, t, shape, high in (("utt_index", utt, (K, U, G), U), ("seq_index", seq, (K, S, U, G, length), length)):
            if not isinstance(t, Tensor) or t.dtype != torch.int64 or tuple(t.shape) != shape:
                raise RuntimeError(f"expected negatives {name} as an int64 tensor of shape {shape}, got "
                                   f"{tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__}"
                                   f"{' ' + str(t.dtype) if isinstance(t, Tensor) else ''}")
            lo, hi = torch.aminmax(t)                         # a comparison entry, not a hot one: one reduction per array
            if int(lo) < 0 or int(hi) >= high:
                raise IndexError(f"negatives {name} holds values in [{int(lo)}, {int(hi)}], outside [0, {high})")
        return utt.to(device).contiguous(), seq.to(device).contiguous()

    def _check_inputs(self, z: Tensor, c: Tensor, negatives):
        """The checks every call starts with.  -> (T, L, device, utt_index, seq_index), the index arrays on the device or None."""
        _lib.require_cuda(z, "z")
        _lib.require_cuda(c, "c")
        K, N = self.n_prediction_steps, self.n_speakers_per_batch * self.n_utterances_per_speaker
        if z.dim() != 3 or c.dim() != 3 or z.size(0) != N or z.size(2) != self.z_dim or tuple(c.shape) != (N, z.size(1), self.c_dim):
            raise RuntimeError(f"expected z of shape ({N}, T, {self.z_dim}) and c of shape ({N}, T, {self.c_dim}) "
                               f"[{self.n_speakers_per_batch} speakers x {self.n_utterances_per_speaker} utterances], "
                               f"got {tuple(z.shape)} and {tuple(c.shape)}")
        T = z.size(1)
        if T < K + 2:
            raise RuntimeError(f"expected T >= {K + 2} frames ({K} prediction steps + 2 anchors, model.py:259), got T = {T}")
        _lib.require_same_device(z, self.predictors[0].weight, "z")
        _lib.require_same_device(c, self.predictors[0].weight, "c")
        dev, L = z.device, T - K
        utt = seq = None
        if negatives is not None:
            utt, seq = self._check_negatives(negatives, L, dev)
        return T, L, dev, utt, seq

    @torch.no_grad()
    def forward_detailed(self, z: Tensor, c: Tensor, negatives: Optional[Tuple[Tensor, Tensor]] = None, seed: int = 13,
                         stream_id: int = 0, want_correct: bool = False, want_scores: bool = False) -> dict:
        """``forward`` with everything the kernel computes, as device tensors: ``loss`` (0-dim), ``step_loss`` (K),
        ``accuracy`` (K); on request ``correct`` (K, N, L) uint8 and ``scores`` (K, N, 1 + Neg, L) = ``f`` of
        ``model.py:291``.  K = n_prediction_steps // 2, L = T - K.  Nothing is synchronised."""
        K, N = self.n_prediction_steps, self.n_speakers_per_batch * self.n_utterances_per_speaker
        T, L, dev, utt, seq = self._check_inputs(z, c, negatives)
        z = z.detach().to(torch.float32).contiguous()
        c = c.detach().to(torch.float32).contiguous()
        h = self._native()
        out = torch.empty(1 + 2 * K, device=dev)
        correct = torch.empty(K, N, L, dtype=torch.uint8, device=dev) if want_correct else None
        scores = torch.empty(K, N, 1 + self.n_negatives, L, device=dev) if want_scores else None
        with _lib.device_guard(dev):
            _lib.check(_lib.load().vqcpc_cpc_score(
                h, z.data_ptr(), c.data_ptr(), T, utt.data_ptr() if utt is not None else None,
                seq.data_ptr() if seq is not None else None, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF,
                out[0:].data_ptr(), out[1:].data_ptr(), out[1 + K:].data_ptr(),
                correct.data_ptr() if correct is not None else None, scores.data_ptr() if scores is not None else None,
                _lib.current_stream()))
        return {"loss": out[0], "step_loss": out[1:1 + K], "accuracy": out[1 + K:], "correct": correct, "scores": scores}

    def _grad_call(self, z, c, W, b, utt, seq, seed, stream_id, want):
        """One ``vqcpc_cpc_grad`` call on contiguous fp32 device tensors.  want = (z, c, W, b) booleans.
        -> (out = [loss, step_loss (K), accuracy (K)], the four gradients or None)."""
        K, dev = self.n_prediction_steps, z.device
        h = self._sizes_handle(dev)
        out = torch.empty(1 + 2 * K, device=dev)
        grads = [torch.empty_like(t) if w else None for t, w in zip((z, c, W, b), want)]
        ptr = lambda t: t.data_ptr() if t is not None else None
        with _lib.device_guard(dev):
            _lib.check(_lib.load().vqcpc_cpc_grad(
                h, z.data_ptr(), c.data_ptr(), z.size(1), W.data_ptr(), b.data_ptr(), ptr(utt), ptr(seq),
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF, out[0:].data_ptr(), out[1:].data_ptr(),
                out[1 + K:].data_ptr(), *[ptr(g) for g in grads], _lib.current_stream()))
        return out, grads

    @torch.no_grad()
    def gradients(self, z: Tensor, c: Tensor, negatives: Optional[Tuple[Tensor, Tensor]] = None, seed: int = 13, stream_id: int = 0,
                  wrt: Tuple[str, ...] = ("z", "c", "W", "b")) -> dict:
        """The ``vqcpc_cpc_grad`` call without autograd, as device tensors: ``loss`` (0-dim), ``step_loss`` (K), ``accuracy`` (K)
        and, for every name in ``wrt``, the gradient of ``loss`` -- ``z`` (N, T, 64), ``c`` (N, T, c_dim), ``W`` (K, 64, c_dim) and
        ``b`` (K, 64), the first K predictors stacked; a name not asked for maps to None.  Nothing is synchronised."""
        K = self.n_prediction_steps
        _, _, _, utt, seq = self._check_inputs(z, c, negatives)
        W = torch.stack([m.weight for m in self.predictors[:K]]).to(torch.float32)
        b = torch.stack([m.bias for m in self.predictors[:K]]).to(torch.float32)
        out, grads = self._grad_call(z.detach().to(torch.float32).contiguous(), c.detach().to(torch.float32).contiguous(), W, b, utt, seq,
                                     seed, stream_id, tuple(k in wrt for k in ("z", "c", "W", "b")))
        return dict(zip(("z", "c", "W", "b"), grads), loss=out[0], step_loss=out[1:1 + K], accuracy=out[1 + K:])

    def forward(self, z: Tensor, c: Tensor, negatives: Optional[Tuple[Tensor, Tensor]] = None, seed: int = 13,
                stream_id: int = 0, *, differentiable: bool = False) -> Tuple[Tensor, List[float]]:
        """``model.py:191-316``: ``(loss, accuracies)`` -- a 0-dim tensor on ``z``'s device and a list of K floats (reading
        them costs one synchronisation, as ``.item()`` does in the reference, ``model.py:312``).
        z (Spk * Utt, T, z_dim), c (Spk * Utt, T, c_dim), utterances speaker-major.

        differentiable=False (the default): scoring under ``no_grad``; the result is detached.  differentiable=True, grad mode on
        and any of ``z``, ``c`` or the first K predictors requiring grad: the loss carries a ``grad_fn``; one ``vqcpc_cpc_grad``
        call computes it together with the gradients that ``backward()`` will hand out (only those that are needed), and its
        bits are those of the default call.  Predictors K .. 2K - 1 are not used and get no gradient.  Under ``torch.no_grad()``
        the flag changes nothing.

        negatives: None = drawn in the kernel from ``(seed, stream_id)`` (``synth.cpc_negatives`` returns the same
        arrays), or ``(utt_index (K, Utt, Neg), seq_index (K, Spk, Utt, Neg, L))`` int64 = the index arrays of
        ``model.py:282`` for each step, e.g. what the reference drew."""
        K = self.n_prediction_steps
        if differentiable and torch.is_grad_enabled() and (
                z.requires_grad or c.requires_grad or any(p.requires_grad for m in self.predictors[:K] for p in m.parameters())):
            _, _, _, utt, seq = self._check_inputs(z, c, negatives)
            W = torch.stack([m.weight for m in self.predictors[:K]])          # glue: autograd hands each predictor its slice
            b = torch.stack([m.bias for m in self.predictors[:K]])
            if W.dtype != torch.float32:
                raise RuntimeError("CPCLoss: parameters must be float32")
            loss, acc = _CPCGrad.apply(self, z.to(torch.float32), c.to(torch.float32), W, b, utt, seq, seed, stream_id)
            return loss, acc.tolist()
        r = self.forward_detailed(z, c, negatives=negatives, seed=seed, stream_id=stream_id)
        return r["loss"], r["accuracy"].tolist()


class _ContextGrad(torch.autograd.Function):
    """``Encoder.context(z, differentiable=True)``: ``forward`` is ``vqcpc_encoder_context_fwd`` and keeps ``saved``; ``backward``
    is one ``vqcpc_encoder_context_bwd`` call asking for the gradients ``needs_input_grad`` names."""

    @staticmethod
    def forward(ctx, module, z, w_ih, w_hh, b_ih, b_hh):
        z = z.detach().contiguous()
        ws = [w.detach().contiguous() for w in (w_ih, w_hh, b_ih, b_hh)]
        c, saved = module._context_fwd(z, ws)
        ctx.module, ctx.kept = module, (z, saved)
        ctx.save_for_backward(w_ih, w_hh, c)             # torch refuses the backward if an in-place step has moved them since
        ctx.want = (ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3],
                    ctx.needs_input_grad[4] or ctx.needs_input_grad[5])
        return c

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_c):
        (z, saved), (w_ih, w_hh, c) = ctx.kept, ctx.saved_tensors
        gz, gi, gh, gb = ctx.module._context_bwd(z, c, saved, grad_c.to(torch.float32).contiguous(),
                                                 (w_ih.detach().contiguous(), w_hh.detach().contiguous()), ctx.want)
        need = ctx.needs_input_grad
        return None, gz, gi, gh, gb if need[4] else None, gb if need[5] else None


class _FrontGrad(torch.autograd.Function):
    """``Encoder.front_end(mels, differentiable=True)``: ``forward`` is ``vqcpc_encoder_front_fwd`` and keeps ``saved``;
    ``backward`` is one ``vqcpc_encoder_front_bwd`` call asking for the gradients ``needs_input_grad`` names."""

    @staticmethod
    def forward(ctx, module, mel, conv_mode, *ws):
        z_pre, saved = module._front_fwd(mel, [w.detach().contiguous() for w in ws], conv_mode)
        ctx.module, ctx.kept, ctx.conv_mode = module, (mel, saved), conv_mode
        ctx.save_for_backward(*ws)                       # torch refuses the backward if an in-place step has moved them since
        return z_pre

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_z_pre):
        mel, saved = ctx.kept
        grads = ctx.module._front_bwd(mel, saved, grad_z_pre.to(torch.float32).contiguous(),
                                      [w.detach().contiguous() for w in ctx.saved_tensors], ctx.needs_input_grad[3:], ctx.conv_mode)
        return (None, None, None) + tuple(grads)


class _VQGrad(torch.autograd.Function):
    """``Encoder.quantize(z_pre, differentiable=True)``: ``forward`` is the VQ step and keeps the rows and their codes' rows;
    ``backward`` is one ``vqcpc_encoder_vq_bwd`` call; a term whose upstream gradient is absent is dropped."""

    @staticmethod
    def forward(ctx, module, z_pre, adapt):
        xf = z_pre.detach().reshape(-1, z_pre.size(2)).contiguous()
        z_st, stats, idx, q = module._quantize_rows(xf, adapt, True)
        ctx.module, ctx.kept, ctx.shape = module, (xf, q), z_pre.shape
        ctx.set_materialize_grads(False)
        loss, ppl, idx = stats[0], stats[1], idx.view(z_pre.shape[:2])
        ctx.mark_non_differentiable(ppl, idx)
        return z_st.view_as(z_pre), loss, ppl, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_z_st, grad_loss, _grad_ppl, _grad_idx):
        if grad_z_st is None and grad_loss is None:
            return None, None, None
        xf, q = ctx.kept
        gs = grad_z_st.to(torch.float32).contiguous() if grad_z_st is not None else None
        gl = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None
        out = torch.empty_like(xf)
        ptr = lambda t: t.data_ptr() if t is not None else None
        with _lib.device_guard(xf.device):
            _lib.check(_lib.load().vqcpc_encoder_vq_bwd(ctx.module._sizes_handle(xf.device), xf.data_ptr(), q.data_ptr(), xf.size(0),
                                                        ptr(gs), ptr(gl), out.data_ptr(), _lib.current_stream()))
        return None, out.view(ctx.shape), None


class _CPCGrad(torch.autograd.Function):
    """``CPCLoss.forward(..., differentiable=True)``: ``forward`` makes the single ``vqcpc_cpc_grad`` call, asking for the
    gradients ``needs_input_grad`` names, and keeps them; ``backward`` multiplies them by the upstream gradient."""

    @staticmethod
    def forward(ctx, module, z, c, W, b, utt, seq, seed, stream_id):
        want = ctx.needs_input_grad[1:5]
        out, grads = module._grad_call(z.detach().contiguous(), c.detach().contiguous(), W.detach().contiguous(),
                                       b.detach().contiguous(), utt, seq, seed, stream_id, want)
        ctx.kept = grads
        K = module.n_prediction_steps
        loss, acc = out[0], out[1 + K:]
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_acc):
        return (None,) + tuple(g * grad_loss if g is not None else None for g in ctx.kept) + (None, None, None, None)
