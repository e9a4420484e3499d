"""Drop-in ``Vocoder`` for the reference's ``network_vocoder.py`` (inference path).

``Vocoder(conf: ConfVocoder)``, ``generate(z, speaker)`` and ``forward(x, z, speaker)`` keep
the reference signatures (``network_vocoder.py:31``, ``:41``, ``:69``).  The RNN_MS core the
reference imports from the third-party ``rnnms`` package (``network_vocoder.py:8``) is not
available offline; ``RNNMSVocoder`` below is this project's statement of it (shapes from
``config.py:67-77``) -- parity with ``rnnms`` itself is unpinned.  Sub-modules only
hold parameters; all arithmetic runs in ``libvqcpc_hip.so``.
"""
import ctypes as C
import numbers
from dataclasses import dataclass, field

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib

MISSING = "???"


@dataclass
class ConfPreNet:
    num_layers: int = 2           # config.py:72
    bidirectional: bool = True    # config.py:73


@dataclass
class ConfWaveAR:
    size_i_embed_ar: int = 256    # config.py:75
    size_h_rnn: int = 896         # config.py:76
    size_h_fc: int = 256          # config.py:77


@dataclass
class ConfRNNMSVocoder:
    """``config.py:67-77`` (+ ``dim_i_feature`` set at ``config.py:198-199``)."""
    dim_i_feature: int = 128
    dim_voc_latent: int = 256
    bits_mu_law: int = 8
    upsampling_t: int = 160
    prenet: ConfPreNet = field(default_factory=ConfPreNet)
    wave_ar: ConfWaveAR = field(default_factory=ConfWaveAR)


@dataclass
class ConfVocoder:
    """``network_vocoder.py:11-24``; defaults from ``config.py:62-66``."""
    size_i_codebook: int = 512
    dim_i_embedding: int = 64
    n_speakers: int = 102
    dim_speaker_embedding: int = 64
    rnnms: ConfRNNMSVocoder = field(default_factory=ConfRNNMSVocoder)


class _WaveAR(nn.Module):
    def __init__(self, size_i_cnd, conf: ConfWaveAR, size_o):
        super().__init__()
        self.embedding = nn.Embedding(size_o, conf.size_i_embed_ar)
        self.rnn = nn.GRU(conf.size_i_embed_ar + size_i_cnd, conf.size_h_rnn, batch_first=True)
        self.fc1 = nn.Linear(conf.size_h_rnn, conf.size_h_fc)
        self.fc2 = nn.Linear(conf.size_h_fc, size_o)


class RNNMSVocoder(nn.Module):
    """Parameter container of the RNN_MS core: bi-GRU PreNet + embedding-AR GRU + 2 FC."""

    def __init__(self, conf: ConfRNNMSVocoder):
        super().__init__()
        if conf.prenet.num_layers != 2 or not conf.prenet.bidirectional:
            raise ValueError("RNNMSVocoder: the MI355X path implements the 2-layer bidirectional PreNet of config.py:71-73")
        self.conf = conf
        self.prenet = nn.GRU(conf.dim_i_feature, conf.dim_voc_latent // 2, num_layers=2, batch_first=True,
                             bidirectional=True)
        self.ar = _WaveAR(conf.dim_voc_latent, conf.wave_ar, 2 ** conf.bits_mu_law)


class Vocoder(_lib.NativeModule):
    """bidirectional_PreNet + WaveRNN (=RNN_MS) conditioned on VQ-CPC codes (``network_vocoder.py:26-78``)."""

    def __init__(self, conf: ConfVocoder):
        super().__init__()
        self.conf = conf
        self.code_embedding = nn.Embedding(conf.size_i_codebook, conf.dim_i_embedding)
        self.speaker_embedding = nn.Embedding(conf.n_speakers, conf.dim_speaker_embedding)
        if conf.rnnms.dim_i_feature != conf.dim_i_embedding + conf.dim_speaker_embedding:
            raise ValueError("rnnms.dim_i_feature must equal dim_i_embedding + dim_speaker_embedding (config.py:198-199)")
        self.rnnms = RNNMSVocoder(conf.rnnms)
        self._utterances_done = 0

    # ------------------------------------------------------------------ native handle (lifecycle: _lib.NativeModule)
    _NAME, _CREATE, _DESTROY, _SET_OPTION = "Vocoder", "vqcpc_vocoder_create", "vqcpc_vocoder_destroy", "vqcpc_vocoder_set_option"
    _WEIGHT_NAMES = (["code_embedding.weight", "speaker_embedding.weight"] +                    # = list(state_dict())
                     [f"rnnms.prenet.{k}_l{layer}{suf}" for layer in range(2) for suf in ("", "_reverse")
                      for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] +
                     ["rnnms.ar.embedding.weight"] + [f"rnnms.ar.rnn.{k}_l0" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] +
                     [f"rnnms.ar.{fc}.{k}" for fc in ("fc1", "fc2") for k in ("weight", "bias")])

    # what the gradient entries read from the handle's copies although the nine tensors of rnnms.ar are the caller's
    _FROZEN_NAMES = frozenset(n for n in _WEIGHT_NAMES if not n.startswith("rnnms.ar."))

    def _weights(self, p):
        w = _lib.VocoderWeights()
        w.code_embedding, w.speaker_embedding = p("code_embedding.weight"), p("speaker_embedding.weight")
        for layer in range(2):
            for d, suf in enumerate(("", "_reverse")):
                w.prenet_w_ih[layer][d] = p(f"rnnms.prenet.weight_ih_l{layer}{suf}")
                w.prenet_w_hh[layer][d] = p(f"rnnms.prenet.weight_hh_l{layer}{suf}")
                w.prenet_b_ih[layer][d] = p(f"rnnms.prenet.bias_ih_l{layer}{suf}")
                w.prenet_b_hh[layer][d] = p(f"rnnms.prenet.bias_hh_l{layer}{suf}")
        w.ar_embedding = p("rnnms.ar.embedding.weight")
        w.ar_w_ih, w.ar_w_hh = p("rnnms.ar.rnn.weight_ih_l0"), p("rnnms.ar.rnn.weight_hh_l0")
        w.ar_b_ih, w.ar_b_hh = p("rnnms.ar.rnn.bias_ih_l0"), p("rnnms.ar.rnn.bias_hh_l0")
        w.fc1_weight, w.fc1_bias = p("rnnms.ar.fc1.weight"), p("rnnms.ar.fc1.bias")
        w.fc2_weight, w.fc2_bias = p("rnnms.ar.fc2.weight"), p("rnnms.ar.fc2.bias")
        c, r = self.conf, self.conf.rnnms
        w.n_codes, w.dz, w.n_speakers, w.ds = c.size_i_codebook, c.dim_i_embedding, c.n_speakers, c.dim_speaker_embedding
        w.Hp, w.de, w.Hr, w.Hf = r.dim_voc_latent // 2, r.wave_ar.size_i_embed_ar, r.wave_ar.size_h_rnn, r.wave_ar.size_h_fc
        w.n_cls, w.upsample_t, w.bits_mu_law = 2 ** r.bits_mu_law, r.upsampling_t, r.bits_mu_law
        return w

    def check(self):
        """Synchronise the current stream and raise if a call since the last check went wrong in a way only the device
        knows (``vqcpc_vocoder_check``): ``IndexError`` for a code index or speaker id outside its embedding table (what
        ``nn.Embedding`` raises at ``network_vocoder.py:73,75``), ``RuntimeError`` if an in-kernel hand-off timed out or the
        resident decoders' workgroups were not dealt 32 per XCD -- that call's waveform is incomplete (or was not written),
        and repeating the call gives the samples the fast path would have produced."""
        if self._handle is None:
            return
        torch.cuda.current_stream().synchronize()
        rc = _lib.load().vqcpc_vocoder_check(self._handle)
        if rc != 0:
            msg = _lib.load().vqcpc_last_error().decode()
            if "index out of range in self" in msg:
                raise IndexError("index out of range in self")
            raise RuntimeError(f"libvqcpc_hip: {msg} (status {rc})")

    def _check_rc(self, rc: int):
        """``_lib.check`` for a call that may follow another on the same handle without a synchronisation between them: the later
        call reports what the earlier one's kernels have already written to the status word, and a bad index is ``check()``'s
        ``IndexError`` there as well (the word is cleared by the report)."""
        if rc != 0 and "index out of range in self" in _lib.load().vqcpc_last_error().decode():
            raise IndexError("index out of range in self")
        _lib.check(rc)

    def last_timing(self):
        """(milliseconds, samples) of the last decode loop, from HIP events on its stream."""
        ms, n = C.c_float(), C.c_int()
        torch.cuda.current_stream().synchronize()
        _lib.check(_lib.load().vqcpc_vocoder_last_timing(self._native(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_path(self) -> int:
        """Decode loop of the last call (``vqcpc_vocoder_last_path``): 2 the per-XCD resident decoders (up to 68 utterances in
        flight), 3 their matrix-core form (69 .. 511), 0 the launch-per-step kernels -- which also take every call whose
        dimensions are not the reference's (size_h_rnn 896, size_h_fc 256, 8-bit mu-law: ``config.py:69,76-77``), at about
        half the speed; 1 = nothing has run yet."""
        return int(_lib.load().vqcpc_vocoder_last_path(self._native()))

    def last_slots(self) -> int:
        """Decode slots the last call's loop ran through (``vqcpc_vocoder_last_slots``)."""
        return int(_lib.load().vqcpc_vocoder_last_slots(self._native()))

    def workspace_bytes(self) -> int:
        """Device bytes of the native handle's grow-only work buffers (conditioning rows, schedules, exchange areas)."""
        n = C.c_uint64()
        _lib.check(_lib.load().vqcpc_vocoder_workspace_bytes(self._native(), C.byref(n)))
        return int(n.value)

    def kernel_times(self, reps: int = 1000):
        """(us GRU step, us fc1, us fc2 + draw, decode slots per launch, GRU kernel kind): ``vqcpc_vocoder_kernel_times``."""
        out = (C.c_float * 5)()
        _lib.check(_lib.load().vqcpc_vocoder_kernel_times(self._native(), int(reps), out, _lib.current_stream()))
        return tuple(float(v) for v in out)

    # ------------------------------------------------------------------ reference surface
    def _prep(self, z: Tensor, speaker: Tensor):
        _lib.require_cuda(z, "z")
        _lib.require_same_device(z, self.code_embedding.weight, "z")
        if z.dim() != 2 or speaker.dim() != 1 or speaker.size(0) != z.size(0):
            raise RuntimeError(f"expected z (B, T') and speaker (B), got {tuple(z.shape)} and {tuple(speaker.shape)}")
        if z.is_floating_point() or speaker.is_floating_point():
            raise RuntimeError("z and speaker must be integer tensors (nn.Embedding indices, network_vocoder.py:73,75)")
        z = z.detach().to(torch.int64).contiguous()
        speaker = speaker.detach().to(device=z.device, dtype=torch.int64).contiguous()
        # nn.Embedding raises on an out-of-range index (network_vocoder.py:73,75).  The glue kernel checks every index it reads
        # and reports through the handle's status word, which check() turns into the same IndexError: no reduce kernels and
        # no device synchronisation here (round 3 read min / max back on every call).
        return z, speaker

    def _sampling_args(self, B: int, seed, utt_base, utt_ids, n_codes):
        """``(n_codes, seed, utt_base, utt_ids)`` as ``vqcpc_vocoder_generate`` / ``_stream_open`` take them, from the keyword
        arguments of the sampling protocol: the default seed is torch's, the default stream ids are the next ``B`` of this
        module's count (``_utterances_done`` moves only when neither ``utt_base`` nor ``utt_ids`` is given)."""
        seed = (torch.initial_seed() if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        nc = _lib.int_array(n_codes, B, "n_codes")
        ids = _lib.int_array(None if utt_ids is None else [int(v) & 0xFFFFFFFF for v in utt_ids], B, "utt_ids", C.c_uint32)
        if utt_base is None:
            utt_base = self._utterances_done
            if utt_ids is None:
                self._utterances_done += B
        return nc, seed, int(utt_base) & 0xFFFFFFFF, ids

    @torch.no_grad()
    def generate(self, z: Tensor, speaker: Tensor, *, n_codes=None, seed=None, utt_base=None, utt_ids=None,
                 return_mulaw: bool = False, max_steps: int = 0, async_: bool = False):
        """``network_vocoder.py:69-78``: waveform (B, 2*upsampling_t*T') from code indices and speaker ids.

        Keyword extras (not in the reference): ``n_codes`` per-utterance valid code counts of a
        padded batch; ``seed`` / ``utt_base`` / ``utt_ids`` of the sampling protocol (default: torch's
        seed and the number of utterances this module has generated so far; ``utt_ids`` gives every
        row its own stream id, so results do not depend on batching); ``return_mulaw`` also returns
        the int64 mu-law classes.

        The reference's caller takes the result to the host right away (``convert.py:77-83``), so by default this call
        synchronises its stream once and checks the handle's status word (``check()``): an index outside its table raises
        ``IndexError`` like ``nn.Embedding``; if an in-kernel hand-off of the resident decoders gave up (a shared GPU), the
        call is repeated ONCE -- same sampling streams, so the same samples -- with a warning.  ``async_=True`` only enqueues
        the work (no synchronisation: pipelined callers); such callers call ``check()`` themselves before they use the
        waveform.
        """
        if not async_:
            kw = dict(n_codes=n_codes, seed=seed, utt_base=utt_base, utt_ids=utt_ids, return_mulaw=return_mulaw, max_steps=max_steps)
            if utt_base is None:
                kw["utt_base"] = self._utterances_done             # a repeat must draw from the same streams
            out = _lib.run_checked(lambda: self.generate(z, speaker, async_=True, **kw), self.check,
                                   "Vocoder.generate: decode repeated ({})")
            if utt_base is None and utt_ids is None:
                self._utterances_done += int(z.size(0))
            return out
        z, speaker = self._prep(z, speaker)
        B, Tc = z.shape
        h = self._native()
        L = 2 * self.conf.rnnms.upsampling_t * Tc
        wav = torch.empty(B, L, device=z.device)
        mulaw = torch.empty(B, L, dtype=torch.int64, device=z.device) if return_mulaw else None
        sampling = self._sampling_args(B, seed, utt_base, utt_ids, n_codes)
        with _lib.device_guard(z.device):
            _lib.check(_lib.load().vqcpc_vocoder_generate(
                h, z.data_ptr(), speaker.data_ptr(), B, Tc, *sampling, wav.data_ptr(),
                mulaw.data_ptr() if return_mulaw else None, int(max_steps), _lib.current_stream()))
        return (wav, mulaw) if return_mulaw else wav

    @torch.no_grad()
    def generate_stream(self, z: Tensor, speaker: Tensor, *, chunk_samples: int, n_codes=None, seed=None, utt_base=None,
                        utt_ids=None, return_mulaw: bool = False) -> "VocoderStream":
        """``generate`` chunk by chunk: an iterable of (B, n) device waveforms (or ``(wav, mulaw)`` pairs) of ``chunk_samples``
        samples each, the last one shorter; ``torch.cat(list(stream), 1)`` equals ``generate(...)`` with the same seed and ids.
        The prenet runs here, over all of ``z`` (it is bidirectional); every chunk then resumes the sample loop where the last
        one stopped.  Default ids take ``B`` utterances from this module's count, as ``generate`` does."""
        up = self.conf.rnnms.upsampling_t
        if isinstance(chunk_samples, bool) or not isinstance(chunk_samples, numbers.Integral) or chunk_samples <= 0 or chunk_samples % up:
            raise ValueError(f"chunk_samples must be a positive multiple of upsampling_t = {up} (got {chunk_samples!r})")
        z, speaker = self._prep(z, speaker)
        B, Tc = z.shape
        h = self._native()
        sampling = self._sampling_args(B, seed, utt_base, utt_ids, n_codes)
        st = C.c_void_p()
        with _lib.device_guard(z.device):
            _lib.check(_lib.load().vqcpc_vocoder_stream_open(
                h, z.data_ptr(), speaker.data_ptr(), B, Tc, *sampling, C.byref(st), _lib.current_stream()))
        return VocoderStream(self, h, st, B, int(chunk_samples), z.device, return_mulaw)

    @torch.no_grad()
    def forward(self, x: Tensor, z: Tensor, speaker: Tensor) -> Tensor:
        """``network_vocoder.py:41-67``: teacher-forced energies (B, T_s, 2**bits).  Synchronises its stream (``check()``)."""
        z, speaker = self._prep(z, speaker)
        x = x.detach().to(device=z.device, dtype=torch.int64).contiguous()
        B, Tc = z.shape
        if x.dim() != 2 or x.size(0) != B:
            raise RuntimeError(f"expected x (B, T_s), got {tuple(x.shape)}")
        Ts = x.size(1)
        if Ts > 2 * self.conf.rnnms.upsampling_t * Tc:
            raise RuntimeError("x is longer than the conditioning series covers")
        if x.min().item() < 0 or x.max().item() >= 2 ** self.conf.rnnms.bits_mu_law:
            raise IndexError("index out of range in self")
        logits = torch.empty(B, Ts, 2 ** self.conf.rnnms.bits_mu_law, device=z.device)
        with _lib.device_guard(z.device):
            _lib.check(_lib.load().vqcpc_vocoder_logits(self._native(), x.data_ptr(), z.data_ptr(), speaker.data_ptr(),
                                                        B, Tc, Ts, logits.data_ptr(), _lib.current_stream()))
            self.check()              # a bad z / speaker raises here, like nn.Embedding, and is not left latched for generate()
        return logits

    # ------------------------------------------------------------------ scoring and its gradients
    AR_KEYS = ("embedding", "w_ih", "w_hh", "b_ih", "b_hh", "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias")   # vqcpc_vocoder_ar_weights

    def _ar_params(self):
        """The nine parameters of ``rnnms.ar`` in the order of ``AR_KEYS``."""
        ar = self.rnnms.ar
        return [ar.embedding.weight, ar.rnn.weight_ih_l0, ar.rnn.weight_hh_l0, ar.rnn.bias_ih_l0, ar.rnn.bias_hh_l0,
                ar.fc1.weight, ar.fc1.bias, ar.fc2.weight, ar.fc2.bias]

    def _nll_call(self, audio: Tensor, z: Tensor, speaker: Tensor, lengths, n_codes):
        """What every scoring entry takes, checked: ``(audio, z, speaker, B, Tc, L, n_audio, n_codes)`` with the tensors int64,
        contiguous and on the module's device and the two per-utterance lists as ``c_int`` arrays (or None)."""
        z, speaker = self._prep(z, speaker)
        _lib.require_cuda(audio, "audio")
        _lib.require_same_device(audio, self.code_embedding.weight, "audio")
        B, Tc = z.shape
        if audio.dim() != 2 or audio.size(0) != B or audio.size(1) < 1:
            raise RuntimeError(f"expected audio (B, L) with B = {B} and L >= 1, got {tuple(audio.shape)}")
        if audio.is_floating_point() or audio.dtype == torch.bool:
            raise RuntimeError("audio must be an integer tensor of mu-law classes (the targets of F.cross_entropy, vocoder.py:63)")
        audio = audio.detach().to(torch.int64).contiguous()
        return (audio, z, speaker, B, Tc, audio.size(1), _lib.int_array(lengths, B, "lengths"), _lib.int_array(n_codes, B, "n_codes"))

    def _ar_struct(self, tensors):
        """``VocoderArTensors`` of nine tensors (None = NULL member), or None for ``tensors`` None."""
        if tensors is None:
            return None
        s = _lib.VocoderArTensors()
        for k, t in zip(self.AR_KEYS, tensors):
            setattr(s, k, None if t is None else t.data_ptr())
        return s

    def _ar_weights(self, weights, dev):
        """The nine tensors a gradient call reads: None (the handle's copies) or nine fp32 tensors on ``dev``, made contiguous."""
        if weights is None:
            return None
        ws = [w.detach().contiguous() for w in weights]
        for k, w, p in zip(self.AR_KEYS, ws, self._ar_params()):
            if w.dtype != torch.float32 or w.device != dev or w.shape != p.shape:
                raise RuntimeError(f"rnnms.ar {k} must be a float32 tensor of shape {tuple(p.shape)} on {dev} "
                                   f"(got {w.dtype}, {tuple(w.shape)}, {w.device})")
        return ws

    def _ar_handle(self, dev, weights, cond_in):
        """The handle of a gradient call on ``rnnms.ar``.  With the caller's nine tensors and the conditioning series given, nothing
        is read from the handle's copies: a live handle serves whatever has moved since it was built."""
        if weights is None:
            return self._native()
        return self._sizes_handle(dev, () if cond_in is not None else self._FROZEN_NAMES)

    def _ar_fwd(self, call, weights=None, want_cond: bool = False, cond_in=None):
        """One ``vqcpc_vocoder_ar_fwd`` call -> (nll_sum, n_scored, n_correct, cond or None, saved).  ``call``: ``_nll_call``'s
        tuple; ``weights``: ``_ar_weights``'s list; ``cond_in`` (B, 2T', dim_voc_latent): the conditioning series given
        (``vqcpc_vocoder_ar_fwd_cond``: the prenet does not run)."""
        audio, z, speaker, B, Tc, L, na, nc = call
        dev = z.device
        h = self._ar_handle(dev, weights, cond_in)
        lib = _lib.load()
        n = C.c_uint64()
        _lib.check(lib.vqcpc_vocoder_ar_saved_bytes(h, B, L, C.byref(n)))
        nll_sum = torch.empty(B, dtype=torch.float64, device=dev)
        n_scored = torch.empty(B, dtype=torch.int64, device=dev)
        n_correct = torch.empty(B, dtype=torch.int64, device=dev)
        cond = torch.empty(B, 2 * Tc, self.conf.rnnms.dim_voc_latent, device=dev) if want_cond else None
        saved = torch.empty(int(n.value) // 4, device=dev)
        head = (h, audio.data_ptr(), z.data_ptr(), speaker.data_ptr(), B, Tc, L, nc, na, self._ar_struct(weights))
        tail = (nll_sum.data_ptr(), n_scored.data_ptr(), n_correct.data_ptr(), cond.data_ptr() if want_cond else None, saved.data_ptr(),
                _lib.current_stream())
        with _lib.device_guard(dev):
            if cond_in is None:
                _lib.check(lib.vqcpc_vocoder_ar_fwd(*head, *tail))
            else:
                self._check_rc(lib.vqcpc_vocoder_ar_fwd_cond(*head, cond_in.data_ptr(), *tail))
        return nll_sum, n_scored, n_correct, cond, saved

    def _ar_bwd(self, call, saved, weights=None, grad_loss=None, want=(True,) * 9, cond_grad: bool = False, cond_in=None):
        """One ``vqcpc_vocoder_ar_bwd`` call -> (nine gradients or None in the order of ``AR_KEYS``, grad_cond or None).
        ``grad_loss``: fp32 device scalar or None = 1; ``cond_in``: that of the forward (``vqcpc_vocoder_ar_bwd_cond``)."""
        audio, z, speaker, B, Tc, L, na, nc = call
        dev = z.device
        h = self._ar_handle(dev, weights, cond_in)
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) if w else None for p, w in zip(self._ar_params(), want)]
        gc = torch.empty(B, 2 * Tc, self.conf.rnnms.dim_voc_latent, device=dev) if cond_grad else None
        head = (h, audio.data_ptr(), z.data_ptr(), speaker.data_ptr(), B, Tc, L, nc, na, self._ar_struct(weights))
        tail = (saved.data_ptr(), None if grad_loss is None else grad_loss.data_ptr(), self._ar_struct(grads),
                gc.data_ptr() if cond_grad else None, _lib.current_stream())
        with _lib.device_guard(dev):
            if cond_in is None:
                _lib.check(_lib.load().vqcpc_vocoder_ar_bwd(*head, *tail))
            else:
                self._check_rc(_lib.load().vqcpc_vocoder_ar_bwd_cond(*head, cond_in.data_ptr(), *tail))
        return grads, gc

    # ------------------------------------------------------------------ the conditioning path's gradients
    # vqcpc_vocoder_cond_weights, by state_dict() name: the two tables, then w_ih, w_hh, b_ih, b_hh, each [layer][direction]
    COND_KEYS = ("code_embedding.weight", "speaker_embedding.weight") + tuple(
        f"rnnms.prenet.{k}_l{layer}{suf}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for layer in range(2)
        for suf in ("", "_reverse"))
    AR_NAMES = tuple(n for n in _WEIGHT_NAMES if n.startswith("rnnms.ar."))      # the state_dict() names behind AR_KEYS, in its order
    TRAIN_PARTS = ("ar", "prenet", "embeddings")

    def _cond_params(self):
        """The eighteen parameters of the conditioning path in the order of ``COND_KEYS``."""
        return [self.get_parameter(n) for n in self.COND_KEYS]

    def _part_params(self, part: str):
        """The parameters of one of ``TRAIN_PARTS``."""
        if part == "ar":
            return self._ar_params()
        cond = self._cond_params()
        return cond[:2] if part == "embeddings" else cond[2:]

    @classmethod
    def _train_parts(cls, train, who: str):
        train = tuple(train)
        unknown = [t for t in train if t not in cls.TRAIN_PARTS]
        if unknown or not train or len(set(train)) != len(train):
            raise ValueError(f"{who}: train must name each of {cls.TRAIN_PARTS} at most once and at least one of them, got {train!r}")
        return train

    def _cond_struct(self, tensors):
        """``VocoderCondTensors`` of eighteen tensors in the order of ``COND_KEYS`` (None = NULL member), or None for None."""
        if tensors is None:
            return None
        s = _lib.VocoderCondTensors()
        p = [None if t is None else t.data_ptr() for t in tensors]
        s.code_embedding, s.speaker_embedding = p[0], p[1]
        for i, field in enumerate((s.prenet_w_ih, s.prenet_w_hh, s.prenet_b_ih, s.prenet_b_hh)):
            for layer in range(2):
                for d in range(2):
                    field[layer][d] = p[2 + 4 * i + 2 * layer + d]
        return s

    def _cond_weights(self, weights, dev):
        """The eighteen tensors a gradient call reads: None (the handle's copies) or fp32 tensors on ``dev``, made contiguous."""
        if weights is None:
            return None
        ws = [w.detach().contiguous() for w in weights]
        if len(ws) != len(self.COND_KEYS):
            raise RuntimeError(f"the conditioning path has {len(self.COND_KEYS)} tensors (Vocoder.COND_KEYS), got {len(ws)}")
        for k, w, p in zip(self.COND_KEYS, ws, self._cond_params()):
            if w.dtype != torch.float32 or w.device != dev or w.shape != p.shape:
                raise RuntimeError(f"{k} must be a float32 tensor of shape {tuple(p.shape)} on {dev} "
                                   f"(got {w.dtype}, {tuple(w.shape)}, {w.device})")
        return ws

    def _cond_fwd(self, z, speaker, nc, weights=None):
        """One ``vqcpc_vocoder_cond_fwd`` call -> (cond (B, 2T', dim_voc_latent), saved).  ``z``, ``speaker``: ``_prep``'s;
        ``nc``: ``c_int`` array or None; ``weights``: ``_cond_weights``'s list."""
        B, Tc = z.shape
        dev = z.device
        h = self._sizes_handle(dev) if weights is not None else self._native()
        lib = _lib.load()
        n = C.c_uint64()
        _lib.check(lib.vqcpc_vocoder_cond_saved_bytes(h, B, Tc, C.byref(n)))
        cond = torch.empty(B, 2 * Tc, self.conf.rnnms.dim_voc_latent, device=dev)
        saved = torch.empty(int(n.value) // 4, device=dev)
        with _lib.device_guard(dev):
            self._check_rc(lib.vqcpc_vocoder_cond_fwd(h, z.data_ptr(), speaker.data_ptr(), B, Tc, nc, self._cond_struct(weights), cond.data_ptr(),
                                                      saved.data_ptr(), _lib.current_stream()))
        return cond, saved

    def _cond_bwd(self, z, speaker, nc, saved, grad_cond, weights=None, want=(True,) * 18):
        """One ``vqcpc_vocoder_cond_bwd`` call -> eighteen gradients or None in the order of ``COND_KEYS``."""
        B, Tc = z.shape
        dev = z.device
        h = self._sizes_handle(dev) if weights is not None else self._native()
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) if w else None for p, w in zip(self._cond_params(), want)]
        with _lib.device_guard(dev):
            self._check_rc(_lib.load().vqcpc_vocoder_cond_bwd(h, z.data_ptr(), speaker.data_ptr(), B, Tc, nc, self._cond_struct(weights),
                                                              saved.data_ptr(), grad_cond.data_ptr(), self._cond_struct(grads),
                                                              _lib.current_stream()))
        return grads

    @torch.no_grad()
    def cond_gradients(self, z: Tensor, speaker: Tensor, grad_cond: Tensor, *, n_codes=None, want=COND_KEYS, weights=None) -> dict:
        """The gradients of ``sum(cond * grad_cond)`` -- ``cond`` the conditioning series (B, 2T', dim_voc_latent) of ``z`` and
        ``speaker``, summed over every utterance's own ``2 * n_codes[b]`` frames -- with respect to the tensors of the conditioning
        path that ``want`` names (``COND_KEYS``: the two embedding tables and the sixteen tensors of ``rnnms.prenet``, by
        ``state_dict()`` name): one ``vqcpc_vocoder_cond_fwd`` and one ``vqcpc_vocoder_cond_bwd`` call (``csrc/prenet_grad.hip``).
        -> dict of device tensors: the wanted names and ``cond``.  ``weights``: eighteen tensors in the order of ``COND_KEYS`` read
        in place of the native handle's copies (default: the parameters themselves, as they are now).  Synchronises its stream
        (``check()``): an index outside its table raises ``IndexError``."""
        unknown = [k for k in want if k not in self.COND_KEYS]
        if unknown:
            raise ValueError(f"cond_gradients: unknown tensors {unknown}; known: {self.COND_KEYS}")
        z, speaker = self._prep(z, speaker)
        B, Tc = z.shape
        dev = z.device
        nc = _lib.int_array(n_codes, B, "n_codes")
        want_shape = (B, 2 * Tc, self.conf.rnnms.dim_voc_latent)
        if tuple(grad_cond.shape) != want_shape or grad_cond.dtype != torch.float32 or grad_cond.device != dev:
            raise RuntimeError(f"grad_cond must be a float32 tensor of shape {want_shape} on {dev} "
                               f"(got {grad_cond.dtype}, {tuple(grad_cond.shape)}, {grad_cond.device})")
        ws = self._cond_weights(self._cond_params() if weights is None else weights, dev)
        cond, saved = self._cond_fwd(z, speaker, nc, ws)
        grads = self._cond_bwd(z, speaker, nc, saved, grad_cond.detach().contiguous(), ws, tuple(k in want for k in self.COND_KEYS))
        with _lib.device_guard(dev):
            self.check()
        out = {k: g for k, g in zip(self.COND_KEYS, grads) if g is not None}
        out["cond"] = cond
        return out

    @torch.no_grad()
    def vocoder_gradients(self, audio: Tensor, z: Tensor, speaker: Tensor, *, lengths=None, n_codes=None, grad_loss=None) -> dict:
        """The gradients of ``nll(...).loss`` with respect to all 27 tensors of the vocoder, by ``state_dict()`` name: the direct
        form of ``nll(..., differentiable=True, train=TRAIN_PARTS).loss.backward()`` -- ``vqcpc_vocoder_cond_fwd``,
        ``vqcpc_vocoder_ar_fwd_cond``, ``vqcpc_vocoder_ar_bwd_cond`` asking for ``grad_cond``, ``vqcpc_vocoder_cond_bwd`` -- on the
        parameters as they are now.  -> dict of device tensors: the 27 names, ``loss`` (float64 scalar), ``nll_sum``, ``n_scored``,
        ``n_correct``.  Synchronises its stream (``check()``)."""
        call = self._nll_call(audio, z, speaker, lengths, n_codes)
        _, z, speaker, _, _, _, _, nc = call
        dev = z.device
        cw, aw = self._cond_weights(self._cond_params(), dev), self._ar_weights(self._ar_params(), dev)
        cond, csaved = self._cond_fwd(z, speaker, nc, cw)
        nll_sum, n_scored, n_correct, _, saved = self._ar_fwd(call, aw, cond_in=cond)
        gl = None if grad_loss is None else torch.tensor(float(grad_loss), dtype=torch.float32, device=dev)
        ar_grads, gc = self._ar_bwd(call, saved, aw, gl, cond_grad=True, cond_in=cond)
        cond_grads = self._cond_bwd(z, speaker, nc, csaved, gc, cw)
        with _lib.device_guard(dev):
            self.check()
        out = dict(zip(self.COND_KEYS + self.AR_NAMES, cond_grads + ar_grads))
        out.update(loss=nll_sum.sum() / n_scored.sum(), nll_sum=nll_sum, n_scored=n_scored, n_correct=n_correct)
        return out

    @torch.no_grad()
    def ar_gradients(self, audio: Tensor, z: Tensor, speaker: Tensor, *, lengths=None, n_codes=None, want=AR_KEYS, cond_grad: bool = False,
                     weights=None, grad_loss=None) -> dict:
        """The gradients of ``nll(...).loss`` (the mean NLL over every scored sample of the batch) with respect to the tensors of
        ``rnnms.ar`` that ``want`` names (keys of ``AR_KEYS``), and with ``cond_grad=True`` with respect to the conditioning series:
        one ``vqcpc_vocoder_ar_fwd`` and one ``vqcpc_vocoder_ar_bwd`` call (``csrc/vocoder_grad.hip``).  -> dict of device tensors:
        the wanted keys, ``cond`` and ``grad_cond`` (B, 2T', dim_voc_latent) with ``cond_grad``, ``loss`` (float64 scalar),
        ``nll_sum``, ``n_scored``, ``n_correct``.  ``weights``: nine tensors in the order of ``AR_KEYS`` read in place of the
        module's parameters' copies in the native handle (default: the parameters themselves, as they are now); ``grad_loss``: the
        upstream gradient, a number (default 1).  ``code_embedding``, ``speaker_embedding`` and ``rnnms.prenet`` receive no gradient
        here: ``cond_gradients`` takes ``grad_cond`` on to them, ``vocoder_gradients`` does both.  Synchronises its stream (``check()``)."""
        unknown = [k for k in want if k not in self.AR_KEYS]
        if unknown:
            raise ValueError(f"ar_gradients: unknown tensors {unknown}; known: {self.AR_KEYS}")
        call = self._nll_call(audio, z, speaker, lengths, n_codes)
        dev = call[1].device
        ws = self._ar_weights(self._ar_params() if weights is None else weights, dev)
        nll_sum, n_scored, n_correct, cond, saved = self._ar_fwd(call, ws, cond_grad)
        gl = None if grad_loss is None else torch.tensor(float(grad_loss), dtype=torch.float32, device=dev)
        grads, gc = self._ar_bwd(call, saved, ws, gl, tuple(k in want for k in self.AR_KEYS), cond_grad)
        with _lib.device_guard(dev):
            self.check()
        out = {k: g for k, g in zip(self.AR_KEYS, grads) if g is not None}
        out.update(loss=nll_sum.sum() / n_scored.sum(), nll_sum=nll_sum, n_scored=n_scored, n_correct=n_correct)
        if cond_grad:
            out.update(cond=cond, grad_cond=gc)
        return out

    def nll(self, audio: Tensor, z: Tensor, speaker: Tensor, *, lengths=None, n_codes=None, per_sample: bool = False,
            differentiable: bool = False, train=("ar",)) -> "VocoderNLL":
        """Teacher-forced negative log-likelihood per utterance: the vocoder's training objective (``vocoder.py:62-63``: the
        energies of ``audio[:, :-1]`` against the targets ``audio[:, 1:]``) as a number for held-out data, without the
        ``(B, T_s, 2**bits)`` energies ever existing (``vqcpc_vocoder_nll``).

        ``audio`` (B, L) integer mu-law classes; ``lengths`` valid samples per row of a padded batch (default L): row b scores
        the positions ``0 .. lengths[b] - 2`` and nothing behind them is read; ``n_codes`` valid codes per row (default T'),
        with ``lengths[b] - 1 <= 2 * upsampling_t * n_codes[b]``.  ``per_sample=True`` also returns the (B, L - 1) fp32 values.
        A class outside ``[0, 2**bits)`` in a scored position raises ``IndexError``.  Synchronises its stream (``check()``).

        ``differentiable=True`` (grad mode on, a parameter of ``rnnms.ar`` requiring grad): the returned ``.loss`` carries a
        ``grad_fn``.  Its forward is ``vqcpc_vocoder_ar_fwd`` on the parameters as they are (an optimizer step costs no new
        handle) and keeps ``h_t`` of every scored step; ``loss.backward()`` is one ``vqcpc_vocoder_ar_bwd`` call that asks only
        for the gradients of those of the nine ``rnnms.ar`` parameters that require one.  ``per_sample`` is not available with it.

        ``train``: the parts that receive a gradient, any of ``"ar"`` (``rnnms.ar``), ``"prenet"`` (``rnnms.prenet``) and
        ``"embeddings"`` (``code_embedding``, ``speaker_embedding``); the parameters of a part that is not named receive NONE.
        The default leaves the conditioning path frozen, as above.  With a conditioning part named the forward is
        ``vqcpc_vocoder_cond_fwd`` then ``vqcpc_vocoder_ar_fwd_cond`` on the parameters as they are, and ``backward()`` is one
        ``vqcpc_vocoder_ar_bwd_cond`` call asking for ``grad_cond`` then one ``vqcpc_vocoder_cond_bwd`` call, each asking only for
        the tensors of named parts that require a gradient: an optimizer step on any of the 27 tensors costs no new handle."""
        train = self._train_parts(train, "Vocoder.nll")
        if differentiable and torch.is_grad_enabled() and any(p.requires_grad for part in train for p in self._part_params(part)):
            if per_sample:
                raise ValueError("Vocoder.nll: per_sample is not available with differentiable=True")
            call = self._nll_call(audio, z, speaker, lengths, n_codes)
            if train == ("ar",):
                loss, nll_sum, n_scored, n_correct = _ArGrad.apply(self, call, *self._ar_params())
            else:
                loss, nll_sum, n_scored, n_correct = _VocGrad.apply(self, call, train, *self._cond_params(), *self._ar_params())
            with _lib.device_guard(call[1].device):
                self.check()
            return VocoderNLL(nll_sum, n_scored, n_correct, None, loss)
        with torch.no_grad():
            return self._nll_scored(audio, z, speaker, lengths, n_codes, per_sample)

    def _nll_scored(self, audio, z, speaker, lengths, n_codes, per_sample):
        audio, z, speaker, B, Tc, L, na, nc = self._nll_call(audio, z, speaker, lengths, n_codes)
        dev = z.device
        nll_sum = torch.empty(B, dtype=torch.float64, device=dev)
        n_scored = torch.empty(B, dtype=torch.int64, device=dev)
        n_correct = torch.empty(B, dtype=torch.int64, device=dev)
        nll = torch.empty(B, L - 1, device=dev) if per_sample else None
        with _lib.device_guard(dev):
            _lib.check(_lib.load().vqcpc_vocoder_nll(
                self._native(), audio.data_ptr(), z.data_ptr(), speaker.data_ptr(), B, Tc, L, nc, na, nll_sum.data_ptr(),
                n_scored.data_ptr(), n_correct.data_ptr(), nll.data_ptr() if per_sample and L > 1 else None,
                _lib.current_stream()))
            self.check()              # a bad class / code / speaker raises here and is not left latched
        return VocoderNLL(nll_sum, n_scored, n_correct, nll)

    @torch.no_grad()
    def glue(self, z: Tensor, speaker: Tensor) -> Tensor:
        """What ``network_vocoder.py:69-77`` hands to ``rnnms``: (B, 2T', dim_i_embedding + dim_speaker_embedding).  Synchronises
        its stream (``check()``)."""
        z, speaker = self._prep(z, speaker)
        B, Tc = z.shape
        out = torch.empty(B, 2 * Tc, self.conf.dim_i_embedding + self.conf.dim_speaker_embedding, device=z.device)
        with _lib.device_guard(z.device):
            _lib.check(_lib.load().vqcpc_vocoder_glue(self._native(), z.data_ptr(), speaker.data_ptr(), B, Tc, out.data_ptr(),
                                                      _lib.current_stream()))
            self.check()
        return out

    @torch.no_grad()
    def condition(self, z: Tensor, speaker: Tensor) -> Tensor:
        """PreNet output (B, 2T', dim_voc_latent) -- stage-level checks.  Synchronises its stream (``check()``)."""
        z, speaker = self._prep(z, speaker)
        B, Tc = z.shape
        out = torch.empty(B, 2 * Tc, self.conf.rnnms.dim_voc_latent, device=z.device)
        with _lib.device_guard(z.device):
            _lib.check(_lib.load().vqcpc_vocoder_condition(self._native(), z.data_ptr(), speaker.data_ptr(), B, Tc,
                                                           out.data_ptr(), _lib.current_stream()))
            self.check()
        return out


@dataclass
class VocoderNLL:
    """What ``Vocoder.nll`` returns: per utterance the summed negative log-likelihood in nats (float64), the number of scored
    samples and of samples whose target was the first maximum of the energies (int64), and per sample (B, L - 1) fp32 or None."""
    nll_sum: Tensor
    n_scored: Tensor
    n_correct: Tensor
    nll: object = None
    attached: object = None       # ``Vocoder.nll(..., differentiable=True)``: the same mean, carrying its ``grad_fn``

    @property
    def loss(self) -> Tensor:
        """Mean over every scored sample; with equal lengths exactly the reference's ``F.cross_entropy`` mean (``vocoder.py:63``)."""
        return self.attached if self.attached is not None else self.nll_sum.sum() / self.n_scored.sum()


class _ArGrad(torch.autograd.Function):
    """``Vocoder.nll(..., differentiable=True)``: ``forward`` is ``vqcpc_vocoder_ar_fwd`` and keeps ``saved``; ``backward`` is one
    ``vqcpc_vocoder_ar_bwd`` call asking for the gradients ``needs_input_grad`` names."""

    @staticmethod
    def forward(ctx, module, call, *ws):
        weights = module._ar_weights(ws, call[1].device)
        nll_sum, n_scored, n_correct, _, saved = module._ar_fwd(call, weights)
        ctx.module, ctx.kept = module, (call, saved)
        ctx.save_for_backward(*ws)                       # torch refuses the backward if an in-place step has moved them since
        ctx.mark_non_differentiable(nll_sum, n_scored, n_correct)
        return nll_sum.sum() / n_scored.sum(), nll_sum, n_scored, n_correct

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, *_):
        call, saved = ctx.kept
        module = ctx.module
        grads, _ = module._ar_bwd(call, saved, module._ar_weights(ctx.saved_tensors, call[1].device),
                                  grad_loss.to(torch.float32).contiguous(), ctx.needs_input_grad[2:])
        return (None, None) + tuple(grads)


class _VocGrad(torch.autograd.Function):
    """``Vocoder.nll(..., differentiable=True, train=...)`` with a conditioning part named: ``forward`` is ``vqcpc_vocoder_cond_fwd``
    then ``vqcpc_vocoder_ar_fwd_cond`` and keeps both ``saved`` buffers and the series; ``backward`` is one
    ``vqcpc_vocoder_ar_bwd_cond`` call asking for ``grad_cond`` and one ``vqcpc_vocoder_cond_bwd`` call, each asking for the
    gradients ``needs_input_grad`` names among the tensors of the parts in ``train``."""

    @staticmethod
    def forward(ctx, module, call, train, *ws):
        _, z, speaker, _, _, _, _, nc = call
        dev = z.device
        cw, aw = module._cond_weights(ws[:18], dev), module._ar_weights(ws[18:], dev)
        cond, csaved = module._cond_fwd(z, speaker, nc, cw)
        nll_sum, n_scored, n_correct, _, saved = module._ar_fwd(call, aw, cond_in=cond)
        ctx.module, ctx.kept, ctx.train = module, (call, cond, csaved, saved), train
        ctx.save_for_backward(*ws)                       # torch refuses the backward if an in-place step has moved them since
        ctx.mark_non_differentiable(nll_sum, n_scored, n_correct)
        return nll_sum.sum() / n_scored.sum(), nll_sum, n_scored, n_correct

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, *_):
        call, cond, csaved, saved = ctx.kept
        module, train = ctx.module, ctx.train
        _, z, speaker, _, _, _, _, nc = call
        dev = z.device
        need = ctx.needs_input_grad[3:]
        want_cond = tuple(n and (("embeddings" if i < 2 else "prenet") in train) for i, n in enumerate(need[:18]))
        want_ar = tuple(n and "ar" in train for n in need[18:])
        ws = ctx.saved_tensors
        ar_grads, gc = module._ar_bwd(call, saved, module._ar_weights(ws[18:], dev), grad_loss.to(torch.float32).contiguous(), want_ar,
                                      cond_grad=any(want_cond), cond_in=cond)
        cond_grads = [None] * 18
        if any(want_cond):
            cond_grads = module._cond_bwd(z, speaker, nc, csaved, gc, module._cond_weights(ws[:18], dev), want_cond)
        return (None, None, None) + tuple(cond_grads) + tuple(ar_grads)


class VocoderStream:
    """Chunks of one ``Vocoder.generate_stream`` call (``vqcpc_vocoder_stream_*``).  Each ``__next__`` decodes the next chunk,
    synchronises its stream and checks the handle like ``generate``: if the resident decoders reported the chunk (a shared GPU),
    it is decoded ONCE more from the state it started from -- the same samples -- with a warning; if that fails as well, the
    stream is closed (the state the next chunk would start from is not there) and the error raised.  Keeps its vocoder alive;
    ``close()`` frees the native stream (also at exhaustion and on garbage collection); ``position`` stays readable after it."""

    def __init__(self, voc, handle, st, B, chunk, device, return_mulaw):
        self._voc, self._handle, self._st = voc, handle, st
        self._B, self._chunk, self._device, self._return_mulaw = B, chunk, device, return_mulaw
        self._final = None                               # (done, total) at close

    def __iter__(self):
        return self

    @property
    def position(self):
        """(samples decoded so far per utterance, samples in all = 2 * upsampling_t * T'); after ``close()`` the last values."""
        if self._st is None:
            return self._final
        done, total = C.c_int64(), C.c_int64()
        _lib.check(_lib.load().vqcpc_vocoder_stream_position(self._st, C.byref(done), C.byref(total)))
        return int(done.value), int(total.value)

    @torch.no_grad()
    def __next__(self):
        if self._st is None:
            if self._final is not None and self._final[0] < self._final[1]:
                raise RuntimeError("VocoderStream was closed before its last chunk")
            raise StopIteration
        done, total = self.position
        if done >= total:
            self.close()
            raise StopIteration
        if self._voc._handle is None or self._voc._handle.value != self._handle.value:
            raise RuntimeError("VocoderStream: the vocoder's native handle was rebuilt (.to(), refresh(), load_state_dict) "
                               "after the stream was opened")
        lib = _lib.load()
        n = self._chunk
        wav = torch.empty(self._B, n, device=self._device)
        mulaw = torch.empty(self._B, n, dtype=torch.int64, device=self._device) if self._return_mulaw else None
        mp = mulaw.data_ptr() if mulaw is not None else None
        with _lib.device_guard(self._device):
            _lib.check(lib.vqcpc_vocoder_stream_next(self._st, n, wav.data_ptr(), mp, _lib.current_stream()))
            try:
                self._voc.check()
            except RuntimeError as e:
                import warnings
                warnings.warn(f"VocoderStream: chunk repeated ({e})")
                try:
                    _lib.check(lib.vqcpc_vocoder_stream_redo(self._st, wav.data_ptr(), mp, _lib.current_stream()))
                    self._voc.check()
                except BaseException:
                    self.close()                     # no good state to go on from: later chunks would decode garbage
                    raise
        keep = min(n, total - done)
        wav = wav[:, :keep]
        if mulaw is not None:
            return wav, mulaw[:, :keep]
        return wav

    def close(self):
        if getattr(self, "_st", None) is not None:
            self._final = self.position
            _lib.load().vqcpc_vocoder_stream_close(self._st)
            self._st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
