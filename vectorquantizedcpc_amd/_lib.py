"""ctypes binding of ``libvqcpc_hip.so`` (C ABI declared in ``include/vqcpc.h``).

There is no CPU fallback: if the shared library is missing this module raises, and every
compute entry point fails on a machine without a gfx950 device.
"""
import contextlib
import ctypes as C
import os
import warnings
import weakref

import numpy as np
import torch
import torch.nn as nn

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvqcpc_hip.so")

# every symbol include/vqcpc.h declares (tests check the library exports exactly these)
SYMBOLS = [
    "vqcpc_abi_version", "vqcpc_last_error", "vqcpc_device_count",
    "vqcpc_encoder_create", "vqcpc_encoder_destroy", "vqcpc_encoder_encode",
    "vqcpc_encoder_forward_stats", "vqcpc_encoder_context", "vqcpc_encoder_context_saved_bytes", "vqcpc_encoder_context_fwd", "vqcpc_encoder_context_bwd", "vqcpc_encoder_stage", "vqcpc_encoder_vq_encode", "vqcpc_encoder_vq_adapt", "vqcpc_encoder_workspace_bytes", "vqcpc_encoder_set_option", "vqcpc_encoder_last_schedule",
    "vqcpc_cpc_create", "vqcpc_cpc_destroy", "vqcpc_cpc_score", "vqcpc_cpc_grad",
    "vqcpc_abx_workspace_bytes", "vqcpc_abx_score", "vqcpc_abx_index_workspace_bytes", "vqcpc_abx_code_table", "vqcpc_abx_score_indices",
    "vqcpc_encoder_check", "vqcpc_vocoder_check", "vqcpc_vocoder_last_path", "vqcpc_vocoder_last_slots", "vqcpc_vocoder_workspace_bytes", "vqcpc_vocoder_plan",
    "vqcpc_vocoder_create", "vqcpc_vocoder_destroy", "vqcpc_vocoder_generate",
    "vqcpc_vocoder_logits", "vqcpc_vocoder_nll", "vqcpc_vocoder_condition", "vqcpc_vocoder_glue", "vqcpc_vocoder_set_option",
    "vqcpc_vocoder_last_timing", "vqcpc_vocoder_kernel_times",
    "vqcpc_vocoder_stream_open", "vqcpc_vocoder_stream_next", "vqcpc_vocoder_stream_redo", "vqcpc_vocoder_stream_position",
    "vqcpc_vocoder_stream_close",
    "vqcpc_melfront_create", "vqcpc_melfront_destroy", "vqcpc_melfront_frames", "vqcpc_melfront_run",
    "vqcpc_loudness_create", "vqcpc_loudness_destroy", "vqcpc_loudness_blocks", "vqcpc_loudness_integrated",
    "vqcpc_loudness_normalize",
    "vqcpc_resampler_create", "vqcpc_resampler_destroy", "vqcpc_resampler_out_len", "vqcpc_resampler_run",
    "vqcpc_encoder_front_saved_bytes", "vqcpc_encoder_front_fwd", "vqcpc_encoder_front_bwd", "vqcpc_encoder_vq_bwd",
    "vqcpc_vocoder_ar_saved_bytes", "vqcpc_vocoder_ar_fwd", "vqcpc_vocoder_ar_bwd", "vqcpc_vocoder_ar_fwd_cond", "vqcpc_vocoder_ar_bwd_cond",
    "vqcpc_vocoder_cond_saved_bytes", "vqcpc_vocoder_cond_fwd", "vqcpc_vocoder_cond_bwd",
    "vqcpc_adam_step",
]

# the test surface of csrc/gate_probe.hip and csrc/runtime.hip: bound below, exported by the library, not declared in include/vqcpc.h
TEST_SYMBOLS = ["vqcpc_probe_gates", "vqcpc_probe_draw", "vqcpc_probe_words", "vqcpc_debug_live_bytes"]


class EncoderWeights(C.Structure):
    _fields_ = [("conv_weight", C.c_void_p), ("ln_weight", C.c_void_p * 5), ("ln_bias", C.c_void_p * 5),
                ("fc_weight", C.c_void_p * 4), ("out_weight", C.c_void_p), ("out_bias", C.c_void_p),
                ("codebook", C.c_void_p), ("rnn_w_ih", C.c_void_p), ("rnn_w_hh", C.c_void_p),
                ("rnn_b_ih", C.c_void_p), ("rnn_b_hh", C.c_void_p),
                ("in_channels", C.c_int), ("channels", C.c_int), ("n_embeddings", C.c_int),
                ("z_dim", C.c_int), ("c_dim", C.c_int)]


class EncoderFrontTensors(C.Structure):
    """``vqcpc_encoder_front_weights`` and ``vqcpc_encoder_front_grads`` (``include/vqcpc.h``): the same members, read or written."""
    _fields_ = [("conv_weight", C.c_void_p), ("ln_weight", C.c_void_p * 5), ("ln_bias", C.c_void_p * 5),
                ("fc_weight", C.c_void_p * 4), ("out_weight", C.c_void_p), ("out_bias", C.c_void_p)]


def fill_front(s, values):
    """Set the seventeen members ``EncoderWeights`` and ``EncoderFrontTensors`` share from ``values`` (device pointers or None) in
    the order of ``Encoder._FRONT_NAMES``: conv, 5 LayerNorm weights, 5 LayerNorm biases, 4 fc, out weight, out bias.  -> ``s``."""
    v = list(values)
    s.conv_weight, s.ln_weight[:], s.ln_bias[:], s.fc_weight[:], s.out_weight, s.out_bias = v[0], v[1:6], v[6:11], v[11:15], v[15], v[16]
    return s


class VocoderArTensors(C.Structure):
    """``vqcpc_vocoder_ar_weights`` and ``vqcpc_vocoder_ar_grads`` (``include/vqcpc.h``): the same nine members of
    ``rnnms.ar``, read or written."""
    _fields_ = [(n, C.c_void_p) for n in ("embedding", "w_ih", "w_hh", "b_ih", "b_hh", "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias")]


class VocoderCondTensors(C.Structure):
    """``vqcpc_vocoder_cond_weights`` and ``vqcpc_vocoder_cond_grads`` (``include/vqcpc.h``): the same eighteen
    members of the conditioning path, read or written; the prenet's indexed ``[layer][direction]`` as in ``VocoderWeights``."""
    _fields_ = [("code_embedding", C.c_void_p), ("speaker_embedding", C.c_void_p),
                ("prenet_w_ih", (C.c_void_p * 2) * 2), ("prenet_w_hh", (C.c_void_p * 2) * 2),
                ("prenet_b_ih", (C.c_void_p * 2) * 2), ("prenet_b_hh", (C.c_void_p * 2) * 2)]


class AdamTensor(C.Structure):
    """``vqcpc_adam_tensor`` (``include/vqcpc.h``)."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_uint64)]


class AdamHyper(C.Structure):
    """``vqcpc_adam_hyper`` (``include/vqcpc.h``)."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("step", C.c_int64)]


class CPCWeights(C.Structure):
    _fields_ = [("weight", C.c_void_p * 16), ("bias", C.c_void_p * 16),
                ("n_steps", C.c_int), ("n_speakers", C.c_int), ("n_utterances", C.c_int), ("n_negatives", C.c_int),
                ("z_dim", C.c_int), ("c_dim", C.c_int)]


class VocoderWeights(C.Structure):
    _fields_ = [("code_embedding", C.c_void_p), ("speaker_embedding", C.c_void_p),
                ("prenet_w_ih", (C.c_void_p * 2) * 2), ("prenet_w_hh", (C.c_void_p * 2) * 2),
                ("prenet_b_ih", (C.c_void_p * 2) * 2), ("prenet_b_hh", (C.c_void_p * 2) * 2),
                ("ar_embedding", C.c_void_p), ("ar_w_ih", C.c_void_p), ("ar_w_hh", C.c_void_p),
                ("ar_b_ih", C.c_void_p), ("ar_b_hh", C.c_void_p),
                ("fc1_weight", C.c_void_p), ("fc1_bias", C.c_void_p), ("fc2_weight", C.c_void_p), ("fc2_bias", C.c_void_p),
                ("n_codes", C.c_int), ("dz", C.c_int), ("n_speakers", C.c_int), ("ds", C.c_int), ("Hp", C.c_int),
                ("de", C.c_int), ("Hr", C.c_int), ("Hf", C.c_int), ("n_cls", C.c_int),
                ("upsample_t", C.c_int), ("bits_mu_law", C.c_int)]


_lib = None


def load():
    """Load the HIP library (raises if it has not been built: ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C vectorquantizedcpc_amd/csrc` "
            "(or __graft_entry__.build()).  vectorquantizedcpc_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64p = C.c_void_p, C.c_int, C.c_void_p
    lib.vqcpc_abi_version.restype = i32
    lib.vqcpc_last_error.restype = C.c_char_p
    lib.vqcpc_device_count.restype = i32
    lib.vqcpc_encoder_create.argtypes = [C.POINTER(EncoderWeights), C.POINTER(vp)]
    lib.vqcpc_encoder_destroy.argtypes = [vp]
    lib.vqcpc_encoder_destroy.restype = None
    lib.vqcpc_encoder_encode.argtypes = [vp, vp, i32, i32, i32, vp, vp, i64p, vp, vp]
    lib.vqcpc_encoder_forward_stats.argtypes = [vp, vp, vp, i64p, i32, vp, vp, vp, vp]
    lib.vqcpc_encoder_context.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.vqcpc_encoder_context_saved_bytes.argtypes = [vp, i32, i32, C.POINTER(C.c_uint64)]
    lib.vqcpc_encoder_context_fwd.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.vqcpc_encoder_context_bwd.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.vqcpc_encoder_front_saved_bytes.argtypes = [vp, i32, i32, C.POINTER(C.c_uint64)]
    lib.vqcpc_encoder_front_fwd.argtypes = [vp, vp, i32, i32, i32, C.POINTER(EncoderFrontTensors), vp, vp, vp]
    lib.vqcpc_encoder_front_bwd.argtypes = [vp, vp, i32, i32, i32, C.POINTER(EncoderFrontTensors), vp, vp, C.POINTER(EncoderFrontTensors), vp]
    lib.vqcpc_encoder_vq_bwd.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    lib.vqcpc_encoder_stage.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    lib.vqcpc_encoder_vq_encode.argtypes = [vp, vp, i32, vp, i64p, vp]
    lib.vqcpc_encoder_vq_adapt.argtypes = [vp, vp, i32, C.c_double, C.c_double, vp, vp, vp, vp, i64p, vp, vp, vp]
    lib.vqcpc_encoder_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.vqcpc_encoder_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.vqcpc_encoder_check.argtypes = [vp]
    lib.vqcpc_encoder_last_schedule.argtypes = [vp]
    lib.vqcpc_cpc_create.argtypes = [C.POINTER(CPCWeights), C.POINTER(vp)]
    lib.vqcpc_cpc_destroy.argtypes = [vp]
    lib.vqcpc_cpc_destroy.restype = None
    lib.vqcpc_cpc_score.argtypes = [vp, vp, vp, i32, i64p, i64p, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp, vp]
    lib.vqcpc_cpc_grad.argtypes = [vp, vp, vp, i32, vp, vp, i64p, i64p, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.vqcpc_adam_step.argtypes = [C.POINTER(AdamTensor), i32, C.POINTER(AdamHyper), vp]
    lib.vqcpc_abx_workspace_bytes.argtypes = [i32, i32, C.POINTER(C.c_uint64)]
    lib.vqcpc_abx_score.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp]
    lib.vqcpc_abx_index_workspace_bytes.argtypes = [i32, i32, C.POINTER(C.c_uint64)]
    lib.vqcpc_abx_code_table.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.vqcpc_abx_score_indices.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, i32]
    lib.vqcpc_vocoder_check.argtypes = [vp]
    lib.vqcpc_vocoder_last_path.argtypes = [vp]
    lib.vqcpc_vocoder_last_slots.argtypes = [vp]
    lib.vqcpc_vocoder_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.vqcpc_vocoder_plan.argtypes = [i32] * 7 + [C.POINTER(C.c_int), i32, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    lib.vqcpc_vocoder_create.argtypes = [C.POINTER(VocoderWeights), C.POINTER(vp)]
    lib.vqcpc_vocoder_destroy.argtypes = [vp]
    lib.vqcpc_vocoder_destroy.restype = None
    lib.vqcpc_vocoder_generate.argtypes = [vp, i64p, i64p, i32, i32, C.POINTER(C.c_int), C.c_uint64, C.c_uint32,
                                           C.POINTER(C.c_uint32), vp, i64p, i32, vp]
    lib.vqcpc_vocoder_logits.argtypes = [vp, i64p, i64p, i64p, i32, i32, i32, vp, vp]
    lib.vqcpc_vocoder_nll.argtypes = [vp, i64p, i64p, i64p, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int), vp, i64p, i64p, vp, vp]
    lib.vqcpc_vocoder_ar_saved_bytes.argtypes = [vp, i32, i32, C.POINTER(C.c_uint64)]
    lib.vqcpc_vocoder_ar_fwd.argtypes = [vp, i64p, i64p, i64p, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(VocoderArTensors),
                                         vp, i64p, i64p, vp, vp, vp]
    lib.vqcpc_vocoder_ar_bwd.argtypes = [vp, i64p, i64p, i64p, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(VocoderArTensors),
                                         vp, vp, C.POINTER(VocoderArTensors), vp, vp]
    lib.vqcpc_vocoder_cond_saved_bytes.argtypes = [vp, i32, i32, C.POINTER(C.c_uint64)]
    lib.vqcpc_vocoder_cond_fwd.argtypes = [vp, i64p, i64p, i32, i32, C.POINTER(C.c_int), C.POINTER(VocoderCondTensors), vp, vp, vp]
    lib.vqcpc_vocoder_cond_bwd.argtypes = [vp, i64p, i64p, i32, i32, C.POINTER(C.c_int), C.POINTER(VocoderCondTensors), vp, vp,
                                           C.POINTER(VocoderCondTensors), vp]
    lib.vqcpc_vocoder_ar_fwd_cond.argtypes = [vp, i64p, i64p, i64p, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.POINTER(VocoderArTensors), vp, vp, i64p, i64p, vp, vp, vp]
    lib.vqcpc_vocoder_ar_bwd_cond.argtypes = [vp, i64p, i64p, i64p, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.POINTER(VocoderArTensors), vp, vp, vp, C.POINTER(VocoderArTensors), vp, vp]
    lib.vqcpc_vocoder_condition.argtypes = [vp, i64p, i64p, i32, i32, vp, vp]
    lib.vqcpc_vocoder_glue.argtypes = [vp, i64p, i64p, i32, i32, vp, vp]
    lib.vqcpc_vocoder_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.vqcpc_vocoder_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.vqcpc_vocoder_kernel_times.argtypes = [vp, i32, C.POINTER(C.c_float), vp]
    lib.vqcpc_vocoder_stream_open.argtypes = [vp, i64p, i64p, i32, i32, C.POINTER(C.c_int), C.c_uint64, C.c_uint32,
                                              C.POINTER(C.c_uint32), C.POINTER(vp), vp]
    lib.vqcpc_vocoder_stream_next.argtypes = [vp, i32, vp, i64p, vp]
    lib.vqcpc_vocoder_stream_redo.argtypes = [vp, vp, i64p, vp]
    lib.vqcpc_vocoder_stream_position.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.vqcpc_vocoder_stream_close.argtypes = [vp]
    lib.vqcpc_vocoder_stream_close.restype = None
    lib.vqcpc_melfront_create.argtypes = [i32, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.POINTER(vp)]
    lib.vqcpc_melfront_destroy.argtypes = [vp]
    lib.vqcpc_melfront_destroy.restype = None
    lib.vqcpc_melfront_frames.argtypes = [vp, i32]
    lib.vqcpc_melfront_run.argtypes = [vp, vp, C.POINTER(C.c_int), i32, i32, vp, vp]
    lib.vqcpc_loudness_create.argtypes = [i32, C.POINTER(vp)]
    lib.vqcpc_loudness_destroy.argtypes = [vp]
    lib.vqcpc_loudness_destroy.restype = None
    lib.vqcpc_loudness_blocks.argtypes = [vp, i32]
    lib.vqcpc_loudness_integrated.argtypes = [vp, vp, C.POINTER(C.c_int), i32, i32, vp, vp, vp]
    lib.vqcpc_loudness_normalize.argtypes = [vp, vp, C.POINTER(C.c_int), i32, i32, vp, vp, vp]
    lib.vqcpc_resampler_create.argtypes = [i32, i32, C.POINTER(vp)]
    lib.vqcpc_resampler_destroy.argtypes = [vp]
    lib.vqcpc_resampler_destroy.restype = None
    lib.vqcpc_resampler_out_len.argtypes = [vp, i32]
    lib.vqcpc_resampler_run.argtypes = [vp, vp, C.POINTER(C.c_int), i32, i32, vp, i32, vp]
    lib.vqcpc_probe_gates.argtypes = [vp, i32, vp, vp]          # test surface of csrc/gate_probe.hip, not in include/vqcpc.h
    lib.vqcpc_probe_draw.argtypes = [vp, i32, vp, vp, vp]       # likewise
    lib.vqcpc_probe_words.argtypes = [vp, i32, i32, vp, vp]     # likewise
    lib.vqcpc_debug_live_bytes.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]    # likewise (csrc/runtime.hip)
    _lib = lib
    return lib


def check(rc: int):
    """Non-zero status -> RuntimeError(vqcpc_last_error()), like torch raising from an operator."""
    if rc != 0:
        raise RuntimeError(f"libvqcpc_hip: {load().vqcpc_last_error().decode()} (status {rc})")


def current_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class WeightSlots:
    """The tensors behind a fixed list of ``state_dict()`` names, re-read per call WITHOUT ``state_dict()`` (which
    costs ~70 us on these modules -- more than a small kernel call): each name is resolved once to the
    ``_parameters`` / ``_buffers`` dict that holds it, so a later ``.to()``, ``load_state_dict`` or assignment is
    still seen.  ``key()`` = ((data_ptr, _version), ...), what the native handles are cached on."""

    def __init__(self, module, names):
        self.names = list(names)
        self._module = weakref.ref(module)       # the module keeps its slots in its __dict__: a strong reference back would make
        self._resolve()                          # every module garbage that only the cycle collector frees -- its native handle
                                                 # (hipFree synchronises the device) would then go whenever a collection happens to run

    @property
    def module(self):
        return self._module()

    def _resolve(self):
        self.slots, self.owners = [], []
        for name in self.names:
            *path, leaf = name.split(".")
            mod, chain = self.module, []
            for part in path:
                chain.append((mod._modules, part, mod._modules[part]))
                mod = mod._modules[part]
            self.slots.append((mod._parameters if leaf in mod._parameters else mod._buffers, leaf))
            self.owners.append(chain)

    def tensors(self):
        # a submodule replaced after the first call (enc.rnn = nn.LSTM(...)) leaves the resolved dicts pointing at the old
        # one: one identity check per path element (~1 us for the whole list) catches it
        for chain in self.owners:
            for mods, part, seen in chain:
                if mods.get(part) is not seen:
                    self._resolve()
                    return [d[k] for d, k in self.slots]
        return [d[k] for d, k in self.slots]

    @staticmethod
    def key(tensors):
        dev = tensors[0].device
        return (dev.type, dev.index) + tuple([(t.data_ptr(), t._version) for t in tensors])


def device_guard(dev):
    """``torch.cuda.device(dev)`` only when ``dev`` is not already current (the context manager costs ~5 us)."""
    return contextlib.nullcontext() if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def require_same_device(t, ref, what: str):
    """torch's 'expected all tensors to be on the same device' for an input next to the module's weights."""
    if t.device != ref.device:
        raise RuntimeError(f"Expected all tensors to be on the same device, but {what} is on {t.device} and the "
                           f"module's parameters are on {ref.device}")


def require_cuda(t, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: vectorquantizedcpc_amd runs on MI355X only "
                           "(move the module and its inputs with .to('cuda')); there is no CPU fallback")


def int_array(values, n: int, what: str, ctype=C.c_int):
    """Per-utterance host integers (list or Tensor; ``None`` stays ``None``) -> ``ctype[n]`` for the C ABI.  A list of the wrong
    length raises: ctypes would zero-fill a short one without a word, so those utterances would run as empty."""
    if values is None:
        return None
    v = values.tolist() if isinstance(values, torch.Tensor) else values
    if len(v) != n:
        raise RuntimeError(f"{what} must have one entry per utterance ({n}), got {len(v)}")
    return (ctype * n)(*map(int, v))


def wave_batch(wave, lengths, what: str = "wave"):
    """A waveform argument of the front ends -> ``(single, w, lens, c_int[B])``: ``w`` (B, Lmax) fp32, contiguous, on its HIP
    device -- a numpy waveform is moved to the current one, (L,) becomes (1, L) and ``single`` says so -- and ``lens`` the
    valid samples per row (default Lmax), as a list and as the array the C calls take."""
    if isinstance(wave, np.ndarray):
        wave = torch.from_numpy(np.ascontiguousarray(wave, dtype=np.float32)).cuda()
    require_cuda(wave, what)
    single = wave.dim() == 1
    w = wave[None] if single else wave
    if w.dim() != 2:
        raise ValueError("mono audio only: (L,) or (B, Lmax) with lengths")
    B, Lmax = w.shape
    lens = [Lmax] * B if lengths is None else [int(v) for v in lengths]
    if len(lens) != B:
        raise ValueError("lengths must have one entry per row")
    return single, w.detach().to(torch.float32).contiguous(), lens, int_array(lens, B, "lengths")


def cached_handle(cache: dict, device, create: str, *args):
    """The process-wide handle of a front end (mel, loudness, resampler): ``cache[args + (device.index,)]``, made on first use
    by the library's ``create(*args, &handle)`` on ``device``.  Such handles hold only tables and live as long as the process."""
    key = args + (device.index,)
    h = cache.get(key)
    if h is None:
        h = C.c_void_p()
        with device_guard(device):
            check(getattr(load(), create)(*args, C.byref(h)))
        cache[key] = h
    return h


def adam_step(table, n: int, hyper, device):
    """One ``vqcpc_adam_step`` call: the first ``n`` rows of ``table`` (an ``AdamTensor`` array) with ``hyper`` (an ``AdamHyper``), on
    the current stream of ``device``."""
    with device_guard(device):
        check(load().vqcpc_adam_step(table, n, C.byref(hyper), current_stream()))


def run_checked(run, check, message: str):
    """The repeat-once policy of every call whose result the host takes right away: ``out = run()``, then ``check()`` (one
    stream synchronisation and the handle's status word).  A ``RuntimeError`` there means an in-kernel exchange gave up (a shared
    GPU) and the handle has fallen back to its launch-per-step path: warn with ``message`` (``{}`` = the error), run ONCE more
    and check again.  Anything else ``check()`` raises (``IndexError`` for a bad index) passes straight through."""
    out = run()
    try:
        check()
    except RuntimeError as e:
        warnings.warn(message.format(e))
        out = run()
        check()
    return out


class NativeModule(nn.Module):
    """An ``nn.Module`` whose arithmetic runs behind one native handle of ``libvqcpc_hip.so``: the lifecycle of that handle.
    The handle holds re-laid COPIES of the weights; it is built at the first call that needs it (``_native()``), keyed on
    ``WeightSlots.key`` of the weights, rebuilt when that key moves (``load_state_dict``, ``.to``, optimizer steps) -- with the
    options set so far applied again -- and never copied or pickled with the module.

    A subclass states what differs: ``_NAME`` for the messages, ``_WEIGHT_NAMES`` (``state_dict()`` names; or
    ``_weight_names()`` where they depend on the instance), the library symbols ``_CREATE``, ``_DESTROY`` and, if it has options,
    ``_SET_OPTION``, and ``_weights(p)``: its ctypes weights struct, filled, with ``p(name)`` = the device pointer of weight
    ``name``."""
    _NAME = _CREATE = _DESTROY = _SET_OPTION = None
    _WEIGHT_NAMES = ()

    def __init__(self):
        super().__init__()
        self._handle = None
        self._handle_key = None

    def _weight_names(self):
        return self._WEIGHT_NAMES

    def _weights(self, p):
        raise NotImplementedError

    def _native(self):
        slots = self.__dict__.get("_slots")
        if slots is None:                       # resolved once: state_dict() costs more than a short call's launch
            slots = self.__dict__["_slots"] = WeightSlots(self, self._weight_names())
        ws = slots.tensors()
        key = WeightSlots.key(ws)
        if self._handle is not None and key == self._handle_key:
            return self._handle
        for t in ws:
            require_cuda(t, f"{self._NAME} parameter")
            if t.dtype != torch.float32:
                raise RuntimeError(f"{self._NAME}: parameters must be float32")
            require_same_device(t, ws[0], "a parameter")
        self._release()
        sd = dict(zip(slots.names, ws))
        keep = []                               # contiguous copies stay alive until create has re-laid them

        def p(name):
            t = sd[name].detach().contiguous()
            keep.append(t)
            return t.data_ptr()

        w = self._weights(p)
        lib = load()
        h = C.c_void_p()
        with device_guard(ws[0].device):
            torch.cuda.current_stream().synchronize()
            check(getattr(lib, self._CREATE)(C.byref(w), C.byref(h)))
        self._handle, self._handle_key = h, key
        for name, value in self.__dict__.get("_options", {}).items():     # options survive a rebuild of the handle
            check(getattr(lib, self._SET_OPTION)(h, name.encode(), value))
        return h

    def _live_handle(self, dev):
        """The handle if one is live on ``dev`` -- also one whose copies an optimizer step has made stale -- else None."""
        if self._handle is not None and self._handle_key[:2] == (dev.type, dev.index):
            return self._handle
        return None

    def _sizes_handle(self, dev, read_from_handle=()):
        """The handle for a call that reads weights from the CALLER's pointers (the ``*_fwd`` / ``*_bwd`` / ``*_grad`` entries).
        For those tensors the handle gives sizes and work space only, so a live handle on ``dev`` whose copies of them an optimizer
        step has made stale still serves: ``_native()`` would answer the moved ``WeightSlots.key`` with destroy, create and a
        synchronisation per step.  ``read_from_handle``: the ``state_dict()`` names such an entry nevertheless reads from the
        handle's COPIES (the vocoder's frozen conditioning path); the live handle is reused only while the key of every one of them
        is the one it was built from, and rebuilt through ``_native()`` otherwise -- ``load_state_dict`` or an in-place write to
        one of them is never missed.  Calls that read the handle's copies throughout go through ``_native()``, which rebuilds once
        when it sees a moved ``_version``."""
        h = self._live_handle(dev)
        if h is not None and read_from_handle:
            slots = self.__dict__["_slots"]                  # a live handle was built from them
            for i, (name, t) in enumerate(zip(slots.names, slots.tensors())):
                if name in read_from_handle and (t.data_ptr(), t._version) != self._handle_key[2 + i]:
                    h = None
                    break
        return h if h is not None else self._native()

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            getattr(load(), self._DESTROY)(self._handle)
            self._handle = None

    def __getstate__(self):                             # the native handle is per object: a copy builds its own
        d = self.__dict__.copy()
        d["_handle"], d["_handle_key"] = None, None
        d.pop("_slots", None)
        return d

    def set_option(self, name: str, value: int):
        """The subclass's ``vqcpc_*_set_option``.  ``Encoder``: ``fused`` (-1 auto, 0 layered kernels, 1 fused front end);
        ``Vocoder``: the decode-loop options (``use_graph``, ``steps_per_graph``, ``xcd``, ...).  Options are kept on the
        Python object and re-applied when the native handle is rebuilt (``.to()``, ``load_state_dict``)."""
        if self._SET_OPTION is None:
            raise AttributeError(f"{self._NAME} has no options")
        check(getattr(load(), self._SET_OPTION)(self._native(), name.encode(), int(value)))
        self.__dict__.setdefault("_options", {})[name] = int(value)

    def refresh(self):
        """Drop the native handle so that the next call re-reads the parameters.  The handle holds re-laid
        COPIES of the weights and is rebuilt automatically when a parameter's storage or ``_version`` changes
        (``load_state_dict``, ``.to``, optimizer steps); a write through ``.data`` bumps neither -- call this
        after one."""
        self._release()
        self._handle_key = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass
