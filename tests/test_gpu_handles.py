"""-m gpu: lifecycle of the native handles behind ``Encoder``, ``CPCLoss`` and ``Vocoder`` (``_lib.NativeModule``) and of the
process-wide front-end handles: options survive a rebuild, a copy builds its own handle, ``refresh()`` and a reload are followed,
the front-end caches hand out one handle per key, a ``lengths`` list of the wrong size is refused, and a destroyed handle leaves
nothing behind: the library's own count of live device and pinned bytes (``vqcpc_debug_live_bytes``) returns exactly to where it
was, and ``workspace_bytes()`` is what the calls allocated.  Smallest shapes that reach the code: mel (1, 80, 32), codes (1, 4)
with ``max_steps=64``, the ``one_utt`` CPC shape, 1 600-sample waves."""
import copy
import ctypes as C
import gc

import pytest
import torch

import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib, loudness, preprocess, synth

pytestmark = pytest.mark.gpu

STEPS = 64


def encoder():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict())
    return enc.to("cuda").eval()


def vocoder():
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(synth.vocoder_state_dict())
    return voc.to("cuda").eval()


def cpc_module():
    cpc = V.CPCLoss(V.ConfCPC(2, 1, 1, 4, 64, 256))
    cpc.load_state_dict(synth.cpc_state_dict(n_prediction_steps=2))
    return cpc.to("cuda").eval()


def mel():
    return synth.mel("handles", 1, 32).cuda()


def encode(enc):
    return enc.encode_indices(mel())


def decode(voc):
    """The first STEPS mu-law classes of a (1, 4) call (nothing behind them is written)."""
    z, spk = torch.tensor([[3, 1, 4, 1]], device="cuda"), torch.tensor([5], device="cuda")
    return voc.generate(z, spk, seed=9, utt_base=0, return_mulaw=True, max_steps=STEPS)[1][:, :STEPS].clone()


def score(cpc):
    z, c = (t.cuda() for t in synth.cpc_inputs("handles", 1, 12))
    return cpc.forward_detailed(z, c)["loss"].clone()


def test_encoder_option_survives_a_rebuild():
    enc = encoder()
    encode(enc)
    assert enc.last_schedule() != 0                       # what a handle without the option runs on this shape
    enc.set_option("fused", 0)
    before = encode(enc)
    assert enc.last_schedule() == 0
    enc.load_state_dict(synth.encoder_state_dict())       # same weights, new versions: the handle is rebuilt
    after = encode(enc)
    assert enc.last_schedule() == 0
    assert torch.equal(after, before)


def test_vocoder_option_survives_a_rebuild():
    voc = vocoder()
    voc.set_option("xcd", 0)
    before = decode(voc)
    assert voc.last_path() == 0
    voc.load_state_dict(synth.vocoder_state_dict())
    after = decode(voc)
    assert voc.last_path() == 0
    assert torch.equal(after, before)


@pytest.mark.parametrize("make,call", [(encoder, encode), (cpc_module, score), (vocoder, decode)], ids=["Encoder", "CPCLoss", "Vocoder"])
def test_a_copy_builds_its_own_handle(make, call):
    m = make()
    want = call(m)
    assert m._handle is not None
    dup = copy.deepcopy(m)
    assert dup._handle is None
    got = call(dup)
    assert dup._native().value != m._native().value
    assert torch.equal(got, want)
    del dup
    gc.collect()
    assert torch.equal(call(m), want)


def test_cpc_refresh_and_reload():
    cpc = cpc_module()
    first = score(cpc)
    cpc.refresh()
    assert cpc._handle is None
    assert torch.equal(score(cpc), first) and cpc._handle is not None
    cpc.load_state_dict(synth.cpc_state_dict(seed=14, n_prediction_steps=2))
    assert not torch.equal(score(cpc), first)
    cpc.load_state_dict(synth.cpc_state_dict(n_prediction_steps=2))
    assert torch.equal(score(cpc), first)


def test_front_end_handles_are_cached():
    dev = torch.device("cuda", torch.cuda.current_device())
    conf = preprocess.ConfPreprocessing()
    assert preprocess._handle(conf, dev) is preprocess._handle(conf, dev)
    assert loudness._handle(16000, dev) is loudness._handle(16000, dev)
    w = torch.zeros(1600, device=dev)
    preprocess.resample(w, 16000, 8000)
    before = dict(preprocess._resamplers)
    preprocess.resample(w, 16000, 8000)
    assert before and preprocess._resamplers.keys() == before.keys()
    assert all(preprocess._resamplers[k] is h for k, h in before.items())


@pytest.mark.parametrize("n", [1, 3], ids=["one_too_few", "one_too_many"])
def test_lengths_of_the_wrong_size_are_refused(n):
    w = torch.zeros(2, 1600, device="cuda")
    with pytest.raises(ValueError, match="lengths must have one entry per row"):
        preprocess.wave_to_mel(w, lengths=[1600] * n)
    with pytest.raises(ValueError, match="lengths must have one entry per row"):
        preprocess.resample(w, 16000, 8000, lengths=[1600] * n)


# ------------------------------------------------------------------------------------------ ownership of device memory
def live_bytes():
    """(device, pinned) bytes the library holds in this process: every live handle's, the modules' cached ones included."""
    d, p = C.c_uint64(), C.c_uint64()
    _lib.check(_lib.load().vqcpc_debug_live_bytes(C.byref(d), C.byref(p)))
    return int(d.value), int(p.value)


def use_encoder(enc=None):
    enc = enc or encoder()
    enc.encode(mel())
    enc.forward(mel())
    enc.adapt_codebook(mel())
    return enc


def use_cpc():
    cpc = cpc_module()
    z, c = (t.cuda() for t in synth.cpc_inputs("handles", 1, 12))
    cpc.forward_detailed(z, c)
    g = cpc.gradients(z, c)
    assert all(g[k] is not None for k in ("z", "c", "W", "b"))
    return cpc


def use_vocoder(voc=None):
    """``generate`` on the resident decoders and on the launch path, ``nll``, and one chunk of a stream, which is returned open."""
    voc = voc or vocoder()
    decode(voc)
    assert voc.last_path() == 2
    voc.set_option("xcd", 0)
    decode(voc)
    assert voc.last_path() == 0
    z, spk = torch.tensor([[3, 1, 4, 1]], device="cuda"), torch.tensor([5], device="cuda")
    voc.nll(synth.randint("handles/audio", (1, STEPS + 1), 256).cuda(), z, spk)
    voc.set_option("xcd", -1)
    st = voc.generate_stream(z, spk, chunk_samples=160, seed=9, utt_base=0)
    assert next(st).shape == (1, 160)
    return voc, st


def wave():
    return (synth.mel("handles/wave", 1, 20)[0].reshape(-1) - 0.5).cuda()          # 1 600 samples in [-0.5, 0.5)


def abi_handle(create, *args):
    h = C.c_void_p()
    _lib.check(getattr(_lib.load(), create)(*args, C.byref(h)))
    return h


def use_melfront():
    lib, conf, w = _lib.load(), preprocess.ConfPreprocessing(), wave()
    h = abi_handle("vqcpc_melfront_create", conf.sr, conf.n_fft, conf.n_mels, conf.hop_length, conf.win_length, float(conf.fmin),
                   float(conf.preemph), float(conf.top_db))
    out = torch.empty(1, conf.n_mels, 1 + w.numel() // conf.hop_length, device="cuda")
    _lib.check(lib.vqcpc_melfront_run(h, w.data_ptr(), (C.c_int * 1)(w.numel()), 1, w.numel(), out.data_ptr(), _lib.current_stream()))
    return lambda: lib.vqcpc_melfront_destroy(h)


def use_loudness():
    lib, w = _lib.load(), wave()
    h = abi_handle("vqcpc_loudness_create", 4000)                  # 1 600 samples are one 400 ms block at 4 kHz
    lens, s = (C.c_int * 1)(w.numel()), _lib.current_stream()
    lufs, target = torch.empty(1, dtype=torch.float64, device="cuda"), torch.full((1,), -23.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.vqcpc_loudness_integrated(h, w.data_ptr(), lens, 1, w.numel(), lufs.data_ptr(), None, s))
    _lib.check(lib.vqcpc_loudness_normalize(h, w.data_ptr(), lens, 1, w.numel(), lufs.data_ptr(), target.data_ptr(), s))
    return lambda: lib.vqcpc_loudness_destroy(h)


def use_resampler():
    lib, w = _lib.load(), wave()
    h = abi_handle("vqcpc_resampler_create", 16000, 8000)
    n_out = lib.vqcpc_resampler_out_len(h, w.numel())
    out = torch.empty(n_out, device="cuda")
    _lib.check(lib.vqcpc_resampler_run(h, w.data_ptr(), (C.c_int * 1)(w.numel()), 1, w.numel(), out.data_ptr(), n_out, _lib.current_stream()))
    return lambda: lib.vqcpc_resampler_destroy(h)


def use_module(use):
    return lambda: use().refresh


def use_vocoder_and_stream():
    voc, st = use_vocoder()

    def drop():
        voc.refresh()
        st.close()                        # a stream owns its buffers: closing it after its vocoder is gone must not raise

    return drop


@pytest.mark.parametrize("use", [use_module(use_encoder), use_module(use_cpc), use_vocoder_and_stream, use_melfront, use_loudness,
                                 use_resampler], ids=["Encoder", "CPCLoss", "Vocoder", "melfront", "loudness", "resampler"])
def test_destroy_returns_every_byte(use):
    """Build a handle, make its calls, drop it: both counts are back where they were, exactly -- other live handles of the
    process are in both readings, so there is no tolerance."""
    gc.collect()                          # no module of an earlier test may go while this one counts
    torch.cuda.synchronize()
    before = live_bytes()
    drop = use()
    torch.cuda.synchronize()
    during = live_bytes()
    print("live (device, pinned) bytes: before", before, "with the handle", during)
    assert during[0] > before[0]
    drop()
    after = live_bytes()
    print("after the handle was dropped", after)
    assert after == before


# Allocated per call but not part of vqcpc_encoder_workspace_bytes, which include/vqcpc.h defines as front-end activations,
# statistics and the work space of the codebook update: the context scan's buffers belong to the LstmPlan (csrc/scan.hip) and
# have never been counted.  Sizes for mel (1, 80, 32): B = 1, T = 16 output frames, H = c_dim = 256, one 16-utterance tile.
CONTEXT_SCAN_BUFFERS = {"gi: hoisted input projection (B * T, 4 H) fp32": 1 * 16 * 4 * 256 * 4,
                        "hbuf: two halves of h, one tile (2, 16, H) fp32": 2 * 16 * 256 * 4,
                        "cbuf: cell state, one tile (16, H) fp32": 16 * 256 * 4,
                        "px: the resident scan's granules (2, 32 workers, 16) 8 bytes each": 2 * 32 * 16 * 8}


@pytest.mark.parametrize("name", ["Vocoder", "Encoder"])
def test_workspace_bytes_matches_the_count(name):
    """What the calls themselves allocated on a fresh handle (the rise of the device count since ``_native()`` built it: weights
    excluded) is what ``workspace_bytes()`` reports -- the hand-kept list of grow-only buffers, pinned to the truth in both
    directions."""
    gc.collect()
    m = vocoder() if name == "Vocoder" else encoder()
    m._native()
    torch.cuda.synchronize()
    base = live_bytes()[0]
    uncounted = 0
    if name == "Vocoder":
        use_vocoder(m)[1].close()         # the stream's buffers are its own and go with it
    else:
        use_encoder(m)
        uncounted = sum(CONTEXT_SCAN_BUFFERS.values())
    torch.cuda.synchronize()
    rise = live_bytes()[0] - base
    print(name, "rise of the device count", rise, "workspace_bytes", m.workspace_bytes(), "listed as uncounted", uncounted)
    assert rise == m.workspace_bytes() + uncounted
