"""-m gpu: lifecycle of the native handles behind ``Encoder``, ``CPCLoss`` and ``Vocoder`` (``_lib.NativeModule``) and of the
process-wide front-end handles: options survive a rebuild, a copy builds its own handle, ``refresh()`` and a reload are followed,
the front-end caches hand out one handle per key, and a ``lengths`` list of the wrong size is refused.  Smallest shapes that
reach the code: mel (1, 80, 32), codes (1, 4) with ``max_steps=64``, the ``one_utt`` CPC shape."""
import copy
import gc

import pytest
import torch

import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import loudness, preprocess, synth

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
