"""-m gpu: streaming decode (Vocoder.generate_stream / vqcpc_vocoder_stream_*).  Every check is bit equality of the concatenated
chunks with one generate() call on the same seed and sampling-stream ids, waveform and mu-law classes: on the resident per-XCD
decoders (all three slot layouts), on the launch-per-step kernels (fused and three-launch, large-batch kernel, back-to-back slots),
with more utterances than decode slots, at other model sizes, at the benchmark's sizes, across interleaved streams and calls on
one handle, and through a reported chunk that is decoded again."""
import ctypes as C

import pytest
import torch

import decode_harness as H
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib, synth

pytestmark = pytest.mark.gpu
vocoder = H.Handles()


def inputs(tag, B, Tc, ragged=True):
    z, spk = H.inputs(f"st/?{tag}{B}", B, Tc)
    return z, spk, H.ragged_countdown(B, Tc) if ragged and B > 1 else None


@pytest.mark.parametrize("B,slots", [(1, (1, 1)), (5, (5, 5)), (12, (9, 16)), (20, (17, 32)), (32, (32, 32))])
@pytest.mark.parametrize("chunk", [160, 480, 1120])
def test_resident_decoders(B, slots, chunk):
    """The slot layout follows the slots in use (xd_pick_bxt of slots per XCD): B = 1 and 5 run ar_xcd_resume_kernel<1> (one slot
    per XCD, some XCDs idle at 5), 12 <2> (two per XCD), 20 <4>, 32 <4> with all four MFMA columns live."""
    voc, _ = vocoder()
    z, spk, n_codes = inputs("r", B, 4)
    st = voc.generate_stream(z, spk, chunk_samples=chunk, seed=17, utt_base=5, n_codes=n_codes)
    next(st)                                              # the first chunk: every utterance live
    assert voc.last_path() == 2 and slots[0] <= voc.last_slots() <= slots[1]
    st.close()
    assert st.position == (chunk, 1280)
    H.assert_same(voc, z, spk, chunk, path=2, n_codes=n_codes)


@pytest.mark.parametrize("B,fuse", [(1, 1), (3, 0), (3, 1), (17, 1), (40, 0), (80, 1)])
def test_launch_path(B, fuse):
    """xcd = 0: ar_gru_kernel (one and two tiles, fused and three-launch), two tile groups on two streams at 40 three-launch
    (three tiles: 2 + 1, each group with its own state, slot table and call record), ar_gru_big_kernel at 80 (five tiles)."""
    voc, _ = vocoder(fresh=True)
    voc.set_option("xcd", 0)
    voc.set_option("fuse_fc2", fuse)
    z, spk, n_codes = inputs("l", B, 4)
    for chunk in (160, 480):
        H.assert_same(voc, z, spk, chunk, path=0, n_codes=n_codes)


def test_launch_path_back_to_back_slots():
    voc, _ = vocoder(fresh=True)
    voc.set_option("xcd", 0)
    voc.set_option("slots", 4)
    z, spk, n_codes = inputs("b", 6, 4)
    H.assert_same(voc, z, spk, 480, path=0, n_codes=n_codes)
    assert voc.last_slots() == 4


@pytest.mark.parametrize("B", [40, 100])
def test_more_utterances_than_slots(B):
    """Resumed segments back to back in the 32 slots of ar_xcd.hip; the one-shot call at 100 runs on ar_xcm.hip."""
    voc, _ = vocoder()
    z, spk, n_codes = inputs("m", B, 3)
    voc.generate(z, spk, seed=3, utt_base=0, n_codes=n_codes)
    assert voc.last_path() == (2 if B <= 68 else 3)
    st = voc.generate_stream(z, spk, chunk_samples=640, seed=3, utt_base=0, n_codes=n_codes)
    next(st)
    assert voc.last_slots() == 32                          # the first chunk: every utterance live, 32 slots, the rest behind them
    st.close()
    H.assert_same(voc, z, spk, 640, path=2, n_codes=n_codes)


def test_other_sizes_launch_path():
    sd = synth.vocoder_state_dict(size_h_rnn=512, size_h_fc=512, bits_mu_law=9)
    conf = V.ConfVocoder()
    conf.rnnms.bits_mu_law = 9
    conf.rnnms.wave_ar.size_h_rnn = 512
    conf.rnnms.wave_ar.size_h_fc = 512
    voc, _ = vocoder(conf=conf, sd=sd)
    z, spk, n_codes = inputs("o", 3, 3)
    for chunk in (160, 320):
        H.assert_same(voc, z, spk, chunk, path=0, n_codes=n_codes)


@pytest.mark.parametrize("B,chunk", [(1, 1600), (32, 3200), (1, 32000)])
def test_full_size(B, chunk):
    """1 x 32 000 and the benchmark's 32 x 32 000 (Tc = 100 codes), and one chunk for the whole utterance."""
    voc, _ = vocoder()
    z = synth.randint(f"st/full{B}", (B, 100), 512).cuda()
    spk = synth.randint(f"st/fulls{B}", (B,), 102).cuda()
    H.assert_same(voc, z, spk, chunk, path=2, seed=11, utt_base=0)


def test_interleaved_streams_and_calls():
    voc, _ = vocoder(fresh=True)
    za, sa, na = inputs("ia", 3, 4)
    zb, sb, _ = inputs("ib", 2, 3, ragged=False)
    zc, sc, _ = inputs("ic", 5, 2, ragged=False)
    torch.manual_seed(1234)
    a = voc.generate_stream(za, sa, chunk_samples=320, n_codes=na, return_mulaw=True, seed=21)
    b = voc.generate_stream(zb, sb, chunk_samples=480, return_mulaw=True, seed=22)
    assert voc._utterances_done == 5                       # default ids: 0..2 for a, 3..4 for b
    got = {"a": [], "b": []}
    other = None
    while a.position[0] < a.position[1] or b.position[0] < b.position[1]:
        for name, st in (("a", a), ("b", b)):
            if st.position[0] < st.position[1]:
                got[name].append(next(st))
            w = voc.generate(zc, sc, seed=5, utt_base=100)      # overwrites the handle's own conditioning buffers
            other = w if other is None else other
            assert torch.equal(w, other)
    with pytest.raises(StopIteration):
        next(a)
    for name, z, s, seed, base, nc in (("a", za, sa, 21, 0, na), ("b", zb, sb, 22, 3, None)):
        want_w, want_m = voc.generate(z, s, return_mulaw=True, seed=seed, utt_base=base, n_codes=nc)
        assert torch.equal(torch.cat([w for w, _ in got[name]], 1), want_w)
        assert torch.equal(torch.cat([m for _, m in got[name]], 1), want_m)


def test_reported_chunk_is_decoded_again():
    voc, _ = vocoder(fresh=True)
    z, spk, n_codes = inputs("re", 4, 4)
    want_w, want_m = voc.generate(z, spk, return_mulaw=True, seed=9, utt_base=0, n_codes=n_codes)
    # Python: the stream repeats the chunk once, with a warning
    st = voc.generate_stream(z, spk, chunk_samples=320, return_mulaw=True, seed=9, utt_base=0, n_codes=n_codes)
    chunks = [next(st), next(st)]
    voc.set_option("xcd_debug_misplace", 1)
    with pytest.warns(UserWarning, match="not dealt 32"):
        chunks.append(next(st))
    chunks += list(st)
    assert voc.last_path() == 2
    assert torch.equal(torch.cat([w for w, _ in chunks], 1), want_w) and torch.equal(torch.cat([m for _, m in chunks], 1), want_m)
    # C: stream_next + check reports the chunk, stream_redo gives its samples
    lib = _lib.load()
    st = voc.generate_stream(z, spk, chunk_samples=320, return_mulaw=True, seed=9, utt_base=0, n_codes=n_codes)
    head = [next(st), next(st)]
    wav = torch.empty(4, 320, device="cuda")
    mu = torch.empty(4, 320, dtype=torch.int64, device="cuda")
    voc.set_option("xcd_debug_misplace", 1)
    _lib.check(lib.vqcpc_vocoder_stream_next(st._st, 320, wav.data_ptr(), mu.data_ptr(), _lib.current_stream()))
    with pytest.raises(RuntimeError, match="not dealt 32"):
        voc.check()
    done, total = C.c_int64(), C.c_int64()
    _lib.check(lib.vqcpc_vocoder_stream_position(st._st, C.byref(done), C.byref(total)))
    assert (done.value, total.value) == (960, 1280)
    _lib.check(lib.vqcpc_vocoder_stream_redo(st._st, wav.data_ptr(), mu.data_ptr(), _lib.current_stream()))
    voc.check()
    assert torch.equal(mu, want_m[:, 640:960]) and torch.equal(wav, want_w[:, 640:960])
    tail = list(st)
    assert torch.equal(torch.cat([w for w, _ in head] + [wav] + [w for w, _ in tail], 1), want_w)
    assert st.position == (1280, 1280)                   # still readable once the stream closed itself
    assert st._st is None                                # closed at exhaustion


def test_a_chunk_that_fails_twice_ends_the_stream(monkeypatch):
    """If the repeat of a reported chunk is reported as well, the state the next chunk would start from is not there: the stream
    closes, raises, and refuses to go on."""
    voc, _ = vocoder(fresh=True)
    z, spk, n_codes = inputs("f", 3, 2)
    st = voc.generate_stream(z, spk, chunk_samples=160, seed=9, utt_base=0, n_codes=n_codes)
    next(st)

    def failing_check():
        torch.cuda.current_stream().synchronize()
        raise RuntimeError("libvqcpc_hip: decode not run (a test stand-in)")
    monkeypatch.setattr(voc, "check", failing_check)
    with pytest.warns(UserWarning, match="chunk repeated"), pytest.raises(RuntimeError, match="test stand-in"):
        next(st)
    monkeypatch.undo()
    assert st._st is None and st.position == (320, 640)
    with pytest.raises(RuntimeError, match="closed before its last chunk"):
        next(st)
