"""-m gpu: every ``VQCPC_ERR_INVALID`` condition of ``include/vqcpc.h`` through raw ctypes: the call returns -1
with a message that names the condition, and nothing is enqueued -- the outputs keep the pattern they were filled with."""
import ctypes

import pytest
import torch

import cond_grad_ref as R
import voc_grad_ref as VR
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib

pytestmark = pytest.mark.gpu

INVALID = -1
ints = lambda v: None if v is None else (ctypes.c_int * len(v))(*v)
ptr = lambda t: t if isinstance(t, int) or t is None else t.data_ptr()


def test_cond_entries_enqueue_nothing_on_an_error():
    c = R.load("hp64")
    voc = V.Vocoder(V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(dim_voc_latent=c["C"], wave_ar=V.ConfWaveAR(size_h_rnn=512))))
    voc.load_state_dict(c["sd"])
    voc = voc.cuda().eval()
    lib, h, s = _lib.load(), voc._native(), _lib.current_stream()
    B, Tc, C = c["B"], c["Tc"], c["C"]
    z, spk, G = c["z"].cuda(), c["spk"].cuda(), c["G"].cuda()
    n = ctypes.c_uint64()
    saved_bytes = lib.vqcpc_vocoder_cond_saved_bytes
    assert saved_bytes(h, B, Tc, ctypes.byref(n)) == 0 and n.value % 16 == 0 and n.value >= B * 2 * Tc * (128 + 2 * C) * 4
    assert saved_bytes(h, 0, Tc, ctypes.byref(n)) == INVALID and saved_bytes(h, B, 0, ctypes.byref(n)) == INVALID
    assert saved_bytes(None, B, Tc, ctypes.byref(n)) == INVALID and saved_bytes(h, B, Tc, None) == INVALID
    assert saved_bytes(h, B, Tc, ctypes.byref(n)) == 0
    saved = torch.full((n.value // 4,), -7.0, device="cuda")
    cond = torch.full((B, 2 * Tc, C), -7.0, device="cuda")
    ws = [p.detach().contiguous() for p in voc._cond_params()]
    outs = [torch.full_like(w, -7.0) for w in ws]

    def struct(ts):
        return None if ts is None else voc._cond_struct([None if t is None else _Ptr(ptr(t)) for t in ts])

    def fwd(h=h, z=z.data_ptr(), spk=spk.data_ptr(), B=B, Tc=Tc, nc=None, w=ws, cond=cond.data_ptr(), saved=saved.data_ptr()):
        return lib.vqcpc_vocoder_cond_fwd(h, z, spk, B, Tc, ints(nc), struct(w), cond, saved, s)

    def bwd(h=h, z=z.data_ptr(), spk=spk.data_ptr(), B=B, Tc=Tc, nc=None, w=ws, saved=saved.data_ptr(), cond=G.data_ptr(), outs=outs):
        return lib.vqcpc_vocoder_cond_bwd(h, z, spk, B, Tc, ints(nc), struct(w), saved, cond, struct(outs), s)

    err = lib.vqcpc_last_error
    for call in (fwd, bwd):
        assert call(h=None) == INVALID and call(z=None) == INVALID and call(spk=None) == INVALID and call(saved=None) == INVALID
        assert call(cond=None) == INVALID and b"null argument" in err()
        assert call(B=0) == INVALID and call(Tc=0) == INVALID and call(B=-1) == INVALID and b"need B >= 1" in err()
        assert call(nc=[Tc + 1] * B) == INVALID and b"n_codes" in err()
        assert call(nc=[-1] * B) == INVALID and b"n_codes" in err()
        assert call(saved=saved.data_ptr() + 4) == INVALID and b"16-byte aligned" in err()
        assert call(cond=cond.data_ptr() + 4) == INVALID and b"16-byte aligned" in err()
        for i in range(18):
            assert call(w=ws[:i] + [None] + ws[i + 1:]) == INVALID and b"all eighteen tensors" in err(), i
        assert call(w=ws[:5] + [ws[5].data_ptr() + 4] + ws[6:]) == INVALID and b"16-byte aligned" in err()
        if torch.cuda.device_count() > 1:
            with torch.cuda.device(1):
                assert call() == INVALID and b"belongs to device" in err()
    assert bwd(outs=None) == INVALID and b"null argument" in err()
    assert bwd(outs=[None] * 18) == INVALID and b"no wanted output" in err()
    assert bwd(outs=[None] * 17 + [outs[17].data_ptr() + 4]) == INVALID and b"16-byte aligned" in err()
    torch.cuda.synchronize()
    for t in [saved, cond] + outs:
        assert bool((t == -7).all())
    # the same calls, valid: everything wanted is written
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    voc.check()
    assert bool((cond != -7.0).all()) and all(bool((o != -7.0).all()) for o in outs)
    assert fwd(w=None) == 0 and bwd(w=None, outs=[None] * 17 + [outs[17]]) == 0
    assert fwd(nc=[0] * B) == 0 and bwd(nc=[0] * B) == 0              # no utterance has a code: a series and gradients of +0
    torch.cuda.synchronize()
    voc.check()
    assert not cond.view(torch.int32).any() and all(not o.view(torch.int32).any() for o in outs)


class _Ptr:
    """A raw address where ``Vocoder._cond_struct`` expects a tensor."""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def test_scoring_entries_with_a_series_check_it():
    c = VR.load("h512")
    voc = V.Vocoder(V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(dim_voc_latent=c["C"], upsampling_t=c["up"],
                                                           wave_ar=V.ConfWaveAR(size_i_embed_ar=c["de"], size_h_rnn=c["Hr"]))))
    voc.load_state_dict(c["sd"])
    voc = voc.cuda().eval()
    lib, h, s = _lib.load(), voc._native(), _lib.current_stream()
    B, Tc, L, C = c["B"], c["Tc"], c["L"], c["C"]
    audio, z, spk = c["audio"].cuda(), c["z"].cuda(), c["spk"].cuda()
    n = ctypes.c_uint64()
    assert lib.vqcpc_vocoder_ar_saved_bytes(h, B, L, ctypes.byref(n)) == 0
    saved = torch.full((n.value // 4,), -7.0, device="cuda")
    sums = [torch.full((B,), -7.0, dtype=torch.float64, device="cuda"), torch.full((B,), -7, dtype=torch.int64, device="cuda"),
            torch.full((B,), -7, dtype=torch.int64, device="cuda")]
    cond_in = voc.condition(z, spk)
    gcond = torch.full((B, 2 * Tc, C), -7.0, device="cuda")

    def fwd(cond_in=cond_in.data_ptr(), B=B, saved=saved.data_ptr(), nc=None):
        return lib.vqcpc_vocoder_ar_fwd_cond(h, audio.data_ptr(), z.data_ptr(), spk.data_ptr(), B, Tc, L, ints(nc), None, None, cond_in,
                                             *[t.data_ptr() for t in sums], None, saved, s)

    def bwd(cond_in=cond_in.data_ptr(), B=B, saved=saved.data_ptr(), nc=None):
        return lib.vqcpc_vocoder_ar_bwd_cond(h, audio.data_ptr(), z.data_ptr(), spk.data_ptr(), B, Tc, L, ints(nc), None, None, cond_in,
                                             saved, None, None, gcond.data_ptr(), s)

    err = lib.vqcpc_last_error
    for call in (fwd, bwd):
        assert call(cond_in=None) == INVALID and b"cond_in" in err()
        assert call(cond_in=cond_in.data_ptr() + 4) == INVALID and b"cond_in" in err()
        assert call(B=0) == INVALID and call(saved=None) == INVALID and call(nc=[Tc + 1] * B) == INVALID      # the plain entries' conditions
    torch.cuda.synchronize()
    for t in [saved, gcond] + sums:
        assert bool((t == -7).all())
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    voc.check()
    assert bool((sums[1] == L - 1).all()) and bool((gcond != -7.0).all())
