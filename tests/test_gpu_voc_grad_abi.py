"""-m gpu: every ``VQCPC_ERR_INVALID`` condition of ``include/vqcpc.h`` through raw ctypes: the call returns -1 with a
message that names the condition, and nothing is enqueued -- the outputs keep the pattern they were filled with."""
import ctypes

import pytest
import torch

import voc_grad_ref as R
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib

pytestmark = pytest.mark.gpu

INVALID = -1


def vocoder(c, hf=256):
    voc = V.Vocoder(V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(dim_voc_latent=c["C"], upsampling_t=c["up"], wave_ar=V.ConfWaveAR(
        size_i_embed_ar=c["de"], size_h_rnn=c["Hr"], size_h_fc=hf))))
    if hf == 256:
        voc.load_state_dict(c["sd"])
    return voc.cuda().eval()


def test_abi_errors_enqueue_nothing():
    c = R.load("h512")
    voc = vocoder(c)
    lib, h, s = _lib.load(), voc._native(), _lib.current_stream()
    B, Tc, L, Hr, C = c["B"], c["Tc"], c["L"], c["Hr"], c["C"]
    audio, z, spk = c["audio"].cuda(), c["z"].cuda(), c["spk"].cuda()
    n = ctypes.c_uint64()
    assert lib.vqcpc_vocoder_ar_saved_bytes(h, B, L, ctypes.byref(n)) == 0 and n.value % 16 == 0 and n.value >= B * (L - 1) * Hr * 4
    assert lib.vqcpc_vocoder_ar_saved_bytes(h, 0, L, ctypes.byref(n)) == INVALID and lib.vqcpc_vocoder_ar_saved_bytes(h, B, 0, ctypes.byref(n)) == INVALID
    assert lib.vqcpc_vocoder_ar_saved_bytes(None, B, L, ctypes.byref(n)) == INVALID and lib.vqcpc_vocoder_ar_saved_bytes(h, B, L, None) == INVALID
    assert lib.vqcpc_vocoder_ar_saved_bytes(h, B, L, ctypes.byref(n)) == 0
    saved = torch.full((n.value // 4,), -7.0, device="cuda")
    sums = [torch.full((B,), -7.0, dtype=torch.float64, device="cuda"), torch.full((B,), -7, dtype=torch.int64, device="cuda"),
            torch.full((B,), -7, dtype=torch.int64, device="cuda")]
    cond = torch.full((B, 2 * Tc, C), -7.0, device="cuda")
    ws = [p.detach().contiguous() for p in voc._ar_params()]
    outs = [torch.full_like(w, -7.0) for w in ws]
    gcond = torch.full((B, 2 * Tc, C), -7.0, device="cuda")
    gl = torch.tensor(1.0, device="cuda")
    ints = lambda v: None if v is None else (ctypes.c_int * len(v))(*v)
    ptr = lambda t: None if t is None else t.data_ptr()

    def struct(ts):
        if ts is None:
            return None
        st = _lib.VocoderArTensors()
        for k, t in zip(voc.AR_KEYS, ts):
            setattr(st, k, t if isinstance(t, int) or t is None else t.data_ptr())
        return st

    def fwd(h=h, audio=audio.data_ptr(), z=z.data_ptr(), spk=spk.data_ptr(), B=B, Tc=Tc, L=L, nc=None, na=None, w=ws, sums=sums,
            cond=cond.data_ptr(), saved=saved.data_ptr()):
        return lib.vqcpc_vocoder_ar_fwd(h, audio, z, spk, B, Tc, L, ints(nc), ints(na), struct(w), *[ptr(t) for t in sums], cond, saved, s)

    def bwd(h=h, audio=audio.data_ptr(), z=z.data_ptr(), spk=spk.data_ptr(), B=B, Tc=Tc, L=L, nc=None, na=None, w=ws, saved=saved.data_ptr(),
            gl=gl.data_ptr(), outs=outs, gcond=gcond.data_ptr()):
        return lib.vqcpc_vocoder_ar_bwd(h, audio, z, spk, B, Tc, L, ints(nc), ints(na), struct(w), saved, gl, struct(outs), gcond, s)

    err = lib.vqcpc_last_error
    for call in (fwd, bwd):
        # the NULL and range conditions of vqcpc_vocoder_nll
        assert call(h=None) == INVALID and call(audio=None) == INVALID and call(z=None) == INVALID and call(spk=None) == INVALID
        assert b"null argument" in err()
        assert call(B=0) == INVALID and call(Tc=0) == INVALID and call(L=0) == INVALID and b"need B > 0" in err()
        assert call(na=[L + 1] * B) == INVALID and b"n_audio" in err()
        assert call(na=[-1] * B) == INVALID
        assert call(nc=[Tc + 1] * B) == INVALID and b"n_codes" in err()
        assert call(nc=[1] * B) == INVALID and b"samples to score" in err()           # L - 1 = 80 steps, one code covers 16
        # a NULL saved, a NULL member of *w, misaligned pointers
        assert call(saved=None) == INVALID and b"null argument" in err()
        assert call(saved=saved.data_ptr() + 4) == INVALID and b"16-byte aligned" in err()
        for i in range(9):
            assert call(w=ws[:i] + [None] + ws[i + 1:]) == INVALID and b"all nine tensors" in err(), i
        assert call(w=[ws[0].data_ptr() + 4] + ws[1:]) == INVALID and b"16-byte aligned" in err()
        if torch.cuda.device_count() > 1:
            with torch.cuda.device(1):
                assert call() == INVALID and b"belongs to device" in err()
    assert fwd(sums=[None] + sums[1:]) == INVALID and fwd(sums=sums[:2] + [None]) == INVALID and b"null argument" in err()
    assert fwd(cond=cond.data_ptr() + 4) == INVALID and b"16-byte aligned" in err()
    # the backward alone: no wanted output, N == 0, misaligned outputs
    assert bwd(outs=None, gcond=None) == INVALID and b"no wanted output" in err()
    assert bwd(outs=[None] * 9, gcond=None) == INVALID and b"no wanted output" in err()
    assert bwd(na=[1] * B) == INVALID and b"N = 0" in err()
    assert bwd(na=[0] * B) == INVALID and b"N = 0" in err()
    assert bwd(outs=[outs[0].data_ptr() + 4] + [None] * 8) == INVALID and b"16-byte aligned" in err()
    assert bwd(gcond=gcond.data_ptr() + 4) == INVALID and b"16-byte aligned" in err()
    torch.cuda.synchronize()
    for t in [saved, cond, gcond] + sums + outs:
        assert bool((t == -7).all())
    # the same calls, valid: everything wanted is written
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    voc.check()
    assert bool((sums[1] == L - 1).all()) and bool((cond != -7.0).all()) and bool((gcond != -7.0).all())
    assert all(bool((o != -7.0).all()) for o in outs)
    assert fwd(w=None, cond=None) == 0 and bwd(w=None, gl=None, outs=None) == 0 and bwd(outs=[None] * 8 + [outs[8]], gcond=None) == 0
    assert fwd(na=[1] * B) == 0                                       # nothing to score is a valid forward: sums of zero
    torch.cuda.synchronize()
    voc.check()
    assert bool((sums[1] == 0).all()) and bool((sums[0] == 0).all())


def test_sizes_the_scoring_head_does_not_take():
    c = R.load("h512")
    voc = vocoder(c, hf=512)
    lib, h = _lib.load(), voc._native()
    n = ctypes.c_uint64()
    assert lib.vqcpc_vocoder_ar_saved_bytes(h, 2, 81, ctypes.byref(n)) == INVALID and b"size_h_fc 256" in lib.vqcpc_last_error()
    z, spk, audio = c["z"].cuda(), c["spk"].cuda(), c["audio"].cuda()
    with pytest.raises(RuntimeError, match="size_h_fc 256"):
        voc.ar_gradients(audio, z, spk)
    with pytest.raises(RuntimeError, match="size_h_fc 256"):
        voc.nll(audio, z, spk, differentiable=True)
