"""-m gpu: ``vqcpc_vocoder_cond_fwd`` / ``_bwd`` and ``vqcpc_vocoder_ar_fwd_cond`` / ``_bwd_cond`` on a caller's stream -- the stream
contract of ``include/vqcpc.h`` (*all work is enqueued on `stream`; no call synchronises*), held with tests/stream_harness.py exactly
as tests/test_gpu_stream_contract.py holds the other entries.  That file keeps the one table of entries against the header; its
rows name the tests here.

All four: does not synchronise (``busy`` is asserted).  A backward behind a forward of the same handle may wait for the staging arena of
the forward's uploads, so each pair is probed after its first call and the backward is held on its own as well.  The eighteen
tensors of the conditioning path are among the buffers written behind the delay: the per-call re-layout (the stacked w_ih / b_ih /
b_hh and the W_hh fragments) must be made from what the stream holds when the call's turn comes.
"""

import pytest
import torch

import cond_grad_ref as R
import stream_harness as H
import voc_grad_ref as VR
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu

CASE = "ragged"


@pytest.fixture(scope="module", autouse=True)
def release_what_this_file_holds():
    """The cases, the references and the device buffers of this file are released when it is done, and the stream harness's
    session-wide delay chain and report are left as they were found (``stream_harness.release_after`` says why)."""
    yield from H.release_after()


def cond_setup():
    """The vocoder of the case, and its true and decoy inputs: z, speaker, the upstream gradient, the eighteen tensors."""
    c = R.load(CASE)
    voc = V.Vocoder(V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(wave_ar=V.ConfWaveAR(size_h_rnn=512))))
    voc.load_state_dict(c["sd"])
    voc = voc.cuda().eval()
    B, Tc = c["B"], c["Tc"]
    true = [c["z"].cuda(), c["spk"].cuda(), c["G"].cuda()] + [p.detach().clone() for p in voc._cond_params()]
    other = synth.vocoder_state_dict(seed=99, size_h_rnn=512)
    decoy = [synth.randint("cond_grad/sc_decoy/z", (B, Tc), R.N_CODES).cuda(), synth.randint("cond_grad/sc_decoy/s", (B,), R.N_SPK).cuda(),
             -0.5 * c["G"].cuda()] + [other[k].cuda() for k in R.KEYS]
    nc = V._lib.int_array(c["n_codes"], B, "n_codes")
    return c, voc, true, decoy, nc


def test_cond_fwd_then_bwd_weights_in_stream_order():
    c, voc, true, decoy, nc = cond_setup()

    def entry(z, spk, G, *ws):
        cond, saved = voc._cond_fwd(z, spk, nc, list(ws))
        busy = H.probe()
        grads = voc._cond_bwd(z, spk, nc, saved, G, list(ws))
        return H.Early([cond] + grads, busy)

    H.hold(entry, true, decoy, label="cond_fwd + cond_bwd " + CASE)


def test_cond_bwd_alone():
    """The backward as the first call on ``s``, with ``saved`` among the buffers written behind the delay."""
    c, voc, true, decoy, nc = cond_setup()

    def saved_of(inputs):
        return torch.nan_to_num(voc._cond_fwd(inputs[0], inputs[1], nc, list(inputs[3:]))[1])    # rows past the frames are never read: any finite value

    true, decoy = true + [saved_of(true)], decoy + [saved_of(decoy)]
    torch.cuda.synchronize()

    def entry(z, spk, G, *rest):
        return voc._cond_bwd(z, spk, nc, rest[18], G, list(rest[:18]))

    H.hold(entry, true, decoy, label="cond_bwd " + CASE)


def ar_setup():
    """The vocoder of tests/voc_grad_ref.py's case, and its true and decoy inputs: audio, the conditioning series, the nine tensors."""
    c = VR.load(CASE)
    voc = V.Vocoder(V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(dim_voc_latent=c["C"], upsampling_t=c["up"],
                                                           wave_ar=V.ConfWaveAR(size_i_embed_ar=c["de"], size_h_rnn=c["Hr"]))))
    voc.load_state_dict(c["sd"])
    voc = voc.cuda().eval()
    B, Tc, L = c["B"], c["Tc"], c["L"]
    z, spk = c["z"].cuda(), c["spk"].cuda()
    cond = voc._cond_fwd(z, spk, V._lib.int_array(c["n_codes"], B, "n_codes"), None)[0]
    true = [c["audio"].cuda(), cond] + [p.detach().clone() for p in voc._ar_params()]
    other = synth.vocoder_state_dict(seed=99, dim_voc_latent=c["C"], size_i_embed_ar=c["de"], size_h_rnn=c["Hr"])
    decoy = [synth.randint("cond_grad/sc_decoy/a", (B, L), 256).cuda(), -0.5 * cond] + [other["rnnms.ar." + n].cuda() for n in VR.SD_NAMES]
    torch.cuda.synchronize()
    return c, voc, z, spk, true, decoy


def test_ar_fwd_cond_then_bwd_cond():
    c, voc, z, spk, true, decoy = ar_setup()

    def entry(audio, cond, *ws):
        call = voc._nll_call(audio, z, spk, c["lengths"], c["n_codes"])
        nll_sum, n_scored, n_correct, out, saved = voc._ar_fwd(call, list(ws), want_cond=True, cond_in=cond)
        busy = H.probe()
        grads, gc = voc._ar_bwd(call, saved, list(ws), cond_grad=True, cond_in=cond)
        return H.Early([nll_sum, n_scored, n_correct, out] + grads + [gc], busy)

    H.hold(entry, true, decoy, label="ar_fwd_cond + ar_bwd_cond " + CASE)


def test_ar_bwd_cond_alone():
    c, voc, z, spk, true, decoy = ar_setup()

    def saved_of(inputs):
        call = voc._nll_call(inputs[0], z, spk, c["lengths"], c["n_codes"])
        return torch.nan_to_num(voc._ar_fwd(call, list(inputs[2:11]), cond_in=inputs[1])[4])

    true, decoy = true + [saved_of(true)], decoy + [saved_of(decoy)]
    torch.cuda.synchronize()

    def entry(audio, cond, *rest):
        call = voc._nll_call(audio, z, spk, c["lengths"], c["n_codes"])
        grads, gc = voc._ar_bwd(call, rest[9], list(rest[:9]), cond_grad=True, cond_in=cond)
        return grads + [gc]

    H.hold(entry, true, decoy, label="ar_bwd_cond " + CASE)
