"""-m gpu: the front-end and VQ gradient entries (``vqcpc_encoder_front_fwd`` / ``_bwd``, ``vqcpc_encoder_vq_bwd``) on a caller's
stream -- the stream contract of ``include/vqcpc.h`` (*all work is enqueued on `stream`; no call synchronises*), held with
tests/stream_harness.py exactly as tests/test_gpu_stream_contract.py holds the other entries.  That file keeps the one table of
entries against the header; its rows name the tests here.  All three: does not synchronise (``busy`` is asserted).
"""

import pytest
import torch

import front_grad_ref as R
import stream_harness as H
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def release_what_this_file_holds():
    """The cases, the float64 references and the device buffers of this file are released when it is done, and the stream harness's
    session-wide delay chain and report are left as they were found (``stream_harness.release_after`` says why)."""
    yield from H.release_after(R._cases, R._fwd, R._refs)


def encoder():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict(ln_affine="random", codebook="data"))
    return enc.cuda().eval()


def test_front_fwd_bwd_weights_in_stream_order():
    """fwd then bwd back to back on ``s``; the mel, the 17 front-end tensors and the upstream gradient are all written on ``s``
    behind the delay: the conv weight's two k orders and every transpose must be made from what the stream holds when the call's
    turn comes."""
    g = R.load("partial_tile")
    enc = encoder()
    true = [g["mel"].cuda()] + [g["w"][k].cuda() for k in R.KEYS] + [g["G"].cuda()]
    other = synth.encoder_state_dict(seed=99, ln_affine="random")
    decoy = [synth.mel("front_grad/sc_decoy", g["B"], g["T"]).cuda()] + [other[n].cuda() for n in R.SD_NAMES] + \
            [R._u("sc_decoy/G", tuple(g["G"].shape), 1.0).cuda()]

    def entry(mel, *rest):
        ws, G = list(rest[:17]), rest[17]
        z_pre, saved = enc._front_fwd(mel, ws)
        return [z_pre, saved] + enc._front_bwd(mel, saved, G, ws)

    H.hold(entry, true, decoy, label="front_fwd + front_bwd partial_tile")


def test_vq_bwd():
    enc = encoder()
    shape = (3, 21, 64)
    names = ("z_pre", "z_q", "grad_z_st", "grad_loss")
    true = [R._u("sc/vq/" + n, shape if n != "grad_loss" else (1,), 1.0).cuda() for n in names]
    decoy = [R._u("sc/vq_decoy/" + n, shape if n != "grad_loss" else (1,), 1.0).cuda() for n in names]

    def entry(z_pre, z_q, gs, gl):
        return [vq_bwd(enc, z_pre, z_q, gs, gl), vq_bwd(enc, z_pre, z_q, None, gl), vq_bwd(enc, z_pre, z_q, gs, None)]

    H.hold(entry, true, decoy, label="vq_bwd 63 rows")


def vq_bwd(enc, z_pre, z_q, gs, gl):
    from vectorquantizedcpc_amd import _lib
    out = torch.empty_like(z_pre)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.load().vqcpc_encoder_vq_bwd(enc._native(), z_pre.data_ptr(), z_q.data_ptr(), z_pre.numel() // 64, ptr(gs), ptr(gl),
                                                out.data_ptr(), _lib.current_stream()))
    return out
