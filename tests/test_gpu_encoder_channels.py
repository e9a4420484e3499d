"""-m gpu: the encoder front end at channel counts other than the reference's 80.

Every other encoder test builds ``ConfEncoder(80, ...)``, which leaves the generic paths of the three front-end
schedules unrun: a conv weight slice of other than 20 q-steps (C = 16 has 4), the remainder loop of the column-split
conv gather and the generic chain fold (C = 96), the edge of the staged mel window (C = 128) and the channel counts
only the layered kernels take (C = 144: 4 C > 512).  Two mel shapes: (3, 14) is 21 rows whose first 16-row tile
straddles utterances (the gather path); (1, 66) is 33 rows, two whole-utterance tiles (the LDS-window path) and a
ragged one.

At C != 80 the reference's own K-blocking of the convolution is not pinned by any fixture: what this test pins is
this project's three schedules to its C oracle (explicit conv_mode 1 and 2) and to each other, bit for bit.  The
oracle's argmin margins for these exact inputs are far from ties (smallest d_second - d_best seen: 0.0019 at C = 96,
(1, 66)), so an index mismatch is a real one.
"""
import numpy as np
import pytest
import torch

import oracle
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu

_models = {}


def encoder_for(C):
    if C not in _models:
        sd = synth.encoder_state_dict(in_channels=C, ln_affine="random", codebook="data")
        enc = V.Encoder(V.ConfEncoder(C, 512, 512, 64, 256))
        enc.load_state_dict(sd)
        _models[C] = (enc.cuda().eval(), sd)
    return _models[C]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("shape", [(3, 14), (1, 66)])
@pytest.mark.parametrize("C", [16, 96, 128, 144])
def test_three_schedules_match_oracle_at_other_channel_counts(C, shape):
    enc, sd = encoder_for(C)
    B, T = shape
    mel = synth.mel("ch%d" % C, B, T, n_mels=C)
    melc = mel.cuda()
    schedules = (0, 1, 2) if C <= 128 else (0,)
    try:
        if C > 128:
            with pytest.raises(RuntimeError):
                enc.set_option("fused", 1)
        for mode in (1, 2):
            conv = oracle.conv1d_k4s2(mel.numpy(), sd["conv.weight"].numpy(), mode=mode)
            want = oracle.encoder_encode(sd, mel.numpy(), want_c=False, conv_mode=mode)
            margin = float((want["d_second"] - want["d_best"]).min())
            print("C=%d %s mode %d: smallest argmin margin %.6f" % (C, shape, mode, margin))
            stages = {}
            for fused in schedules:
                enc.set_option("fused", fused)
                z, _, idx = enc.encode(melc, conv_mode=mode)
                st = [enc.stage(melc, s, conv_mode=mode).cpu().numpy() for s in range(11)]
                stages[fused] = st
                tag = (C, shape, mode, fused)
                assert np.array_equal(bits(st[0]), bits(conv)), tag
                assert np.array_equal(bits(st[10]), bits(want["z_pre"])), tag
                assert np.array_equal(idx.cpu().numpy(), want["indices"]), tag
                assert np.array_equal(bits(z.cpu().numpy()), bits(want["z"])), tag
            for fused in schedules[1:]:
                for s in range(1, 10):
                    assert np.array_equal(bits(stages[fused][s]), bits(stages[0][s])), (C, shape, mode, fused, s)
    finally:
        enc.set_option("fused", -1)
