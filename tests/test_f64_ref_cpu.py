"""CPU checks of oracle/f64_ref.py, the float64 vocoder reference that tests/test_gpu_vocoder_f64.py judges the GPU against.

1. f64 against the C oracle (fp32) on both weight sets: conditioning and teacher-forced logits over 480 steps (three
   conditioning frames).  Measured: conditioning 3.5e-7 / 1.4e-6, logits 1.7e-7 / 1.1e-5 (default / stressed).
2. torch_ref (fp32) against f64 over 6 400 steps of the stressed set: 7.3e-6, flat over the windows (the last
   1 600-sample window no worse than 2x the first).  This is the fp32 deviation the GPU tolerances are set from (about 10x).
3. A ragged batch is its utterances run one at a time (1e-12).
4. Seeded faults, built here on torch_ref's output, are rejected by the comparators, and unperturbed torch_ref passes:
   conditioning frame f + 1 used from sample 16 000 on; one gate value off by 1e-4 on every step; a ragged utterance
   conditioned on the padded length.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import f64_ref, torch_ref
from vectorquantizedcpc_amd import synth

SEED = 13
# GPU tolerances of tests/test_gpu_vocoder_f64.py (logits), applied to fp32 torch_ref here
TOL = {"default": 1e-6, "stressed": 5e-5}
_cache = {}


def weights(name):
    if name not in _cache:
        sd = synth.vocoder_state_dict()
        _cache[name] = sd if name == "default" else f64_ref.stressed(sd)
    return _cache[name]


def ref(name):
    key = "f64/" + name
    if key not in _cache:
        _cache[key] = f64_ref.F64Vocoder(weights(name))
    return _cache[key]


@pytest.mark.parametrize("name,cond_tol,logit_tol", [("default", 1e-6, 1e-6), ("stressed", 1e-5, 5e-5)])
def test_f64_against_the_c_oracle(name, cond_tol, logit_tol):
    sd, f = weights(name), ref(name)
    z = synth.randint("f64c/z", (2, 3), 512)
    spk = synth.randint("f64c/s", (2,), 102)
    x = synth.randint("f64c/x", (2, 480), 256)
    cond = f.condition(z, spk)
    lg = f.logits(x, cond).numpy()
    ce = le = 0.0
    for b in range(2):
        ce = max(ce, float(np.abs(oracle.vocoder_condition(sd, z[b].numpy(), int(spk[b])) - cond[b].numpy()).max()))
        r = oracle.vocoder_generate(sd, z[b].numpy(), int(spk[b]), seed=0, n_steps=480, inputs=x[b].numpy(), want_logits=True)
        le = max(le, float(np.abs(r["logits"] - lg[b]).max()))
    print(f"{name}: |C oracle - f64| conditioning {ce:.3g}, logits {le:.3g}")
    assert ce <= cond_tol and le <= logit_tol


def _torch_run(sd, z, spk, n, cond=None, inputs=None, cell=None, utt_base=0):
    """torch_ref fp32 free run (or teacher-forced on `inputs`): (samples, logits); `cell` replaces its GRU cell."""
    tv = torch_ref.TorchVocoder(sd)
    if cell is not None:
        tv.cell = cell(tv.cell)
    s, _, lg = tv.generate(z, spk, seed=SEED, utt_base=utt_base, n_steps=n, inputs=inputs, want_logits=True, cond=cond)
    return s.numpy(), lg.numpy()


def _judge(name, samples, logits, cond, lengths=None, utt_base=0):
    """Both comparators on torch_ref output: (logit error, per-window errors, draw check) against f64 on its history."""
    B, n = samples.shape
    x = np.concatenate([np.full((B, 1), 128), samples[:, :-1]], axis=1)
    want = ref(name).logits(x, cond, lengths).numpy()
    err, per = f64_ref.logit_error(logits, want, lengths)
    draws = f64_ref.check_draws(samples, want, SEED, list(range(utt_base, utt_base + B)), lengths, TOL[name])
    return err, per, draws


def test_torch_fp32_stays_near_f64_over_6400_steps_stressed():
    z = synth.randint("f64t/z", (4, 20), 512)
    spk = synth.randint("f64t/s", (4,), 102)
    s, lg = _torch_run(weights("stressed"), z, spk, 6400)
    err, per, (exact, worst, bad, first) = _judge("stressed", s, lg, ref("stressed").condition(z, spk))
    print("stressed, |torch fp32 - f64| logits %.3g, by window %s; draws exact %.5f, worst gap %.3g" % (err, per, exact, worst))
    assert err <= 1.5e-5 and per[-1] <= 2.0 * per[0]
    assert bad == 0 and exact >= 0.999


def test_ragged_batch_equals_utterances_alone():
    f = ref("stressed")
    z = synth.randint("f64r/z", (3, 5), 512)
    spk = synth.randint("f64r/s", (3,), 102)
    n_codes = [5, 2, 3]
    cond = f.condition(z, spk, n_codes)
    x = synth.randint("f64r/x", (3, 1000), 256)
    lengths = [320 * n for n in n_codes]
    lg = f.logits(x, cond, [min(n, 1000) for n in lengths]).numpy()
    for b in range(3):
        one = f.condition(z[b:b + 1, : n_codes[b]], spk[b:b + 1])[0]
        assert one.shape == cond[b].shape and float((one - cond[b]).abs().max()) <= 1e-12
        n = min(lengths[b], 1000)
        lg1 = f.logits(x[b:b + 1, :n], [one]).numpy()
        assert float(np.abs(lg1[0] - lg[b, :n]).max()) <= 1e-12
        assert not lg[b, n:].any()


# ---------------------------------------------------------------------- seeded faults
def test_unperturbed_and_late_frame_shift_default():
    """Conditioning frame f + 1 used for every t >= 16 000 (frame 100 on): caught, and only in the windows from 16 000 on."""
    name = "default"
    sd = weights(name)
    z = synth.randint("f64f/z", (1, 51), 512)
    spk = synth.randint("f64f/s", (1,), 102)
    cond = ref(name).condition(z, spk)
    c32 = torch_ref.TorchVocoder(sd).condition(z, spk)
    n = 16320
    s, lg = _torch_run(sd, z, spk, n, cond=c32)
    err, per, (exact, worst, bad, _) = _judge(name, s, lg, cond)
    print("unperturbed torch fp32: logits %.3g, draws exact %.5f, worst gap %.3g" % (err, exact, worst))
    assert err <= TOL[name] and bad == 0
    shifted = c32.clone()
    shifted[:, 100:-1] = c32[:, 101:]
    s, lg = _torch_run(sd, z, spk, n, cond=shifted)
    err, per, (exact, worst, bad, first) = _judge(name, s, lg, cond)
    print("frame shift from 16 000: logits %.3g (by window %s), draws outside the window %d, first %s" % (err, per, bad, first))
    assert err > TOL[name] and bad > 0
    assert per[:10].max() <= TOL[name] and first[1] >= 16000


class _GatePerturbed(torch.nn.Module):
    """The fp32 GRU cell with the candidate gate n of hidden unit 0 off by `eps` on every step."""

    def __init__(self, cell, eps=1e-4):
        super().__init__()
        self.cell, self.eps = cell, eps

    def forward(self, inp, h):
        c = self.cell
        gi = F.linear(inp, c.weight_ih, c.bias_ih)
        gh = F.linear(h, c.weight_hh, c.bias_hh)
        H = h.shape[1]
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        u = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        n[:, 0] += self.eps
        return (1 - u) * n + u * h


@pytest.mark.parametrize("name", ["default", "stressed"])
def test_gate_off_by_1e4_is_caught(name):
    """The logits catch it on both weight sets (measured 3.9e-6 against 1e-6, 6.5e-5 against 5e-5).  A logit error this small
    flips no draw in 3 200 steps (draws flip at about one per thousand from a 1e-3 logit error): the draw check alone would miss
    it, which is why the GPU tests compare teacher-forced logits at full length as well."""
    sd = weights(name)
    z = synth.randint("f64g/z", (2, 5), 512)
    spk = synth.randint("f64g/s", (2,), 102)
    cond = ref(name).condition(z, spk)
    s, lg = _torch_run(sd, z, spk, 1600, cell=_GatePerturbed)
    err, per, (exact, worst, bad, first) = _judge(name, s, lg, cond)
    print("%s, gate n[0] + 1e-4: logits %.3g, draws outside the window %d, exact %.5f" % (name, err, bad, exact))
    assert err > TOL[name]


def test_ragged_utterance_conditioned_on_the_padded_length():
    name = "default"
    sd = weights(name)
    z = synth.randint("f64p/z", (2, 6), 512)
    spk = synth.randint("f64p/s", (2,), 102)
    n_codes = [6, 3]
    cond = ref(name).condition(z, spk, n_codes)
    padded = torch_ref.TorchVocoder(sd).condition(z, spk)          # the backward GRUs start at the padded end
    n = 960
    s, lg = _torch_run(sd, z[1:], spk[1:], n, cond=padded[1:, :6], utt_base=1)
    err, per, (exact, worst, bad, first) = _judge(name, s, lg, cond[1:], utt_base=1)
    print("ragged row on the padded length: logits %.3g, draws outside the window %d" % (err, bad))
    assert err > TOL[name] and bad > 0
    proper = torch_ref.TorchVocoder(sd).condition(z[1:, :3], spk[1:])
    s, lg = _torch_run(sd, z[1:, :3], spk[1:], n, cond=proper, utt_base=1)
    err, per, (exact, worst, bad, first) = _judge(name, s, lg, cond[1:], utt_base=1)
    assert err <= TOL[name] and bad == 0
