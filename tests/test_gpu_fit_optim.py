"""-m gpu: the fits with ``optimizer=optim.Adam``, ``scheduler=`` and ``opt_state=`` -- ``driver.fit_predictors``, ``fit_context`` and
``fit_encoder`` on two batches of 2 x 2 synthetic utterances and ``driver.fit_vocoder`` on the six utterances of
tests/voc_fit_ref.py, a few steps each.

* Losses.  The fits run twice, with ``optim.Adam`` and with ``torch.optim.Adam``.  The two optimizers are each within the judge of
  float64 Adam per update, ``4 * 2^-24 * max |p|`` at the least, so after k updates their parameters may stand
  ``2 k 4 2^-24 max |p|`` apart; to first order that moves the loss by at most ``||g||_1`` times as much.  With that as ``e_ref``
  the gradient tests' rule for step k + 1 reads ``|L_hip - L_torch| <= 4 max(e_ref, 2^-24 |L|)``.  ``||g||_1`` and ``max |p|`` are
  read off the recorded gradients and the start parameters; the first loss (no update yet) must be equal bit for bit.
  ``fit_encoder`` is held to the first loss only: its front end moves under the codebook, a parameter difference of one ulp can
  move a frame to another code, and past that the loss is not smooth in the parameters -- no first-order bound holds.  Its
  optimizer is judged by the final parameters alone.
* Final parameters.  Every step's HIP gradients are recorded by the optimizer subclass below; ``torch.optim.Adam`` in float64 on
  the CPU is fed them from the same start, the fp32 run of the same gives ``e_ref``, tests/grad_judge.py judges.
* The schedule: ``group["lr"]`` at every ``step()`` against tests/golden/warmup_lrs.json.
* A fit of 2n steps equals, bit for bit, two fits of n steps joined by ``opt_state``.
* ``cli.main`` with ``--optimizer hip --optimizer-state``: written, then read.
"""
import json
import os

import numpy as np
import pytest
import torch

import adam_ref as A
import voc_fit_ref as F
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import cli, driver, optim, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24


def recording(base, log):
    """``base`` with a ``step()`` that first appends (``group["lr"]``, the gradients as float64 CPU tensors) to ``log``."""
    class Recording(base):
        def step(self, closure=None):
            log.append((self.param_groups[0]["lr"], [None if p.grad is None else p.grad.detach().double().cpu() for p in self.param_groups[0]["params"]]))
            return super().step(closure)
    return Recording


def golden_lrs(name="example"):
    with open(os.path.join(ROOT, "tests", "golden", "warmup_lrs.json")) as f:
        case = json.load(f)["cases"][name]
    return case["args"], dict(zip(case["epochs"], case["lrs"]))


# ------------------------------------------------------------------ the small fits
def cpc_models():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict(ln_affine="random", codebook="data"))
    cpc = V.CPCLoss(V.ConfCPC(4, 2, 2, 3, 64, 256))
    cpc.load_state_dict(synth.cpc_state_dict(n_prediction_steps=4))
    by_speaker = {f"S{s}": [synth.mel(f"fit_optim/S{s}_{u}", 1, 44)[0] for u in "ab"] for s in (1, 2, 3, 4)}
    return enc.cuda().eval(), cpc.cuda().eval(), by_speaker


def fit_predictors(optimizer, steps, **kw):
    enc, cpc, by_speaker = cpc_models()
    params = driver._predictor_params(cpc)
    start = [p.detach().cpu().clone() for p in params]
    r = driver.fit_predictors(enc, cpc, by_speaker, steps=steps, lr=1e-3, optimizer=optimizer, sample_frames=16, **kw)
    assert r["steps"] == steps and r["batches"] == 2
    return r, start, [p.detach().cpu().clone() for p in params]


def fit_context(optimizer, steps, load=None, **kw):
    """The front end and the codebook are frozen here, so the loss is smooth in the parameters that step."""
    enc, cpc, by_speaker = cpc_models()
    if load is not None:
        enc.load_state_dict(load[0])
        cpc.load_state_dict(load[1])
    params = list(enc.rnn.parameters()) + driver._predictor_params(cpc)
    start = [p.detach().cpu().clone() for p in params]
    r = driver.fit_context(enc, cpc, by_speaker, steps=steps, lr=1e-3, optimizer=optimizer, sample_frames=16, **kw)
    assert r["steps"] == steps and r["batches"] == 2
    r["models"] = (enc, cpc)
    return r, start, [p.detach().cpu().clone() for p in params]


def encoder_parts(enc, cpc):
    return {"front": list(enc.conv.parameters()) + list(enc.encoder.parameters()), "rnn": list(enc.rnn.parameters()),
            "predictors": driver._predictor_params(cpc)}


def fit_encoder(optimizer, steps, load=None, train=driver.FIT_ENCODER_PARTS, **kw):
    """The whole training step: the front end, the LSTM and the predictors the loss reads under one optimizer (25 tensors at this
    model's two predictors, 33 at the reference's six), the codebook adapting under them."""
    enc, cpc, by_speaker = cpc_models()
    if load is not None:
        enc.load_state_dict(load[0])
        cpc.load_state_dict(load[1])
    parts = encoder_parts(enc, cpc)
    params = [p for name in driver.FIT_ENCODER_PARTS if name in train for p in parts[name]]
    assert len(params) == 25 or tuple(train) != driver.FIT_ENCODER_PARTS
    start = [p.detach().cpu().clone() for p in params]
    r = driver.fit_encoder(enc, cpc, by_speaker, steps=steps, lr=1e-3, optimizer=optimizer, sample_frames=16, train=train, **kw)
    assert r["steps"] == steps and r["batches"] == 2
    r["models"] = (enc, cpc)
    return r, start, [p.detach().cpu().clone() for p in params]


def voc_models():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict())
    voc = V.Vocoder(V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(wave_ar=V.ConfWaveAR(size_h_rnn=F.HR))))
    voc.load_state_dict(F.vocoder_state_dict())
    return enc.cuda().eval(), voc.cuda().eval()


def fit_vocoder(optimizer, steps, **kw):
    enc, voc = voc_models()
    params = voc._part_params("ar")
    start = [p.detach().cpu().clone() for p in params]
    r = driver.fit_vocoder(enc, voc, F.waves(), None, F.speakers(), steps=steps, lr=F.LR, optimizer=optimizer, max_batch=F.MAX_BATCH,
                           clip_codes=F.CLIP, seed=F.SEED, **kw)
    assert r["steps"] == steps and r["batches"] == 2
    return r, start, [p.detach().cpu().clone() for p in params]


def check_losses(what, hip, ref, log, start):
    top = max(float(p.abs().max()) for p in start)
    assert hip[0] == ref[0], (what, hip[0], ref[0])                      # no update yet: the same kernels on the same bits
    bad = []
    for k in range(1, len(hip)):
        g1 = sum(float(g.abs().sum()) for g in log[k][1] if g is not None)
        e_ref = g1 * 2 * k * 4 * U32 * top
        bound = 4 * max(e_ref, U32 * abs(ref[k]))
        diff = abs(hip[k] - ref[k])
        print(f"{what} step {k}: loss {hip[k]:.9g} (optim.Adam) {ref[k]:.9g} (torch.optim.Adam), |difference| {diff:.3g}, ||g||_1 {g1:.3g}, "
              f"max|p| {top:.3g}, e_ref {e_ref:.3g}, bound {bound:.3g}, ratio {diff / bound:.3f}")
        if not diff <= bound:
            bad.append((k, diff, bound))
    assert not bad, bad


def check_final_parameters(what, start, final, log, lr):
    """float64 (and, for ``e_ref``, fp32) ``torch.optim.Adam`` on the CPU, fed the recorded gradients from the same start."""
    def run(dtype):
        ps = [torch.nn.Parameter(p.to(dtype)) for p in start]
        opt = torch.optim.Adam(ps, lr=lr)
        for step_lr, grads in log:
            opt.param_groups[0]["lr"] = step_lr
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.to(dtype)
            opt.step()
        return {"p": [p.detach().numpy() for p in ps]}

    ratio = A.judge_snapshot(what, len(log), {"p": [p.numpy() for p in final]}, run(torch.float64), run(torch.float32), what, KEYS=("p",))
    assert ratio <= 1.0
    assert any(not torch.equal(a, b) for a, b in zip(start, final))


@pytest.mark.parametrize("fit,steps,lr", [(fit_predictors, 5, 1e-3), (fit_vocoder, 4, F.LR), (fit_context, 4, 1e-3), (fit_encoder, 4, 1e-3)],
                         ids=["fit_predictors", "fit_vocoder", "fit_context", "fit_encoder"])
def test_fit_with_the_hip_step_follows_torchs_and_float64(fit, steps, lr):
    log = []
    hip, start, final = fit(recording(optim.Adam, log), steps)
    ref, start_ref, _ = fit(torch.optim.Adam, steps)
    assert all(torch.equal(a, b) for a, b in zip(start, start_ref)) and len(log) == steps
    if fit is fit_encoder:
        # not check_losses: its first-order bound needs a loss that is smooth in the parameters, and here a parameter difference of
        # one ulp between the two optimizers can move a frame to another code.  The first loss has no update behind it.
        assert hip["losses"][0] == ref["losses"][0], (hip["losses"][0], ref["losses"][0])
        assert all(g is not None for g in log[-1][1]) and len(log[-1][1]) == 25
    else:
        check_losses(fit.__name__, hip["losses"], ref["losses"], log, start)
    check_final_parameters(fit.__name__, start, final, log, lr)


def test_fit_encoder_leaves_an_untrained_part_alone():
    """``train=("front", "predictors")``: the context LSTM keeps its bits, is in no param group and has no optimizer state."""
    made = []

    class Kept(optim.Adam):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    state = {}
    r, start, final = fit_encoder(Kept, 2, train=("front", "predictors"), opt_state=state)
    enc, cpc = r["models"]
    fresh_enc, fresh_cpc, _ = cpc_models()
    rnn, rnn_before = encoder_parts(enc, cpc)["rnn"], encoder_parts(fresh_enc, fresh_cpc)["rnn"]
    assert len(rnn) == len(rnn_before) > 0
    for p, q in zip(rnn, rnn_before):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)) and p.grad is None and p.requires_grad
    (opt,) = made
    stepped = [p for g in opt.param_groups for p in g["params"]]
    assert len(stepped) == len(start) == 25 - len(rnn) and not {id(p) for p in rnn} & {id(p) for p in stepped}
    assert all(p not in opt.state for p in rnn) and len(opt.state) == len(stepped) == len(state["optimizer"]["state"])
    assert all(float(opt.state[p]["step"]) == 2 for p in stepped)
    assert sum(not torch.equal(a, b) for a, b in zip(start, final)) > len(start) // 2      # the parts that were named did step


# ------------------------------------------------------------------ the schedule
def test_scheduled_fits_run_at_the_recorded_learning_rates():
    args, lrs = golden_lrs()
    factory = lambda opt: optim.WarmupScheduler(opt, *args)               # noqa: E731
    log = []
    fit_predictors(recording(optim.Adam, log), 27, scheduler=factory)     # two batches: an epoch is two steps
    got = [lr for lr, _ in log]
    want = [lrs[step // 2] for step in range(27)]
    assert all(abs(a - b) <= 1e-15 * b for a, b in zip(got, want)), (got, want)
    assert len({round(v, 12) for v in got}) >= 8                          # the ramp, the plateau and both milestones were reached
    log = []
    fit_vocoder(recording(optim.Adam, log), 10, scheduler=factory)        # vocoder.py:102-105: the scheduler steps with every step
    got = [lr for lr, _ in log]
    assert all(abs(a - lrs[step]) <= 1e-15 * lrs[step] for step, a in enumerate(got)), got


# ------------------------------------------------------------------ resumed fits
@pytest.mark.parametrize("fit,n", [(fit_predictors, 3), (fit_vocoder, 2), (fit_context, 2), (fit_encoder, 2)],
                         ids=["fit_predictors", "fit_vocoder", "fit_context", "fit_encoder"])
def test_two_fits_joined_by_opt_state_equal_one(fit, n):
    args, _ = golden_lrs()
    factory = lambda opt: optim.WarmupScheduler(opt, *args)               # noqa: E731
    whole_state = {}
    whole, _, final = fit(optim.Adam, 2 * n, scheduler=factory, opt_state=whole_state)
    state = {}
    first, _, mid = fit(optim.Adam, n, scheduler=factory, opt_state=state)
    assert state["steps_done"] == n and set(state) == {"optimizer", "scheduler", "steps_done"}
    assert float(state["optimizer"]["state"][0]["step"]) == n

    # the second fit starts from the first one's parameters: a fresh model loaded with them
    def resumed(optimizer, steps, **kw):
        if fit in (fit_context, fit_encoder):                            # everything the first fit moved: the codebook's state too
            load = tuple({k: v.detach().clone() for k, v in m.state_dict().items()} for m in first["models"])
            r, _, end = fit(optimizer, steps, load=load, **kw)
            return r, end
        if fit is fit_predictors:
            enc, cpc, by_speaker = cpc_models()
            params = driver._predictor_params(cpc)
            with torch.no_grad():
                for p, v in zip(params, mid):
                    p.copy_(v)
            r = driver.fit_predictors(enc, cpc, by_speaker, steps=steps, lr=1e-3, optimizer=optimizer, sample_frames=16, **kw)
        else:
            enc, voc = voc_models()
            params = voc._part_params("ar")
            with torch.no_grad():
                for p, v in zip(params, mid):
                    p.copy_(v)
            r = driver.fit_vocoder(enc, voc, F.waves(), None, F.speakers(), steps=steps, lr=F.LR, optimizer=optimizer,
                                   max_batch=F.MAX_BATCH, clip_codes=F.CLIP, seed=F.SEED, **kw)
        return r, [p.detach().cpu().clone() for p in params]

    second, joined = resumed(optim.Adam, n, scheduler=factory, opt_state=state)
    assert state["steps_done"] == 2 * n == whole_state["steps_done"]
    assert first["losses"] + second["losses"] == whole["losses"]
    for a, b in zip(joined, final):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert state["scheduler"] == whole_state["scheduler"]
    assert state["optimizer"]["param_groups"] == whole_state["optimizer"]["param_groups"]
    for i, st in whole_state["optimizer"]["state"].items():
        for k, v in st.items():
            assert torch.equal(v.cpu(), state["optimizer"]["state"][i][k].cpu()), (i, k)


# ------------------------------------------------------------------ the command line
def test_cli_hip_optimizer_state_written_then_read(tmp_path, capsys):
    ds = tmp_path / "datasets" / "eng"
    (ds / "test").mkdir(parents=True)
    names = [f"S{s}_{u}" for s in (1, 2) for u in "ab"]
    for n in names:
        np.save(ds / "test" / f"{n}.mel.npy", synth.mel("fit/" + n, 1, 44)[0].numpy())
    (ds / "test.json").write_text(json.dumps([["x", 0, 1, f"eng/test/{n}"] for n in names]))
    src, out, state = tmp_path / "in.pt", tmp_path / "fit.pt", tmp_path / "opt.pt"
    torch.save({"encoder": synth.encoder_state_dict(ln_affine="random", codebook="data"), "cpc": synth.cpc_state_dict(n_prediction_steps=4)}, src)
    common = ["fit-predictors", "--dataset", str(ds), "--prediction-steps", "4", "--speakers", "2", "--utterances", "2", "--negatives", "3",
              "--sample-frames", "16", "--steps", "3", "--lr", "4e-4", "--optimizer", "hip", "--warmup", "5", "--initial-lr", "1e-6",
              "--milestones", "8,12", "--gamma", "0.25", "--optimizer-state", str(state)]
    assert cli.main([*common, "--cpc-checkpoint", str(src), "--out-checkpoint", str(out)]) == 0
    text = capsys.readouterr().out
    assert f"wrote {state}" in text and "after 3 steps" in text
    saved = torch.load(state, map_location="cpu", weights_only=True)
    assert set(saved) == {"optimizer", "scheduler", "steps_done"} and saved["steps_done"] == 3
    assert float(saved["optimizer"]["state"][0]["step"]) == 3 and saved["scheduler"]["last_epoch"] == 3      # one batch: an epoch is a step
    _, lrs = golden_lrs()
    assert abs(saved["optimizer"]["param_groups"][0]["lr"] - lrs[3]) <= 1e-15 * lrs[3]
    # read: the second run goes on from the first one's checkpoint and state
    assert cli.main([*common, "--cpc-checkpoint", str(out), "--out-checkpoint", str(tmp_path / "fit2.pt")]) == 0
    assert "after 6 steps" in capsys.readouterr().out
    again = torch.load(state, map_location="cpu", weights_only=True)
    assert again["steps_done"] == 6 and float(again["optimizer"]["state"][0]["step"]) == 6 and again["scheduler"]["last_epoch"] == 6
    assert abs(again["optimizer"]["param_groups"][0]["lr"] - lrs[6]) <= 1e-15 * lrs[6]
    # torch's Adam reads the same file
    assert cli.main([*[a if a != "hip" else "torch" for a in common], "--cpc-checkpoint", str(out), "--out-checkpoint", str(tmp_path / "fit3.pt")]) == 0
    assert torch.load(state, map_location="cpu", weights_only=True)["steps_done"] == 9
