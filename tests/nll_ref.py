"""Shared by the vocoder-scoring tests (plain module, not a conftest): the float64 reference value of ``Vocoder.nll``, the
derived tolerances, and the synthetic inputs of the GPU cases -- so that the CPU suite can check the conditions on those
inputs (the 1 % ambiguity cap) without a GPU.

Reference: ``F64Vocoder.condition(z, spk, n_codes)`` -> ``F64Vocoder.logits(audio[:, :-1], cond, lengths - 1)`` -> float64
``log_softmax`` -> gather ``audio[:, 1:]``: the objective of the reference's ``vocoder.py:62-63`` restated (the energies of all
but the last sample against all but the first, cross-entropy), checked against ``torch.nn.functional.cross_entropy`` in
tests/test_vocoder_nll_cpu.py.

Per-sample bound.  Log-sum-exp is 1-Lipschitz in the max norm and the target's energy moves by at most the same amount, so
energies within E of float64 (E = LOGIT_TOL of tests/test_gpu_vocoder_f64.py: 1e-6 default, 5e-5 stressed weights) give
|nll_gpu - nll_f64| <= 2 E + R, with R for the fp32 evaluation of the log-sum-exp as a fixed tree over 256 terms in (0, 1]
(8 roundings on a path), expf / logf at a couple of ulp, the final add and subtract: R = 16 ulp_f32(max(1, |lse|, |e_target|)).
"""
import numpy as np
import torch

from oracle import f64_ref
from vectorquantizedcpc_amd import synth

LOGIT_TOL = {"default": 1e-6, "stressed": 5e-5}          # as tests/test_gpu_vocoder_f64.py
AMBIGUOUS_CAP = 0.01
UP2 = 320                                                # samples per code: 2 * upsampling_t

_models = {}
_refs = {}


def state_dict(name):
    sd = synth.vocoder_state_dict()
    return f64_ref.stressed(sd) if name == "stressed" else sd


def f64_model(name):
    if name not in _models:
        _models[name] = f64_ref.F64Vocoder(state_dict(name))
    return _models[name]


def nll_from_energies(energies, targets):
    """float64 (nll, lse, e_target, best - e_target, best - second best) per position from energies (..., n_cls) and targets (...)."""
    e = torch.as_tensor(energies, dtype=torch.float64)
    t = torch.as_tensor(targets).long()
    lse = torch.logsumexp(e, dim=-1)
    et = e.gather(-1, t[..., None])[..., 0]
    nll = -torch.log_softmax(e, dim=-1).gather(-1, t[..., None])[..., 0]
    top = e.topk(2, dim=-1).values
    return nll.numpy(), lse.numpy(), et.numpy(), (top[..., 0] - et).numpy(), (top[..., 0] - top[..., 1]).numpy()


class Ref:
    """The float64 reference of one scoring call and what the checks derive from it.  Arrays are (B, L - 1); `mask` marks the
    scored positions of every row."""

    def __init__(self, name, audio, z, spk, n_codes=None, lengths=None, sd=None, upsample=160, tol=None):
        """`name`: one of the two weight sets of this module -- or, with a state dict `sd`, only a label: the model is then
        F64Vocoder(sd, upsample) at whatever sizes `sd` has, and `tol` its logit tolerance E."""
        audio = torch.as_tensor(audio).long().cpu()
        B, L = audio.shape
        self.name = name
        self.lengths = [L] * B if lengths is None else [int(n) for n in lengths]
        self.n_scored = np.array([max(n - 1, 0) for n in self.lengths], np.int64)
        f = f64_model(name) if sd is None else f64_ref.F64Vocoder(sd, upsample=upsample)
        top = f.n_cls - 1
        lg = f.logits(audio[:, :-1].clamp(0, top), f.condition(z, spk, n_codes), list(self.n_scored))
        self.nll, self.lse, self.et, self.gap_target, self.gap_second = nll_from_energies(lg, audio[:, 1:].clamp(0, top))
        self.mask = np.arange(L - 1)[None, :] < self.n_scored[:, None]
        self.nll = np.where(self.mask, self.nll, 0.0)
        tol = LOGIT_TOL[name] if tol is None else tol
        r = 16.0 * f64_ref.ulp_f32(np.maximum(1.0, np.maximum(np.abs(self.lse), np.abs(self.et))))
        self.R = np.where(self.mask, r, 0.0)
        self.bound = np.where(self.mask, 2.0 * tol + r, 0.0)            # per sample
        d = 2.0 * tol
        sure = self.mask & (self.gap_target == 0.0) & (self.gap_second > d)
        amb = self.mask & ~sure & (self.gap_target <= d)
        self.sure_correct = sure.sum(axis=1)
        self.ambiguous = amb.sum(axis=1)
        self.nll_sum = self.nll.sum(axis=1)
        self.sum_bound = self.bound.sum(axis=1)     # <= n_scored * (largest per-sample bound), the issue's per-utterance bound

    @property
    def loss(self):
        return float(self.nll_sum.sum() / self.n_scored.sum())

    def ambiguous_fraction(self):
        return float(self.ambiguous.sum()) / max(int(self.n_scored.sum()), 1)


def check_result(ref, nll_sum, n_scored, n_correct, nll=None, rows=None, what=""):
    """GPU outputs (host arrays) of the rows `rows` of `ref` (default all, in order) against float64.  Prints the observed maxima
    before it asserts; returns the largest per-sample error."""
    rows = list(range(len(ref.n_scored))) if rows is None else list(rows)
    nll_sum, n_scored, n_correct = np.asarray(nll_sum), np.asarray(n_scored), np.asarray(n_correct)
    worst = ratio = 0.0
    if nll is not None:
        nll = np.asarray(nll, np.float64)
        w = nll.shape[1]
        err = np.abs(nll - ref.nll[rows][:, :w])
        worst = float(err.max()) if err.size else 0.0
        ratio = float((err / np.maximum(ref.bound[rows][:, :w], 1e-300))[ref.mask[rows][:, :w]].max()) if ref.mask[rows].any() else 0.0
    serr = np.abs(nll_sum - ref.nll_sum[rows])
    print("%s %s: max per-sample |GPU - f64| = %.3g (%.3g of its bound), max per-utterance sum error %.3g (bound %.3g), "
          "correct %s within [%s, %s]" % (ref.name, what, worst, ratio, float(serr.max()), float(ref.sum_bound[rows].max()),
                                          n_correct.tolist(), ref.sure_correct[rows].tolist(),
                                          (ref.sure_correct + ref.ambiguous)[rows].tolist()))
    assert np.array_equal(n_scored, ref.n_scored[rows]), (what, n_scored, ref.n_scored[rows])
    if nll is not None:
        assert not nll[~ref.mask[rows][:, :w]].any(), (what, "padding columns of nll must be 0")
        assert (err <= ref.bound[rows][:, :w]).all(), (what, worst, ratio)
    assert (serr <= ref.sum_bound[rows]).all(), (what, serr, ref.sum_bound[rows])
    assert (n_correct >= ref.sure_correct[rows]).all() and (n_correct <= (ref.sure_correct + ref.ambiguous)[rows]).all(), what
    return worst


# ---------------------------------------------------------------------- inputs of the GPU cases
def case_equal():
    """vocoder.py:62-63's shape: B = 4, L = 5120 (5 119 scored steps), Tc = 16."""
    return dict(audio=synth.randint("nll/eq/a", (4, 5120), 256), z=synth.randint("nll/eq/z", (4, 16), 512),
                spk=synth.randint("nll/eq/s", (4,), 102), n_codes=None, lengths=None)


def case_ragged():
    """B = 5, distinct code counts; row 0 scores nothing, row 1 ends exactly where its codes end (n_audio - 1 = 320 n_codes), rows 2
    and 4 are cut short in mid-frame."""
    n_codes = [6, 5, 3, 4, 2]
    lengths = [1, UP2 * 5 + 1, 700, 1200, 333]
    return dict(audio=synth.randint("nll/rag/a", (5, 1700), 256), z=synth.randint("nll/rag/z", (5, 6), 512),
                spk=synth.randint("nll/rag/s", (5,), 102), n_codes=n_codes, lengths=lengths)


def case_big():
    """B = 32 on the large-batch GRU kernel with big_min_tiles 2, 1 700 steps: two whole chunks of 640 and a part of a third.
    The issue names B = 96 with the default big_min_tiles, or B = 16 with big_min_tiles 1.  The second does not reach the kernel: a
    one-tile call (B <= 16) takes the small GRU kernel whatever big_min_tiles says (launch_gru_step tests nbt == 1 first), and
    B = 96 triples the float64 reference's cost.  Two tiles with big_min_tiles 2 is the smallest call that does run
    ar_gru_big_kernel; the GPU test asserts through kernel_times() that it ran."""
    return dict(audio=synth.randint("nll/big/a", (32, 1701), 256), z=synth.randint("nll/big/z", (32, 6), 512),
                spk=synth.randint("nll/big/s", (32,), 102), n_codes=None, lengths=None)


CASES = {"equal": case_equal, "ragged": case_ragged, "big": case_big}


def reference(name, case):
    """Ref of a named case on a weight set, computed once per process."""
    key = (name, case)
    if key not in _refs:
        c = CASES[case]()
        _refs[key] = Ref(name, c["audio"], c["z"], c["spk"], c["n_codes"], c["lengths"])
    return _refs[key]


def waves(n=12, seed="nll/wave"):
    """Mixed-length synthetic utterances at 16 kHz: a few sines plus noise, seeded by name (synth has no wave generator)."""
    out = []
    for i in range(n):
        ln = 3200 + 677 * ((5 * i + 3) % n)
        u = np.asarray(synth.uniform01(f"{seed}/{i}", ln + 8), dtype=np.float64)
        t = np.arange(ln) / 16000.0
        w = 0.25 * (2.0 * u[:ln] - 1.0)
        for k in range(3):
            w = w + (0.2 + 0.3 * u[ln + k]) * np.sin(2 * np.pi * (110.0 + 900.0 * u[ln + 3 + k]) * t + 6.28 * u[ln + 6])
        out.append((0.3 * w).astype(np.float32))
    return out
