#!/usr/bin/env python3
"""Generate tests/golden/cpc_*.npz from the REFERENCE's own ``CPCLoss`` (runs in the build container only).

Imports the reference's ``model.py`` through ``gen_golden.import_reference``, loads ``synth.cpc_state_dict()`` into
``CPCLoss(ConfCPC(...))`` and, for the duration of each call, wraps ``torch.randint`` to RECORD what the reference drew
(``model.py:251-268``) and ``F.cross_entropy`` to read the scores ``f`` (``model.py:291``) it is handed.  The same draws are
then REPLAYED through ``CPCLoss(...).double()``: the reference's own fp32 distance from float64 (``ref_err``,
``ref_loss_err``) is one of the two yardsticks of tests/test_gpu_cpc.py.  Fixtures are DATA only -- parameters, key
lists, index arrays, recorded results; inputs and weights are rebuilt from seeds (``synth.cpc_inputs``).

Index arrays: ``utt_index`` (K, Utt, Neg) and ``seq_index`` (K, Spk, Utt, Neg, L) after the remainder, uint8.  The train
shape's ``seq_index`` is 418 KB of incompressible values below 64, more than any fixture here may weigh, so its draws
are stored one step per file (``cpc_train_draws_k<k>.npz``, ~53 KB each) and shared by ``train_shape`` and ``train_e2e``
(recorded once, replayed for the second): every step stays checked position by position.

``cpc_f64_pins.npz``: the float64 step losses and accuracies of the reference's ``CPCLoss(...).double()`` at the five protocol
cases of tests/cpc_cases.py, with the protocol's own draws replayed (raw sequence draw r = (seq - t) mod L); it pins
``test_cpc_cpu.f64_cpc`` to the reference at those shapes (tests/test_cpc_f64_cpu.py).

Usage:  python tools/gen_cpc_golden.py            (writes tests/golden/cpc_*.npz)
        python tools/gen_cpc_golden.py --pins     (writes tests/golden/cpc_f64_pins.npz only)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden import GOLD, import_reference  # noqa: E402
from vectorquantizedcpc_amd import synth  # noqa: E402

# name -> (Spk, Utt, Neg, T, n_prediction_steps, c_dim, n_codes, runs)
CASES = {
    "train_shape": (8, 8, 17, 70, 12, 256, 512, True),     # config.py:42-47: 128 + 12 mel frames -> 70
    "ties": (2, 4, 5, 24, 6, 256, 8, False),               # 8-entry codebook: bit-equal negatives everywhere
    "small_odd": (3, 2, 7, 19, 4, 128, 512, False),        # odd sizes, tile remainders
    "one_utt": (1, 1, 4, 12, 2, 256, 512, False),          # every negative comes from the anchor's own utterance
}
SHARED_DRAWS = {"train_shape": "train", "train_e2e": "train"}
NEAR_TIE_CAP = 0.005          # share of positions with 0 < |margin| <= 2 tol_max a committed case may hold
MAX_BYTES = 126221            # the largest fixture committed before these (encoder_c2_init.npz)


class Tap:
    """Record (or replay) the reference's ``torch.randint`` draws and read the arguments / results of ``F.cross_entropy``."""

    def __init__(self, replay=None):
        self.draws, self.replay, self.f, self.losses = [], list(replay) if replay is not None else None, [], []

    def __enter__(self):
        self._randint, self._ce = torch.randint, torch.nn.functional.cross_entropy

        def randint(low, high, size, **kw):
            if self.replay is not None:
                return self.replay.pop(0).clone()
            t = self._randint(low, high, size, **kw)
            self.draws.append(t.clone())                         # model.py:270 adds to it in place
            return t

        def cross_entropy(f, labels, *a, **kw):
            out = self._ce(f, labels, *a, **kw)
            self.f.append(f.detach().clone())
            self.losses.append(out.detach().clone())
            return out

        torch.randint, torch.nn.functional.cross_entropy = randint, cross_entropy
        return self

    def __exit__(self, *exc):
        torch.randint, torch.nn.functional.cross_entropy = self._randint, self._ce


def f64_scores(z, c, W, b, utt, seq):
    """Steps 1-4 of CPCLoss.forward in float64 numpy, with the magnitude sums the score tolerance is made of.
    z (N, T, 64), c (N, T, C), W (K, 64, C), b (K, 64), utt (K, Utt, Neg), seq (K, Spk, Utt, Neg, L) -> f, mag (K, N, 1 + Neg, L)."""
    K, Spk, Utt, Neg, L = seq.shape
    z, c, W, b = (np.asarray(a, np.float64) for a in (z, c, W, b))
    zs = z.reshape(Spk, Utt, -1, z.shape[-1])
    f = np.empty((K, Spk * Utt, 1 + Neg, L))
    mag = np.empty_like(f)
    spk = np.arange(Spk).reshape(-1, 1, 1, 1)
    for k in range(1, K + 1):
        wc = c[:, :L] @ W[k - 1].T + b[k - 1]
        wc_abs = np.abs(c[:, :L]) @ np.abs(W[k - 1]).T + np.abs(b[k - 1])
        shift = zs[:, :, k:L + k]
        rows = np.concatenate([shift[:, :, None], shift[spk, utt[k - 1][None, :, :, None], seq[k - 1]]], axis=2)
        rows = rows.reshape(Spk * Utt, 1 + Neg, L, -1)
        f[k - 1] = (rows * wc[:, None]).sum(-1) / 8.0
        mag[k - 1] = ((np.abs(rows) * wc_abs[:, None]).sum(-1) + np.abs(rows * wc[:, None]).sum(-1)) / 8.0
    return f, mag


def run_reference(model, conf, sd, z, c, replay=None, double=False):
    cpc = model.CPCLoss(model.ConfCPC(*conf))
    assert list(sd.keys()) == list(cpc.state_dict().keys())
    cpc.load_state_dict(sd)
    if double:
        cpc, z, c = cpc.double(), z.double(), c.double()
    with torch.no_grad(), Tap(replay) as tap:
        loss, acc = cpc(z, c)
    return cpc, tap, loss, acc


def save(name, out):
    path = os.path.join(GOLD, f"cpc_{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
    return os.path.getsize(path)


def fixture(model, name, z, c, conf, sd, draws=None, full=True, extra=None):
    """One case: fp32 run (recording the draws unless given), float64 replay, derived records."""
    n_pred, Spk, Utt, Neg, _, c_dim = conf
    K, N, L = n_pred // 2, Spk * Utt, z.shape[1] - n_pred // 2
    cpc, tap, loss, acc = run_reference(model, conf, sd, z, c, replay=draws)
    raw = draws if draws is not None else tap.draws
    assert len(raw) == 2 * K
    utt = np.stack([raw[2 * k].numpy() for k in range(K)])
    seq = np.stack([(raw[2 * k + 1].numpy() + np.arange(L)) % L for k in range(K)])             # model.py:270-272
    assert utt.shape == (K, Utt, Neg) and seq.shape == (K, Spk, Utt, Neg, L) and seq.max() < 256
    f32 = np.stack([f.numpy() for f in tap.f])                                                    # (K, N, 1 + Neg, L)
    _, tap64, loss64, _ = run_reference(model, conf, sd, z, c, replay=raw, double=True)
    f64 = np.stack([f.numpy() for f in tap64.f])
    W = np.stack([sd[f"predictors.{k}.weight"].numpy() for k in range(K)])
    b = np.stack([sd[f"predictors.{k}.bias"].numpy() for k in range(K)])
    mine, mag = f64_scores(z.numpy(), c.numpy(), W, b, utt, seq)
    assert np.abs(mine - f64).max() <= 1e-12 * max(1.0, np.abs(f64).max()), "the index arrays do not mean what the ABI says"
    ref_err = float(np.abs(f32.astype(np.float64) - f64).max())
    tol_max = float((ref_err + 1.5e-7 * mag).max())
    margin = f32[:, :, 0] - f32[:, :, 1:].max(axis=2)                                             # fp32, (K, N, L)
    correct = f32.argmax(axis=2) == 0
    assert np.array_equal(correct, margin >= 0)
    assert np.allclose(correct.reshape(K, -1).mean(1), acc, atol=1e-7)
    near = (margin != 0) & (np.abs(margin) <= 2 * tol_max)
    ties = margin == 0
    zs = z.numpy().reshape(Spk, Utt, -1, 64)
    equal = np.mean([(zs[np.arange(Spk).reshape(-1, 1, 1, 1), utt[k][None, :, :, None], seq[k] + k + 1]
                      == zs[:, :, None, k + 1:L + k + 1]).all(-1).mean() for k in range(K)])
    out = {
        "case": np.array([n_pred, Spk, Utt, Neg, 64, c_dim, z.shape[1]]),
        "loss": np.array(loss.item(), np.float32), "step_loss": np.array([l.item() for l in tap.losses], np.float32),
        "accuracies": np.array(acc, np.float32),
        "loss64": np.array(loss64.item()), "step_loss64": np.array([l.item() for l in tap64.losses]),
        "ref_err": np.array(ref_err), "ref_loss_err": np.array(abs(float(loss.item()) - loss64.item())),
        "tol_max": np.array(tol_max),
        "n_near_1e5": (np.abs(margin) <= 1e-5).reshape(K, -1).sum(1),
        "share_equal_negatives": np.array(equal), "share_ties": np.array(ties.mean()), "share_near": np.array(near.mean()),
    }
    if name in SHARED_DRAWS:
        out["draws"] = np.array(SHARED_DRAWS[name])
    else:
        out["draws"] = np.array("inline")
        out["utt_index"], out["seq_index"] = utt.astype(np.uint8), seq.astype(np.uint8)
    if full:
        out.update({
            "keys": np.array(list(cpc.state_dict().keys())),
            "shapes": np.array([list(v.shape) + [0] * (2 - v.dim()) for v in cpc.state_dict().values()]),
            "margin": margin.astype(np.float32), "correct": np.packbits(correct.reshape(-1)),
            "rows_scores": f32[:, :: max(1, N // 2)][:, :2][..., [0, L - 1]].copy(),      # utterances 0 and N / 2, positions 0 and L - 1: all 1 + Neg scores
            "sum_scores": np.array([f32.astype(np.float64).sum(), (f32.astype(np.float64) ** 2).sum()]),
        })
    out.update(extra or {})
    for k in range(K if full else 0):        # cases checked position by position
        assert near[k].mean() <= NEAR_TIE_CAP, (name, k, near[k].mean())      # so the reference alone passes the accuracy check
    if name == "ties":
        assert ties.mean() >= 0.10, ties.mean()
    size = save(name, out)
    print(f"{name}: K={K} N={N} L={L} loss={loss.item():.7f} loss64={loss64.item():.9f} acc={np.round(acc, 4).tolist()} "
          f"ref_err={ref_err:.3g} tol_max={tol_max:.3g} negatives bit-equal to their positive={equal:.4f} "
          f"exact-tie positions={ties.mean():.4f} near-tie positions={near.mean():.5f} ({int(near.sum())}) "
          f"|margin|<=1e-5 per step={out['n_near_1e5'].tolist()} bytes={size}")
    return raw, utt, seq


def pins(model):
    """K float64 step losses and K accuracies per protocol case of tests/cpc_cases.py, from the reference on the protocol's draws."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cpc_cases
    out = {}
    for name in cpc_cases.PROTOCOL_CASES:
        g = cpc_cases.case(name)
        z, c = cpc_cases.inputs(g)
        utt, seq = cpc_cases.negatives(g)
        raw = []
        for k in range(g["K"]):
            r = torch.remainder(seq[k] - torch.arange(g["L"]), g["L"])
            assert int(r.min()) >= 1 and int(r.max()) < g["L"]                    # what randint(1, length) can return
            raw += [utt[k].clone(), r]
        conf = (g["n_pred"], g["Spk"], g["Utt"], g["Neg"], 64, g["c_dim"])
        _, tap, _, acc = run_reference(model, conf, cpc_cases.state_dict(g), z, c, replay=raw, double=True)
        assert not tap.replay and len(tap.losses) == g["K"]
        out[f"{name}_step_loss64"] = np.array([l.item() for l in tap.losses], np.float64)
        out[f"{name}_accuracy"] = np.array(acc, np.float64)
        print(f"{name}: step_loss64 = {np.round(out[f'{name}_step_loss64'], 6).tolist()} accuracy = {np.round(acc, 4).tolist()}")
    path = os.path.join(GOLD, "cpc_f64_pins.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < MAX_BYTES
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(1)
    model = import_reference()
    print("reference imported from", model.__file__, "| torch", torch.__version__)
    if "--pins" in sys.argv[1:]:
        return pins(model)
    train_raw = None
    for i, (name, (Spk, Utt, Neg, T, n_pred, c_dim, n_codes, runs)) in enumerate(CASES.items()):
        torch.manual_seed(1000 + i)
        conf = (n_pred, Spk, Utt, Neg, 64, c_dim)
        sd = synth.cpc_state_dict(n_prediction_steps=n_pred, c_dim=c_dim)
        z, c = synth.cpc_inputs(name, Spk * Utt, T, c_dim=c_dim, n_codes=n_codes, runs=runs)
        raw, utt, seq = fixture(model, name, z, c, conf, sd, extra={"n_codes": np.array(n_codes), "runs": np.array(runs),
                                "source": np.array("reference model.py CPCLoss.forward, fp32 and float64 replay of the same recorded draws; "
                                                   "every step's index arrays stored (train draws: one file per step)")})
        if name == "train_shape":
            train_raw = raw
            for k in range(utt.shape[0]):
                path = os.path.join(GOLD, f"cpc_train_draws_k{k + 1}.npz")
                np.savez_compressed(path, utt_index=utt[k].astype(np.uint8), seq_index=seq[k].astype(np.uint8))
                assert os.path.getsize(path) < MAX_BYTES
    # train_e2e: z, c from the reference's own Encoder.forward (model.py:72-86), the train shape's draws replayed
    enc = model.Encoder(model.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict(ln_affine="random", codebook="data"))
    enc.eval()
    with torch.no_grad():
        z, c, _, _ = enc(synth.mel("cpc_e2e", 64, 140))
    fixture(model, "train_e2e", z.contiguous(), c.contiguous(), (12, 8, 8, 17, 64, 256), synth.cpc_state_dict(), draws=train_raw,
            full=False, extra={"mel": np.array("cpc_e2e"), "source": np.array(
                "reference Encoder.forward on synth.mel('cpc_e2e', 64, 140) (ln_affine random, data codebook) -> reference "
                "CPCLoss.forward with the train shape's recorded draws")})
    pins(model)
    print("wrote", sorted(f for f in os.listdir(GOLD) if f.startswith("cpc_")))


if __name__ == "__main__":
    main()
