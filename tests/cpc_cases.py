"""Shared by the CPC float64 tests (plain module, not a conftest): the six cases that take ``cpc_score_kernel`` /
``cpc_finish_kernel`` past the four reference-recorded fixtures, their float64 reference, and the derived bounds -- so that the
CPU suite can check, without a GPU, that the conditions the GPU checks rest on hold for the reference alone.

Reference: ``test_cpc_cpu.f64_cpc`` (pinned to the reference project's ``CPCLoss(...).double()`` on the four fixtures there, and on
the five protocol cases here through ``tests/golden/cpc_f64_pins.npz``).  ``err32`` of a case is ``max |f32 - f64|`` of the same
statements run in fp32 numpy.  With u = 2^-24, J = 1 + Neg:

* scores, every element: ``|f_gpu - f64| <= tol = err32 + 1.5e-7 mag`` (``mag``: ``f64_cpc``'s magnitude sum) -- the yardstick of
  tests/test_gpu_cpc.py with the recorded ``ref_err`` replaced by ``err32``.  ``tol_pos`` = max of ``tol`` over j at a position.
* stage 3 (log-sum-exp, ``correct``) and the finish kernel against float64 numpy ON THE GPU'S OWN fp32 SCORES: ``correct`` equals
  ``not any(f_j > f_0)`` at every position, ``accuracy[k] = float32(sum) / float32(N L)`` exactly, and
  ``|step_loss_gpu[k] - mean(lse - f0)| <= mean((J + 16) u max(1, |lse|, |f0|, |m|)) + u |step_loss|``: a sequential fp32 sum of J
  non-negative terms has relative error <= (J - 1) u, which is the absolute error of its log; 16 u covers expf, logf and the two
  fp32 additions at the magnitudes named; the last term is the final rounding to fp32; the sums over positions are in double in
  the kernel.  ``loss`` against the float64 mean of the GPU's step losses: ``u |loss|`` (one rounding).
* end to end: log-sum-exp is non-expansive in the max norm, so ``lse`` and ``f0`` each move by at most ``tol_pos``:
  ``|step_loss_gpu[k] - step_loss64[k]| <= mean(2 tol_pos + (J + 16) u max(...)) + u |step_loss|``; ``correct`` equals
  ``margin64 >= 0`` wherever ``margin64 == 0`` (bit-equal rows give exactly equal float64 scores; a tie is correct) or
  ``|margin64| > 2 tol_pos``; the positions in between are listed and may number at most ``NEAR_TIE_CAP`` of a case's positions.
"""
import numpy as np
import torch

from test_cpc_cpu import NEAR_TIE_CAP, f64_cpc
from vectorquantizedcpc_amd import synth

U32 = 2.0 ** -24

# name -> Spk, Utt, Neg, T, n_prediction_steps (K = half), c_dim, n_codes, runs, wscale
CASES = {
    "c64_min": (1, 2, 1, 3, 2, 64, 512, False, 1),          # L = 2, one negative, one MFMA iteration
    "c512_neg64": (2, 2, 64, 35, 4, 512, 512, False, 1),    # 32 MFMA iterations, 5 pair passes, L = 33 (remainder 1)
    "steps16": (1, 3, 3, 31, 32, 128, 512, True, 1),        # K = 16, L = 15: one tile with 15 live anchors
    "partials": (5, 7, 2, 260, 2, 64, 512, True, 1),        # N = 35, L = 259, 17 tiles: P = 595 partials per step
    "peaked": (2, 3, 17, 40, 6, 256, 64, True, 256),        # scores to +-130, losses 52-59 nats
    "edges": (2, 3, 5, 24, 6, 64, 512, False, 1),           # explicit corner indices
}
PROTOCOL_CASES = [n for n in CASES if n != "edges"]
SHRINK_T = 3                                                # the short call of the workspace test, on ``partials``

_refs = {}


def case(name, T=None):
    """Sizes of a case; ``T`` overrides its length (inputs are then the first T frames of the same z, c)."""
    Spk, Utt, Neg, T0, n_pred, c_dim, n_codes, runs, wscale = CASES[name]
    T = T0 if T is None else T
    K = n_pred // 2
    return dict(name=name, Spk=Spk, Utt=Utt, Neg=Neg, T=T, T0=T0, n_pred=n_pred, c_dim=c_dim, n_codes=n_codes, runs=runs, wscale=wscale,
                K=K, N=Spk * Utt, L=T - K, J=1 + Neg)


def state_dict(g):
    sd = synth.cpc_state_dict(n_prediction_steps=g["n_pred"], c_dim=g["c_dim"])
    return {k: v * g["wscale"] for k, v in sd.items()}


def inputs(g):
    z, c = synth.cpc_inputs(f"f64/{g['name']}", g["N"], g["T0"], c_dim=g["c_dim"], n_codes=g["n_codes"], runs=g["runs"])
    return z[:, :g["T"]].contiguous(), c[:, :g["T"]].contiguous()


def edges_negatives(g):
    """Index arrays that reach the corners: s = 0 and s = L - 1 at every anchor (anchor L - 1 at step K reads the last frame of an
    utterance), u = 0 and u = Utt - 1 from every utterance.  ``s`` may equal ``t``: neither the kernel nor ``f64_cpc`` cares."""
    K, Spk, Utt, Neg, L = g["K"], g["Spk"], g["Utt"], g["Neg"], g["L"]
    t = np.arange(L, dtype=np.int64)
    seq = np.empty((K, Spk, Utt, Neg, L), np.int64)
    seq[:, :, :, 0::2] = L - 1 - t
    seq[:, :, :, 1::2] = np.where(t % 2 == 0, 0, L - 1)
    utt = np.empty((K, Utt, Neg), np.int64)
    utt[:] = (Utt - 1 - np.arange(Utt))[None, :, None]
    utt[:, :, 0] = Utt - 1
    utt[:, :, 1] = 0
    return torch.from_numpy(utt), torch.from_numpy(seq)


def negatives(g, seed=13, stream_id=0):
    if g["name"] == "edges":
        return edges_negatives(g)
    return synth.cpc_negatives(seed, stream_id, g["K"], g["Spk"], g["Utt"], g["Neg"], g["L"])


def stage3(scores):
    """Float64 numpy on fp32 scores (K, N, J, L): per position ``pos_loss`` = lse - f0, ``ok`` = no negative scored above the positive
    (compared on the fp32 values), ``term`` = (J + 16) u max(1, |lse|, |f0|, |m|)."""
    assert scores.dtype == np.float32
    f = scores.astype(np.float64)
    J = f.shape[2]
    m = f.max(axis=2)
    lse = m + np.log(np.exp(f - m[:, :, None]).sum(axis=2))
    f0 = f[:, :, 0]
    ok = ~(scores[:, :, 1:] > scores[:, :, :1]).any(axis=2)
    term = (J + 16) * U32 * np.maximum.reduce([np.ones_like(m), np.abs(lse), np.abs(f0), np.abs(m)])
    return {"pos_loss": lse - f0, "ok": ok, "term": term}


def reference(name, T=None):
    """Float64 reference, fp32 restatement and bounds of a case, computed once and shared (treat as read-only)."""
    if (name, T) not in _refs:
        g = case(name, T)
        sd = state_dict(g)
        z, c = inputs(g)
        utt, seq = negatives(g)
        r64 = f64_cpc(z.numpy(), c.numpy(), sd, utt.numpy(), seq.numpy())
        r32 = f64_cpc(z.numpy(), c.numpy(), sd, utt.numpy(), seq.numpy(), dtype=np.float32)
        assert r32["f"].dtype == np.float32 and r32["step_loss"].dtype == np.float32
        err32 = float(np.abs(r32["f"].astype(np.float64) - r64["f"]).max())
        tol = err32 + 1.5e-7 * r64["mag"]
        margin64 = r64["f"][:, :, 0] - r64["f"][:, :, 1:].max(axis=2)
        tol_pos = tol.max(axis=2)
        g.update(sd=sd, z=z, c=c, utt=utt, seq=seq, r64=r64, r32=r32, err32=err32, tol=tol, tol_pos=tol_pos, tol_max=float(tol.max()),
                 margin64=margin64, near=(margin64 != 0) & (np.abs(margin64) <= 2 * tol_pos))
        _refs[(name, T)] = g
    return _refs[(name, T)]


def loss_bound(ref, s3, step_loss):
    """End-to-end bound on |step_loss - step_loss64| per step, given ``stage3`` of the fp32 scores the step losses were made from."""
    K = ref["K"]
    return (2 * ref["tol_pos"] + s3["term"]).reshape(K, -1).mean(axis=1) + U32 * np.abs(step_loss)


def check_result(ref, r, what):
    """Every float64 check of one detailed call ``r`` (``forward_detailed(..., want_correct=True, want_scores=True)``, tensors
    anywhere) against ``reference(...)``.  Prints each figure before it asserts."""
    K, N, L, J = ref["K"], ref["N"], ref["L"], ref["J"]
    r64 = ref["r64"]
    scores = r["scores"].cpu().numpy()
    correct = r["correct"].cpu().numpy().astype(bool)
    step32, acc32, loss32 = r["step_loss"].cpu().numpy(), r["accuracy"].cpu().numpy(), r["loss"].cpu().numpy()
    step, loss = step32.astype(np.float64), float(loss32)
    assert scores.shape == (K, N, J, L) and correct.shape == (K, N, L) and step.shape == (K,) and acc32.shape == (K,)
    assert np.isfinite(scores).all() and np.isfinite(step).all() and np.isfinite(loss)

    # scores, every element
    err = np.abs(scores.astype(np.float64) - r64["f"])
    print(f"\n{what}: max(|f_gpu - f64| / tol) = {(err / ref['tol']).max():.4f}   max|f_gpu - f64| / err32 = {err.max() / ref['err32']:.4f}   "
          f"(max|f_gpu - f64| = {err.max():.3g}, err32 = {ref['err32']:.3g}, tol_max = {ref['tol_max']:.3g}, max|f64| = {np.abs(r64['f']).max():.4g})")
    assert (err <= ref["tol"]).all()

    # stage 3 and the finish kernel against the GPU's own scores
    s3 = stage3(scores)
    assert np.array_equal(correct, s3["ok"]), np.argwhere(correct != s3["ok"]).tolist()
    assert np.array_equal(acc32, s3["ok"].reshape(K, -1).sum(axis=1).astype(np.float32) / np.float32(N * L))
    own = s3["pos_loss"].reshape(K, -1).mean(axis=1)
    own_bound = s3["term"].reshape(K, -1).mean(axis=1) + U32 * np.abs(step)
    own_mean = float(step.mean())
    print(f"{what}: stage 3 on the GPU's scores: max(|step_loss_gpu - mean(lse - f0)| / bound) = {(np.abs(step - own) / own_bound).max():.4f} "
          f"(max error {np.abs(step - own).max():.3g}, bound there {own_bound[np.argmax(np.abs(step - own))]:.3g}); "
          f"|loss - mean(step_loss_gpu)| = {abs(loss - own_mean):.3g} (bound {U32 * abs(loss):.3g})")
    assert (np.abs(step - own) <= own_bound).all()
    assert abs(loss - own_mean) <= U32 * abs(loss)

    # against float64 end to end
    bound = loss_bound(ref, s3, step)
    e2e = np.abs(step - r64["step_loss"])
    print(f"{what}: max|step_loss_gpu - step_loss64| = {e2e.max():.3g} (bound there {bound[np.argmax(e2e)]:.3g}, max ratio {(e2e / bound).max():.4f}); "
          f"|loss_gpu - loss64| = {abs(loss - r64['loss']):.3g}; step_loss64 {r64['step_loss'].min():.4f} .. {r64['step_loss'].max():.4f}")
    assert (e2e <= bound).all()
    assert abs(loss - r64["loss"]) <= bound.mean() + U32 * abs(loss)
    margin64, near = ref["margin64"], ref["near"]
    differ = np.argwhere(correct != (margin64 >= 0))
    print(f"{what}: exact-tie positions {int((margin64 == 0).sum())}, near-tie positions (0 < |margin64| <= 2 tol_pos) {int(near.sum())} of "
          f"{near.size}: {np.argwhere(near).tolist()}; positions where correct differs from float64: {differ.tolist()}")
    assert np.array_equal(correct[~near], (margin64 >= 0)[~near])
    assert correct[margin64 == 0].all()
    assert near.sum() <= NEAR_TIE_CAP * near.size
