"""Writes tests/golden/cond_grad_pins.npz: the pins of tests/cond_grad_ref.py's float64 references -- the conditioning path's
eighteen gradients per case, and the whole vocoder's 27 on the chain cases (``chain_<case>``): per tensor 64 sampled elements, the sum
and the sum of squares, the largest magnitude -- and ``e_ref = max |G_ref32 - G_ref64|``, the error of the same statements run in
fp32 on the CPU (``grad_judge.pin_entries``).  The judge of the GPU tests is built from these alone.  Also ``fit_<run>_losses``: the
per-step losses of the float64 fits with the conditioning parts stepping, which the GPU fits are compared with; the run that
leaves rnnms.ar frozen must fall by several times the spread of its own last five steps, or this script fails.
Then tests/golden/cond_grad_wide_pins.npz: the same pins of ``WIDE_CASES`` and of the chain on ``CHAIN_WIDE``, and for the two table
gradients the row pins of ``grad_judge.row_pin_entries``, whose ``e_ref`` per row is the larger of two fp32 yardsticks: ``nn.GRU``
and the manual loop over the frames.
Written with fixed archive dates: the same bytes at every run.

    python tools/gen_cond_grad_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cond_grad_ref as R  # noqa: E402
import grad_judge  # noqa: E402
import voc_fit_ref  # noqa: E402


def main():
    torch.set_num_threads(1)                                        # one summation order for the recorded fp32 error
    out = {}
    for name in R.ALL_CASES:
        ref, low = R.grads64(name), R.grads(name, torch.float32)
        for k in R.KEYS + ("cond",):                                # tensor by tensor: the archive keeps this order
            out.update(grad_judge.pin_entries(name, ref, low, R.POSITIONS, [k]))
            print(f"{name} {k}: max {out[f'{name}_{k}_max']:.3g}, e_ref {out[f'{name}_{k}_e_ref']:.3g}")
    for name in R.CHAIN_CASES:
        ref, low = R.chain64(name), R.chain_grads(name, torch.float32)
        for k in R.ALL27:
            out.update(grad_judge.pin_entries("chain_" + name, ref, low, R.POSITIONS, [k]))
            print(f"chain_{name} {k}: max {out[f'chain_{name}_{k}_max']:.3g}, e_ref {out[f'chain_{name}_{k}_e_ref']:.3g}")
        out[f"chain_{name}_loss"] = np.float64(ref["loss"])
        print(f"chain_{name} loss: {float(ref['loss']):.9f} (fp32 {float(low['loss']):.9f})")
    for run, (train, steps, lr) in R.FIT_RUNS.items():
        losses = out[f"fit_{run}_losses"] = R.fit_reference_losses(train, steps, lr)
        dec, spread = voc_fit_ref.decrease(losses), float(losses[-5:].max() - losses[-5:].min())
        print(f"fit {run} {train}: losses {losses}, decrease {dec:.5f}, spread of the last five {spread:.5f}")
        assert dec > 4.0 * spread, (run, dec, spread)               # the reference alone must clear its own noise
    grad_judge.write_npz(R.PINS, out)
    out = {}
    for name in R.ALL_WIDE:
        ref, low, loop = R.grads64(name), R.grads(name, torch.float32), R.grads(name, torch.float32, manual=True)
        for k in R.KEYS + ("cond",):
            out.update(grad_judge.pin_entries(name, ref, low, R.POSITIONS, [k]))
            print(f"{name} {k}: max {out[f'{name}_{k}_max']:.3g}, e_ref {out[f'{name}_{k}_e_ref']:.3g}")
        out.update(grad_judge.row_pin_entries(name, ref, [low, loop], R.ROW_TENSORS))
    for name in R.CHAIN_WIDE:
        ref, low = R.chain64(name), R.chain_grads(name, torch.float32)
        for k in R.ALL27:
            out.update(grad_judge.pin_entries("chain_" + name, ref, low, R.POSITIONS, [k]))
            print(f"chain_{name} {k}: max {out[f'chain_{name}_{k}_max']:.3g}, e_ref {out[f'chain_{name}_{k}_e_ref']:.3g}")
        out[f"chain_{name}_loss"] = np.float64(ref["loss"])
        print(f"chain_{name} loss: {float(ref['loss']):.9f} (fp32 {float(low['loss']):.9f})")
    grad_judge.write_npz(R.WIDE_PINS, out)


if __name__ == "__main__":
    main()
