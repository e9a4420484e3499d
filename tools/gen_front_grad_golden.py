"""Writes tests/golden/front_grad_pins.npz (the fifteen cases and ``chain``) and tests/golden/front_grad_wide_pins.npz (the fourteen
``WIDE_CASES``), the pins of tests/front_grad_ref.py's float64 reference of the front-end gradients: per case and tensor 64 sampled elements, the sum and the sum of squares, the largest magnitude -- and ``e_ref = max |G_ref32 - G_ref64|``,
the error of the same torch modules (and, for ``chain``, of the same composition with the VQ step, the LSTM and the CPC loss) run in
fp32 on the CPU under the same forced ReLU masks (and code indices).  Per case it records ``differ``: the number of mask elements in
which the float64 run's own ReLUs differ from the fp32 program's; for ``chain`` also the smallest VQ margin of the fp32 forward, and
-- after asserting that the float64 and the fp32 CPU run of the tests' fit pick the same codes at every step -- of that fit.
The judges of the tests are built from these alone.  Data only; written with fixed archive dates: the same bytes at every run.

    python tools/gen_front_grad_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import front_grad_ref as R  # noqa: E402
import grad_judge  # noqa: E402


def pins_of(names):
    out = {}
    for name in names:
        ref = R.grads64(name)
        low = R.chain_grads(torch.float32) if name == R.CHAIN else R.torch_grads(name, torch.float32)
        out.update(grad_judge.pin_entries(name, ref, low, R.POSITIONS, R.tensors(name)))
        for k in R.tensors(name):
            print(f"{name} {k}: max {out[f'{name}_{k}_max']:.3g}, e_ref {out[f'{name}_{k}_e_ref']:.3g}")
        if "differ" in ref:
            out[f"{name}_differ"] = np.int64(ref["differ"])
            print(f"{name}: {ref['differ']} mask elements differ between the fp32 program and the float64 run")
    return out


def main():
    torch.set_num_threads(1)                                        # one summation order for the recorded fp32 error
    out = pins_of(R.ALL_CASES + [R.CHAIN])
    g = R.chain_case()
    out["chain_vq_margin"] = np.float64(R.chain_forced(g["w"], g["E"], g["mel"])[2])
    print(f"chain: smallest VQ margin of the fp32 forward {out['chain_vq_margin']:.3g}")
    # the fit of the tests: over all its steps the float64 run and the fp32 CPU run must pick the same codes
    _, idx64, _, m64 = R.chain_sgd(torch.float64, R.FIT_STEPS, R.FIT_LR)
    _, idx32, _, m32 = R.chain_sgd(torch.float32, R.FIT_STEPS, R.FIT_LR)
    assert all(np.array_equal(a, b) for a, b in zip(idx64, idx32)), "the fit's batch: float64 and fp32 pick different codes"
    out["chain_fit_vq_margin"] = np.float64(min(m64, m32))
    print(f"chain fit ({R.FIT_STEPS} steps, lr {R.FIT_LR}): the same codes at every step, smallest VQ margin {out['chain_fit_vq_margin']:.3g}")
    grad_judge.write_npz(R.PINS, out)
    wide = pins_of(R.ALL_WIDE)
    for name in R.ALL_WIDE:                                         # what the wide cases are there for
        ref = R.grads64(name)
        assert all(np.isfinite(ref[k]).all() for k in R.tensors(name)), name
    grad_judge.write_npz(R.WIDE_PINS, wide)


if __name__ == "__main__":
    main()
