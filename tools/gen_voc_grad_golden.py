"""Writes tests/golden/voc_grad_pins.npz: the pins of tests/voc_grad_ref.py's float64 reference of the vocoder gradients -- per case
and tensor 64 sampled elements, the sum and the sum of squares, the largest magnitude -- and ``e_ref = max |G_ref32 - G_ref64|``, the
error of the same statements run in fp32 on the CPU (``grad_judge.pin_entries``).  The judge of the GPU test is built from these
alone.  Also ``fit_ref_losses``: the per-step losses of tests/voc_fit_ref.py's float64 fit, which the GPU fit is compared with.
Then tests/golden/voc_grad_wide_pins.npz: the same pins of ``WIDE_CASES``, and for ``embedding`` (per class) and ``grad_cond`` (per
utterance and frame) the row pins of ``grad_judge.row_pin_entries``.
Written with fixed archive dates: the same bytes at every run.

    python tools/gen_voc_grad_golden.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import grad_judge  # noqa: E402
import voc_fit_ref  # noqa: E402
import voc_grad_ref as R  # noqa: E402


def main():
    torch.set_num_threads(1)                                        # one summation order for the recorded fp32 error
    out = {}
    for name in R.ALL_CASES:
        ref, low = R.grads64(name), R.grads(name, torch.float32)
        for k in R.TENSORS:                                         # tensor by tensor: the archive keeps this order
            out.update(grad_judge.pin_entries(name, ref, low, R.POSITIONS, [k]))
            print(f"{name} {k}: max {out[f'{name}_{k}_max']:.3g}, e_ref {out[f'{name}_{k}_e_ref']:.3g}")
        print(f"{name} loss: {float(ref['loss']):.9f} (fp32 {float(low['loss']):.9f})")
    out["fit_ref_losses"] = voc_fit_ref.reference_losses()
    print("fit reference losses:", out["fit_ref_losses"], "decrease", voc_fit_ref.decrease(out["fit_ref_losses"]))
    grad_judge.write_npz(R.PINS, out)
    out = {}
    for name in R.ALL_WIDE:
        ref, low = R.grads64(name), R.grads(name, torch.float32)
        for k in R.TENSORS:
            out.update(grad_judge.pin_entries(name, ref, low, R.POSITIONS, [k]))
            print(f"{name} {k}: max {out[f'{name}_{k}_max']:.3g}, e_ref {out[f'{name}_{k}_e_ref']:.3g}")
        out.update(grad_judge.row_pin_entries(name, ref, [low], R.ROW_TENSORS))
        print(f"{name} loss: {float(ref['loss']):.9f} (fp32 {float(low['loss']):.9f})")
    grad_judge.write_npz(R.WIDE_PINS, out)


if __name__ == "__main__":
    main()
