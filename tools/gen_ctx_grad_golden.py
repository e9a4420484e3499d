"""Writes the pins of tests/ctx_grad_ref.py's float64 reference of the context-LSTM gradients: per case and tensor 64 sampled
elements, the sum and the sum of squares, the largest magnitude -- and ``e_ref = max |G_ref32 - G_ref64|``, the error of the same
``torch.nn.LSTM`` (and, for ``chain``, of the same composition with the CPC loss) run in fp32 on the CPU.  The judges of the tests
are built from these alone.

tests/golden/ctx_grad_wide_pins.npz: the wide cases; for ``c`` and ``z`` also, per time step, ``max |G64[:, t]|`` and
``e_ref[t] = max |G32[:, t] - G64[:, t]|``, both (T,).  Written with fixed archive dates: the same bytes at every run.
tests/golden/ctx_grad_pins.npz: the nine cases and ``chain``; left as it is unless ``--nine`` is given.

    python tools/gen_ctx_grad_golden.py [--nine]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ctx_grad_ref as R  # noqa: E402
import grad_judge  # noqa: E402


def pins_of(names, per_step):
    out = {}
    for name in names:
        ref = R.grads64(name)
        low = R.chain_grads(torch.float32) if name == R.CHAIN else R.torch_grads(name, torch.float32)
        for k, G in ref.items():                                    # tensor by tensor: the archive keeps this order
            out.update(grad_judge.pin_entries(name, ref, low, R.POSITIONS, [k]))
            print(f"{name} {k}: max {out[f'{name}_{k}_max']:.3g}, e_ref {out[f'{name}_{k}_e_ref']:.3g}")
            if per_step and k in R.STEP_TENSORS:
                top, err = R.step_max(G), R.step_max(low[k] - G)
                out[f"{name}_{k}_step_max"], out[f"{name}_{k}_step_e_ref"] = top, err
                print(f"{name} {k} per step: max {top.min():.3g} .. {top.max():.3g}, e_ref {err.min():.3g} .. {err.max():.3g}")
    return out


def main():
    torch.set_num_threads(1)                                        # one summation order for the recorded fp32 error
    if "--nine" in sys.argv[1:]:
        out = pins_of(R.ALL_CASES + [R.CHAIN], per_step=False)
        np.savez(R.PINS, **out)
        print(f"wrote {R.PINS} ({os.path.getsize(R.PINS)} bytes)")
    grad_judge.write_npz(R.WIDE_PINS, pins_of(R.ALL_WIDE, per_step=True))


if __name__ == "__main__":
    main()
