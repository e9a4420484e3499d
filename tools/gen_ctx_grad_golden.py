"""Writes tests/golden/ctx_grad_pins.npz: what tests/ctx_grad_ref.py's float64 reference of the context-LSTM gradients gave when
this ran -- per case and tensor 64 sampled elements, the sum and the sum of squares, the largest magnitude -- and
``e_ref = max |G_ref32 - G_ref64|``, the error of the same ``torch.nn.LSTM`` (and, for ``chain``, of the same composition with the
CPC loss) run in fp32 on the CPU.  The judge of the tests is built from these alone.

    python tools/gen_ctx_grad_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ctx_grad_ref as R  # noqa: E402


def main():
    torch.set_num_threads(1)                                        # one summation order for the recorded fp32 error
    out = {}
    for name in R.ALL_CASES + [R.CHAIN]:
        ref = R.grads64(name)
        low = R.chain_grads(torch.float32) if name == R.CHAIN else R.torch_grads(name, torch.float32)
        for k, G in ref.items():
            out[f"{name}_{k}_samples"] = G.reshape(-1)[R.sample_positions(name, k, G.size)]
            out[f"{name}_{k}_sums"] = np.array([G.sum(), (G ** 2).sum()])
            out[f"{name}_{k}_max"] = np.float64(np.abs(G).max())
            out[f"{name}_{k}_e_ref"] = np.float64(np.abs(low[k] - G).max())
            print(f"{name} {k}: max {out[f'{name}_{k}_max']:.3g}, e_ref {out[f'{name}_{k}_e_ref']:.3g}")
    np.savez(R.PINS, **out)
    print(f"wrote {R.PINS} ({os.path.getsize(R.PINS)} bytes)")


if __name__ == "__main__":
    main()
