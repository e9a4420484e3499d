#!/usr/bin/env python3
"""Generate tests/golden/warmup_lrs.json from the REFERENCE's own scheduler (runs in the build container only).

Imports the reference's ``scheduler.py`` (beside its ``model.py``, found as ``tools/gen_golden.py`` finds it), drives its
``WarmupScheduler`` over a plain SGD optimizer -- the schedule reads and writes ``group["lr"]`` only -- and records DATA: per case
the constructor arguments, the epochs looked at, the learning rate each of those epochs runs at (``group["lr"]`` before the
scheduler's step that ends it) and the scalars of the scheduler's ``state_dict()`` at the end.  The ``resume`` case saves both
state dicts mid-run into a fresh optimizer and scheduler, as the reference's checkpoints do (``train_cpc.py:17-33``), and goes on.

tests/test_adam_cpu.py holds ``optim.WarmupScheduler`` to these numbers within 1e-15 relative.

Usage:  python tools/gen_sched_golden.py            (writes tests/golden/warmup_lrs.json)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "warmup_lrs.json")

# name -> (warmup_epochs, initial_lr, max_lr, milestones, gamma), epochs run, epochs kept (None: all), resume after (None: never)
CASES = {
    "example": ((5, 1e-6, 4e-4, [8, 12], 0.25), 20, None, None),
    "config": ((150, 1e-5, 4e-4, [20000], 0.25), 20004, list(range(160)) + list(range(19997, 20004)), None),
    "repeated_milestone": ((2, 1e-4, 1e-3, [4, 4, 7], 0.5), 10, None, None),
    "resume": ((5, 1e-6, 4e-4, [8, 12], 0.25), 16, None, 7),
}


def scalars(sched):
    sd = sched.state_dict()
    return {"last_epoch": sd["last_epoch"], "_step_count": sd["_step_count"], "_last_lr": list(sd["_last_lr"]),
            "base_lrs": list(sd["base_lrs"]), "warmup_epochs": sd["warmup_epochs"], "gamma": sd["gamma"],
            "milestones": {str(k): v for k, v in sorted(sd["milestones"].items())}}


def main():
    import_reference()
    import scheduler as ref                                   # the reference's scheduler.py
    print("reference scheduler imported from", ref.__file__, "| torch", torch.__version__)
    out = {"torch": torch.__version__, "cases": {}}
    for name, (args, n_epochs, kept, resume_after) in CASES.items():
        def make():
            opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=args[1])     # train_cpc.py:55: lr = initial_lr
            return opt, ref.WarmupScheduler(opt, *args)

        opt, sched = make()
        lrs, mid = [], None
        for e in range(n_epochs):
            if resume_after is not None and e == resume_after:
                mid = scalars(sched)
                saved = {"optimizer": opt.state_dict(), "scheduler": sched.state_dict()}
                opt, sched = make()
                opt.load_state_dict(saved["optimizer"])
                sched.load_state_dict(saved["scheduler"])
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
        epochs = list(range(n_epochs)) if kept is None else kept
        out["cases"][name] = {"args": list(args), "n_epochs": n_epochs, "epochs": epochs, "lrs": [lrs[e] for e in epochs],
                              "resume_after": resume_after, "state_at_resume": mid, "state_at_end": scalars(sched)}
        print(name, "first lrs", lrs[:8], "last", lrs[-1])
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
