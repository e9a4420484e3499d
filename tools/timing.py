"""The timing loop of the ``tools/*_times.py`` tables: HIP events, every variant warmed up, windows of back-to-back calls, the
variants taking turns window by window inside one process."""
import statistics

import torch


def window_ms(fn, reps):
    """ms per call over ``reps`` back-to-back calls, by HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(variants, windows, target_ms, probe=10, min_reps=10):
    """variants: name -> callable.  -> name -> (median, min, max ms per call over ``windows`` windows, calls per window).  Per
    variant: three warm-up calls, a window of ``probe`` calls that sizes the windows to fill ``target_ms`` (at least ``min_reps``
    calls), and one untimed window of that length to settle."""
    reps = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(min_reps, int(target_ms / max(window_ms(fn, probe), 1e-4)))
        window_ms(fn, reps[name])
    times = {name: [] for name in variants}
    for _ in range(windows):
        for name, fn in variants.items():                    # the variants take turns
            times[name].append(window_ms(fn, reps[name]))
    return {n: (statistics.median(v), min(v), max(v), reps[n]) for n, v in times.items()}
