"""The measuring loop of the per-kernel tools (sddmm_kernels.py, row_softmax_kernels.py): everything runs in ONE process after
3 warm-up launches of every configuration; each launch sits between its own pair of device events; a figure is the median of
`reps` launches; `rounds` rounds, the configurations taking turns inside a round (the spread between the rounds of one
configuration is the noise).  A configuration is a name -> callable entry of a dict."""
import statistics

import torch

PEAK = 8.0e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def warm_up(fns):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()


def round_medians(fns, reps, rounds):
    """name -> [median ms of round 0, of round 1, ...]"""
    med = {k: [] for k in fns}
    for _ in range(rounds):
        ts = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():        # the configurations take turns
                ts[k].append(timed(fn))
        for k in fns:
            med[k].append(statistics.median(ts[k]))
    return med


def print_bandwidth(name, width, times, nbytes):
    """One line per configuration: per round its time and `nbytes` over it as a fraction of 8e12 B/s."""
    line = "  ".join(f"round {r}: {t:9.4f} ms  {nbytes / (t * 1e-3) / PEAK:6.3f} of 8 TB/s" for r, t in enumerate(times))
    print(f"   {name:{width}s} {line}")
