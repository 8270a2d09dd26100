"""What the trainers' ``tools/*_bench.py`` scripts share: the HIP-event timer, the emit-and-collect closure, the JSONL
writer and the epoch-hook stamps -> ms per epoch rule."""
import json
import os
import statistics
import time

import torch


def events(fn, reps, rounds=5):
    """Median and spread (min, max) in us of ``rounds`` timings of ``reps`` back-to-back calls after one warm-up call,
    rounded to 0.1 us; ``rounds=None``: one such timing, in us, as measured."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds or 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    if rounds is None:
        return out[0]
    return round(statistics.median(out), 1), [round(min(out), 1), round(max(out), 1)]


def collector():
    """``(emit, lines)``: ``emit(d)`` prints ``d`` as one JSON line and appends it to ``lines``."""
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    return emit, lines


def write_jsonl(path, lines, stamp=True, mode="w"):
    """``lines`` as JSON lines into ``path`` (nothing when it is empty), each with today's date when ``stamp``."""
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, mode) as fh:
        for d in lines:
            fh.write(json.dumps(dict(d, stamp=time.strftime("%Y-%m-%d")) if stamp else d) + "\n")


def steady_ms(times, skip):
    """ms per epoch from the epoch hook's stamps ``times`` (seconds, one per epoch): from stamp ``skip - 1`` -- the
    epochs before it hold the warm-up and the capture -- to the last."""
    return (times[-1] - times[skip - 1]) / (len(times) - skip) * 1e3
