"""What the trainers' ``tools/*_bench.py`` scripts share: the HIP-event timer, the emit-and-collect closure, the JSONL
writer, the epoch-hook stamps -> ms per epoch rule and the timed fit of a source-free trainer."""
import json
import os
import statistics
import time

import numpy as np
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


def source_free_fit_stamps(cls, src, tgt, epochs, graph, device="cuda:0", **kw):
    """``(ms per pretraining epoch, ms per adaptation iteration, last adaptation loss)`` of one fit of the
    graph-transformation trainer ``cls`` at hidden width 128 and 5 classes, from the epoch hook's stamps (an adaptation
    line carries no accuracy).  The once-per-fit final sampling is not what is timed: it is replaced on the instance."""
    m = cls(src.x.size(1), 128, 5, device=device, epoch=epochs, verbose=0, use_hip_graph=graph, **kw)
    stamps = []
    m.epoch_hook = lambda e, loss, acc, secs: stamps.append((secs, loss, acc))
    torch.manual_seed(0)
    np.random.seed(0)
    real = m.sample_final_edges
    m.sample_final_edges = lambda *a, **k: (tgt.edge_index.to(device), torch.ones(tgt.edge_index.size(1), device=device))
    m.fit(src, tgt)
    m.sample_final_edges = real
    torch.cuda.synchronize()
    pre = [s[0] for s in stamps if s[2] is not None]
    ada = [s for s in stamps if s[2] is None]
    return steady_ms(pre, 8 if len(pre) > 12 else 1), steady_ms([s[0] for s in ada], 4 if len(ada) > 6 else 1), ada[-1][1]
