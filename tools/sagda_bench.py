#!/usr/bin/env python
"""SAGDA at the cfg-A shapes (bench.make_cfg_a: 9,360 / 5,484 nodes, 6,775 bag-of-words features), hid 128, adv_dim 40,
num_layers 1 and 2: steady-state ms/epoch of the captured and of the eager step (epoch-hook stamps, each behind a
device synchronisation), the FAConv kernels' HIP-event times over eager epochs with their algorithmic bytes and
fraction of the HBM peak, and UDAGCN's ms/epoch from bench.other_configs in the same process.  One JSON line per
result; ``--out FILE`` also writes them there.

    python tools/sagda_bench.py [--epochs 40] [--out profiles/sagda_cfgA_bench.jsonl]
"""
import argparse
import gc
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops, profiler  # noqa: E402
from _trainer_bench import collector, write_jsonl  # noqa: E402


def ms_per_epoch(src, tgt, layers, graphed, epochs, dev):
    torch.manual_seed(0)
    np.random.seed(0)
    m = pygda_amd.models.SAGDA(src.x.size(1), 128, 5, num_layers=layers, adv_dim=40, device=dev, epoch=epochs,
                               verbose=0, use_hip_graph=graphed)
    stamps = []
    m.epoch_hook = lambda e, loss, acc, secs: stamps.append((time.perf_counter(), loss))
    m.fit(src, tgt)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    half = len(stamps) // 2          # warm-up: ingestion, the PPMI walk, sparse-feature registration, the capture
    ms = (t1 - stamps[half - 1][0]) / (len(stamps) - half) * 1e3
    path = "hipGraph replay" if getattr(m, "_graphed", None) is not None else "eager launches"
    out = dict(num_layers=layers, requested="captured" if graphed else "eager", execution=path, ms_per_epoch=ms,
               epochs_timed=len(stamps) - half, final_loss=stamps[-1][1])
    del m
    gc.collect()
    torch.cuda.synchronize()
    return out


def faconv_kernels(src, tgt, layers, dev, epochs=4):
    """HIP-event times of the FAConv families over eager epochs 1.. (epoch 0 builds the graphs)."""
    torch.manual_seed(0)
    np.random.seed(0)
    m = pygda_amd.models.SAGDA(src.x.size(1), 128, 5, num_layers=layers, adv_dim=40, device=dev, epoch=epochs,
                               verbose=0, use_hip_graph=False)
    seen = []
    m.epoch_hook = lambda e, loss, acc, secs: (seen.append(e), profiler.start() if e == 0 else None)
    m.fit(src, tgt)
    torch.cuda.synchronize()
    profiler.stop()
    prof = profiler.summary()
    n_ep = max(len(seen) - 1, 1)
    out = {}
    for name in ("faconv_fwd", "faconv_bwd"):
        r = prof.get(name)
        if r is None:
            continue
        secs = r["ms"] * 1e-3
        out[name] = dict(us_per_call=1e3 * r["ms"] / r["calls"], calls_per_epoch=r["calls"] / n_ep,
                         bytes_per_call=r["bytes"] / r["calls"],
                         hbm_frac=r["bytes"] / secs / 1e9 / bench.HBM_PEAK_GBS)
    out["step_kernels_ms_per_epoch"] = {k: v["ms"] / n_ep for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:8]}
    del m
    gc.collect()
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-udagcn", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    src, tgt = bench.make_cfg_a()
    emit, lines = collector()
    ns, nnz = src.x.size(0), src.edge_index.size(1) + src.x.size(0)
    fwd, bwd = ops.faconv_bytes(ns, nnz, 128)
    emit(dict(what="faconv_algorithmic_bytes", rows=ns, csr_entries=nnz, width=128, fwd_bytes=fwd, bwd_bytes=bwd,
              reference_order_fwd_gather_bytes=4 * nnz * src.x.size(1)))
    for layers in (1, 2):
        for graphed in (True, False):
            emit(dict(what="sagda_ms_per_epoch", **ms_per_epoch(src, tgt, layers, graphed, a.epochs, dev)))
        emit(dict(what="faconv_kernels", num_layers=layers, **faconv_kernels(src, tgt, layers, dev)))
    if not a.skip_udagcn:
        emit(dict(what="udagcn_ms_per_epoch", **bench.other_configs(dev, epochs=a.epochs, which=("udagcn",))["udagcn"]))
    write_jsonl(a.out, lines, stamp=False)


if __name__ == "__main__":
    main()
