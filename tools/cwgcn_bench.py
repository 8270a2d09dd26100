#!/usr/bin/env python
"""CWGCN at the DBLPv7 -> Citationv1 shapes of the reference's citation sheet (bench.make_cfg_a(ns=5484, es=8117,
nt=8935, et=15098): 6,775 bag-of-words features, hid 128, 5 classes, benchmark/node/run_citation.sh): steady-state
ms/epoch of stage 1 (source, correntropy loss) and stage 2 (target, mean / std matching), captured and eager
(epoch-hook stamps over the second half of each stage), the new kernels' HIP-event times over eager epochs with their
algorithmic bytes and fraction of the HBM peak, and UDAGCN's ms/epoch from bench.other_configs for comparison.  One
JSON line per result, also written to ``--out``.

    python tools/cwgcn_bench.py [--epochs 40] [--out profiles/cwgcn_dblp_citation_bench.jsonl]
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
from _trainer_bench import collector, steady_ms, write_jsonl  # noqa: E402

SHAPES = dict(seed=200, ns=5484, es=8117, nt=8935, et=15098)


def _model(src, epochs, dev, graphed):
    torch.manual_seed(0)
    np.random.seed(0)
    return pygda_amd.models.CWGCN(src.x.size(1), 128, 5, lr=0.0001, weight_decay=0.0001, device=dev, epoch=epochs,
                                  verbose=0, use_hip_graph=graphed)


def ms_per_epoch(src, tgt, graphed, epochs, dev):
    m = _model(src, epochs, dev, graphed)
    stamps = {1: [], 2: []}
    m.epoch_hook = lambda e, loss, acc, secs: stamps[m.stage].append((time.perf_counter(), loss, acc))
    m.fit(src, tgt)
    torch.cuda.synchronize()
    out = dict(requested="captured" if graphed else "eager")
    for stage, st in stamps.items():
        half = len(st) // 2              # warm-up: ingestion, sparse-feature registration, the capture
        out[f"stage{stage}_ms_per_epoch"] = steady_ms([s[0] for s in st], half)
        out[f"stage{stage}_epochs_timed"] = len(st) - half
        out[f"stage{stage}_final_loss"], out[f"stage{stage}_final_acc"] = st[-1][1], st[-1][2]
    del m
    gc.collect()
    torch.cuda.synchronize()
    return out


def kernels(src, tgt, dev, epochs=4):
    """HIP-event times of the CWGCN kernel families over eager epochs (stage-1 epochs 1.. and all of stage 2)."""
    m = _model(src, epochs, dev, False)
    seen = []
    m.epoch_hook = lambda e, loss, acc, secs: (seen.append(e), profiler.start() if (m.stage, e) == (1, 0) else None)
    m.fit(src, tgt)
    torch.cuda.synchronize()
    profiler.stop()
    prof = profiler.summary()
    out = {}
    names = dict(closs_fwd=0, closs_bwd=1, weighted_moments=2, match_fwd=3, match_bwd=4)
    for name, i in names.items():
        r = prof.get(name)
        if r is None:
            continue
        secs = r["ms"] * 1e-3
        out[name] = dict(us_per_call=1e3 * r["ms"] / r["calls"], calls=r["calls"], launches_per_call=r["launches"] / r["calls"],
                         bytes_per_call=r["bytes"] / r["calls"], hbm_frac=r["bytes"] / secs / 1e9 / bench.HBM_PEAK_GBS)
    out["step_kernels_ms_total"] = {k: v["ms"] for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:10]}
    del m
    gc.collect()
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cwgcn_dblp_citation_bench.jsonl"))
    ap.add_argument("--skip-udagcn", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    src, tgt = bench.make_cfg_a(**SHAPES)
    emit, lines = collector()
    ns, nt = src.x.size(0), tgt.x.size(0)
    names = ("closs_fwd", "closs_bwd", "weighted_moments", "match_fwd", "match_bwd")
    emit(dict(what="cwgcn_algorithmic_bytes", source_rows=ns, target_rows=nt, width=128, classes=5,
              **{k: v for k, v in zip(names[:3], ops.cwgcn_bytes(ns, 5, 128)[:3])},
              **{k: v for k, v in zip(names[3:], ops.cwgcn_bytes(nt, 5, 128)[3:])}))
    for graphed in (True, False):
        emit(dict(what="cwgcn_ms_per_epoch", **ms_per_epoch(src, tgt, graphed, a.epochs, dev)))
    emit(dict(what="cwgcn_kernels", **kernels(src, tgt, dev)))
    if not a.skip_udagcn:
        emit(dict(what="udagcn_ms_per_epoch_cfgA", **bench.other_configs(dev, epochs=a.epochs, which=("udagcn",))["udagcn"]))
    write_jsonl(a.out, lines, stamp=False)


if __name__ == "__main__":
    main()
