#!/usr/bin/env python
"""ACDNE at the DBLPv7 -> Citationv1 shapes of the reference's citation sheet (bench.make_cfg_a(ns=5484, es=8117,
nt=8935, et=15098): 6,775 bag-of-words features; benchmark/node/run_citation.sh: hid 128, lr 1e-3, wd 1e-3,
dropout 0.5, the default batch_size 100): process_graph on the device (both domains) against the reference's numpy
lines restated here (source domain), steady-state ms/epoch captured and eager (epoch-hook stamps over the second half;
an epoch includes its predict over the source rows, as the reference's does), and the kernels' HIP-event times with
their algorithmic bytes.  One JSON line per result, also written to ``--out``.

    python tools/acdne_bench.py [--epochs 8] [--out profiles/acdne_dblp_citation_bench.jsonl] [--skip-numpy]
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


def numpy_process_graph(edge_index, x, n, step=3):
    """The reference's process_graph lines (pygda/models/acdne.py: to_dense_adj, my_scale_sim_mat,
    agg_tran_prob_mat with dense np.matmul, compute_ppmi, X_nei = n_A_ppmi @ X) as numpy 2 runs them."""
    import scipy.sparse as sp
    adj = np.zeros((n, n), dtype=np.float32)
    np.add.at(adj, (edge_index[0], edge_index[1]), 1)

    def scale(w):
        rowsum = np.array(np.sum(w, axis=1), dtype=np.float32)
        r_inv = np.power(rowsum + 1e-12, -1).flatten()
        r_inv[np.isinf(r_inv)] = 0.
        return sp.diags(r_inv).dot(w)

    g = np.asarray(scale(sp.csc_matrix(adj)).toarray())
    a_k, a = g, g
    for k in np.arange(2, step + 1):
        a_k = np.matmul(a_k, g)
        a = a + a_k / k
    np.fill_diagonal(a, 0)
    a = scale(a)
    col = np.sum(a, axis=0)
    col[col == 0] = 1
    ppmi = np.log((float(n) * a) / col[None, :] + 1e-12)
    ppmi[np.isnan(ppmi)] = 0
    ppmi[ppmi < 0] = 0
    return ppmi, np.matmul(scale(ppmi), x)


def _model(src, epochs, dev, graphed):
    return pygda_amd.models.ACDNE(src.x.size(1), 128, 5, dropout=0.5, weight_decay=1e-3, lr=1e-3, device=dev,
                                  epoch=epochs, verbose=0, use_hip_graph=graphed)


def preprocessing(src, tgt, dev):
    out = {}
    for name, d in (("source", src), ("target", tgt)):
        n = d.x.size(0)
        x, ei = d.x.to(dev), d.edge_index.to(dev)
        ops.acdne_process_graph(ei, x, n, 3)                     # warm-up (first launches, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, xn = ops.acdne_process_graph(ei, x, n, 3)
        torch.cuda.synchronize()
        out[f"{name}_nodes"] = n
        out[f"{name}_device_ms"] = (time.perf_counter() - t0) * 1e3
        profiler.start()
        ops.acdne_process_graph(ei, x, n, 3)
        torch.cuda.synchronize()
        profiler.stop()
        for k, r in profiler.summary().items():
            out[f"{name}_{k}_ms"] = r["ms"]
            out[f"{name}_{k}_bytes"] = r["bytes"]
        del a, xn
        torch.cuda.empty_cache()
    return out


def ms_per_epoch(src, tgt, graphed, epochs, dev):
    torch.manual_seed(0)
    np.random.seed(0)
    m = _model(src, epochs, dev, graphed)
    st = []
    m.epoch_hook = lambda e, loss, acc, secs: st.append((time.perf_counter(), loss, acc))
    m.fit(src, tgt)
    torch.cuda.synchronize()
    half = len(st) // 2
    out = dict(requested="captured" if graphed else "eager",
               ms_per_epoch=steady_ms([s[0] for s in st], half), epochs_timed=len(st) - half,
               steps_per_epoch=round(max(src.x.size(0), tgt.x.size(0)) / 50), final_loss=st[-1][1],
               final_acc=st[-1][2])
    del m
    gc.collect()
    torch.cuda.synchronize()
    return out


def kernels(src, tgt, dev, epochs=2):
    torch.manual_seed(0)
    np.random.seed(0)
    m = _model(src, epochs, dev, False)
    m.epoch_hook = lambda e, loss, acc, secs: profiler.start() if e == 0 else None
    m.fit(src, tgt)
    torch.cuda.synchronize()
    profiler.stop()
    prof = profiler.summary()
    out = {}
    for name in ("acdne_prox", "acdne_heads"):
        r = prof.get(name)
        if r is None:
            continue
        secs = r["ms"] * 1e-3
        out[name] = dict(us_per_call=1e3 * r["ms"] / r["calls"], calls=r["calls"], bytes_per_call=r["bytes"] / r["calls"],
                         hbm_frac=r["bytes"] / secs / 1e9 / bench.HBM_PEAK_GBS)
    out["step_kernels_ms_total"] = {k: v["ms"] for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:10]}
    del m
    gc.collect()
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acdne_dblp_citation_bench.jsonl"))
    ap.add_argument("--skip-numpy", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    src, tgt = bench.make_cfg_a(**SHAPES)
    emit, lines = collector()
    emit(dict(what="acdne_preprocessing", **preprocessing(src, tgt, dev)))
    if not a.skip_numpy:
        t0 = time.perf_counter()
        numpy_process_graph(src.edge_index.numpy(), src.x.numpy(), src.x.size(0))
        emit(dict(what="acdne_reference_numpy_process_graph", nodes=src.x.size(0),
                  seconds=time.perf_counter() - t0, threads=os.environ.get("OMP_NUM_THREADS")))
    for graphed in (True, False):
        emit(dict(what="acdne_ms_per_epoch", **ms_per_epoch(src, tgt, graphed, a.epochs, dev)))
    emit(dict(what="acdne_kernels", **kernels(src, tgt, dev)))
    write_jsonl(a.out, lines, stamp=False)


if __name__ == "__main__":
    main()
