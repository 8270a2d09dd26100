#!/usr/bin/env python
"""JHGDA at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a: 9,360 / 5,484 nodes, 6,775 bag-of-words features,
hid 128, the trainer's defaults: pooled widths 1,872 / 374 / 74 and 1,096 / 219 / 43): steady-state ms/epoch, eager and
captured, the peak memory of a fit, and the level-0 proximity term alone at the source's shape (S [9,360, 1,872]):
the fused kernel's forward + backward (one launch sequence) in us from HIP events, its achieved TFLOP/s (4 N^2 K
flops) against the fp32 matrix-core peak, and the same term composed densely in torch on the device (S S^T, min,
logs, sums and the autograd backward).  The dense composition runs only here.  One JSON line per result, also
written to ``--out``.

    python tools/jhgda_bench.py [--epochs 12] [--out profiles/jhgda_acm_dblp_bench.jsonl]

``--pseudo gmm [--gmm-max-iter 100]`` times the fits with the mixture pseudo-labels, adds each epoch's kept ``n_iter``
and counts the launches of one eager epoch; ``--skip-prox`` leaves the proximity term's lines out.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops  # noqa: E402
from _trainer_bench import collector, events, steady_ms, write_jsonl  # noqa: E402

DEV = "cuda:0"
FP32_MATRIX_PEAK_TFLOPS = 157.3      # MI355X dense fp32 matrix-core peak (AMD's published figure)


def _fit_ms(src, tgt, epochs, graph, **kw):
    m = pygda_amd.models.JHGDA(src.x.size(1), 128, int(src.y.max()) + 1, device=DEV, epoch=epochs, verbose=0,
                               use_hip_graph=graph, **kw)
    stamps = []
    m.epoch_hook = lambda e, loss, acc, secs: stamps.append((secs, loss))
    torch.manual_seed(0)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.fit(src, tgt)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = steady_ms([s[0] for s in stamps], 4 if epochs > 8 else 1)      # the first replay holds the capture
    U = m.epochs_per_graph if graph else 1
    ends = [s[0] for s in stamps][U - 1::U]                             # one read-back per replay (or eager epoch)
    steps = sorted((b - a) / U * 1e3 for a, b in zip(ends[1:], ends[2:]))
    m.median_ms = steps[len(steps) // 2] if steps else ms
    return ms, peak, stamps[-1][1], m


def _launches(src, tgt, **kw):
    """Launches of the project's kernels in one eager epoch, all and the mixture's alone (profiler regions)."""
    from pygda_amd import profiler
    m = pygda_amd.models.JHGDA(src.x.size(1), 128, int(src.y.max()) + 1, device=DEV, epoch=1, verbose=0,
                               use_hip_graph=False, **kw)
    torch.manual_seed(0)
    profiler.start()
    m.fit(src, tgt)
    torch.cuda.synchronize()
    profiler.stop()
    summ = profiler.summary()
    mix = {k: v for k, v in summ.items() if k.startswith(("gmm_", "lsa_"))}
    return (sum(v["launches"] for v in summ.values()), sum(v["launches"] for v in mix.values()),
            round(sum(v["ms"] for v in mix.values()), 3))


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jhgda_acm_dblp_bench.jsonl"))
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--skip-prox", action="store_true")
    ap.add_argument("--pseudo", default="classifier", choices=("classifier", "gmm"))
    ap.add_argument("--gmm-max-iter", type=int, default=100)
    a = ap.parse_args(argv)
    if a.skip_prox:
        return _fits(a, *collector())
    emit, lines = collector()
    n, k = 9360, 1872
    g = torch.Generator().manual_seed(0)
    S = torch.softmax(torch.randn(n, k, generator=g) * 4, dim=1).to(DEV).requires_grad_(True)
    src, tgt = bench.make_cfg_a()
    ei = src.edge_index.to(DEV)
    edges = ops.JhgdaEdges(ei, n)

    def fused():
        torch.autograd.grad(ops.jhgda_prox(ei, S, edges), S)

    def dense():
        p = torch.min(S @ S.T, torch.ones(1, device=DEV))
        pos, neg = torch.log(p + 1e-7), torch.log(1 - p + 1e-7)
        loss = (-torch.sum(pos[ei[0], ei[1]]) - (torch.sum(neg) - torch.sum(neg[ei[0], ei[1]]))) / float(n * n)
        torch.autograd.grad(loss, S)

    us = events(fused, 5, rounds=None)
    flops = 4.0 * n * n * k
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fused()
    torch.cuda.synchronize()
    fused_peak = torch.cuda.max_memory_allocated() - base
    us_dense = events(dense, 5, rounds=None)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dense()
    torch.cuda.synchronize()
    dense_peak = torch.cuda.max_memory_allocated() - base
    emit(dict(what="jhgda_prox_level0", n=n, k=k, fused_fwd_bwd_us=round(us, 1), dense_torch_fwd_bwd_us=round(us_dense, 1),
              fused_tflops=round(flops / us / 1e6, 2), fp32_matrix_peak_tflops=FP32_MATRIX_PEAK_TFLOPS,
              share_of_peak=round(flops / us / 1e6 / FP32_MATRIX_PEAK_TFLOPS, 3),
              fused_peak_mib=round(fused_peak / 2**20, 1), dense_peak_mib=round(dense_peak / 2**20, 1)))
    del S
    _fits(a, emit, lines)


def _fits(a, emit, lines):
    if not a.skip_fit:
        src, tgt = (pygda_amd.data.Data(x=d.x.to(DEV), edge_index=d.edge_index.to(DEV), y=d.y.to(DEV))
                    for d in bench.make_cfg_a())
        kw = dict(pseudo="gmm", gmm_max_iter=a.gmm_max_iter) if a.pseudo == "gmm" else {}
        for graph in (False, True):
            _fit_ms(src, tgt, a.epochs, graph, **kw)                  # the first fit warms workspaces and code objects
            ms, peak, loss, m = _fit_ms(src, tgt, a.epochs, graph, **kw)
            line = dict(what="jhgda_epoch", captured=graph, ms_per_epoch=round(ms, 2),
                        median_ms_per_epoch=round(m.median_ms, 2),
                        fit_peak_mib=round(peak / 2**20, 1), last_loss=loss, epochs=a.epochs)
            if a.pseudo == "gmm":
                line.update(pseudo="gmm", gmm_max_iter=a.gmm_max_iter, n_iter=[e[0] for e in m.gmm_log],
                            fell_back=sum(e[2] for e in m.gmm_log))
            emit(line)
        if a.pseudo == "gmm":
            every, mix, mix_ms = _launches(src, tgt, **kw)
            emit(dict(what="jhgda_epoch_launches", pseudo="gmm", gmm_max_iter=a.gmm_max_iter, project_kernel_launches=every,
                      mixture_launches=mix, mixture_eager_ms=mix_ms))
    write_jsonl(a.out, lines)


if __name__ == "__main__":
    main(sys.argv[1:])
