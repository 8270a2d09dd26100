#!/usr/bin/env python
"""KBL at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a with 7,410 / 5,578 nodes, 6,775 bag-of-words features,
5 classes, embeddings of width 128, ``k_cross=20``), times over steady-state repetitions after a warm-up:

- the bridge top-k on the kernels (``ops.kbl_bridge_topk``) against the reference's formulation in torch on the same
  GPU -- the cosine a chunk of rows at a time, the sigmoid, a flat ``topk`` per chunk joined to the running one --
  and against the reference's literal form (the full ``[N_src, N_tar]`` array, one flat ``topk``), with the peak
  device memory each of the three allocates;
- the pair loss with its gradient (``ops.kbl_pair_bce``, two lists of 200) against the torch composition on the same GPU
  (the two ``[40000, 128]`` gathers, ``cosine_similarity``, the sigmoid, ``binary_cross_entropy``);
- ms per bridge epoch and per classifier epoch, eager and captured, from the epoch hook's stamps.

The torch compositions are the yardsticks and run only here.  One JSON line per result, also written to ``--out``.

    python tools/kbl_bench.py [--epochs 40] [--out profiles/kbl_acm_dblp_bench.jsonl]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops  # noqa: E402
from _trainer_bench import collector, events as _events, steady_ms, write_jsonl  # noqa: E402

DEV = "cuda:0"
NS, NT, D, K = 7410, 5578, 128, 20


def _fit_stamps(src, tgt, epochs, graph):
    m = pygda_amd.models.KBL(src.x.size(1), 128, 5, k_cross=K, device=DEV, epoch=epochs, bridge_epochs=epochs, verbose=0,
                             use_hip_graph=graph)
    stamps = []
    m.epoch_hook = lambda e, loss, acc, secs: stamps.append((secs, loss, acc))
    torch.manual_seed(0)
    np.random.seed(0)
    ops.dropout_state.counter(torch.device(DEV)).zero_()     # the keep-bit stream restarts: both fits draw the same masks
    m.fit(src, tgt)
    torch.cuda.synchronize()
    bridge = [s[0] for s in stamps if s[2] is None]
    gnn = [s[0] for s in stamps if s[2] is not None]
    skip = 8 if epochs > 12 else 1
    return steady_ms(bridge, skip), steady_ms(gnn, skip), stamps[-1][1]


def _torch_topk_full(a, b, k):
    """The reference's literal form: the whole ``[na, nb]`` array of sigmoid(cos), one flat ``topk``."""
    ah = a / a.norm(dim=1, keepdim=True).clamp_min(1e-8)
    bh = b / b.norm(dim=1, keepdim=True).clamp_min(1e-8)
    val, flat = torch.sigmoid(ah @ bh.t()).view(-1).topk(k)
    return flat // b.size(0), flat % b.size(0), val


def _torch_topk_chunked(a, b, k, rows=1000):
    """The same a chunk of rows at a time (the reference's ``bridge_batch_size`` is 1000): a flat ``topk`` per chunk,
    joined to the running one."""
    ah = a / a.norm(dim=1, keepdim=True).clamp_min(1e-8)
    bh = b / b.norm(dim=1, keepdim=True).clamp_min(1e-8)
    val = torch.empty(0, device=a.device)
    flat = torch.empty(0, dtype=torch.long, device=a.device)
    for i0 in range(0, a.size(0), rows):
        v, f = torch.sigmoid(ah[i0:i0 + rows] @ bh.t()).view(-1).topk(k)
        val, flat = torch.cat([val, v]), torch.cat([flat, f + i0 * b.size(0)])
        val, keep = val.topk(k)
        flat = flat[keep]
    return flat // b.size(0), flat % b.size(0), val


def _peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kbl_acm_dblp_bench.jsonl"))
    a = ap.parse_args(argv)
    emit, lines = collector()
    g = torch.Generator().manual_seed(0)
    us_, ut_ = torch.randn(NS, D, generator=g).to(DEV), torch.randn(NT, D, generator=g).to(DEV)
    paths = (("kernels", lambda: ops.kbl_bridge_topk(us_, ut_, K)),
             ("torch_row_chunked_on_gpu", lambda: _torch_topk_chunked(us_, ut_, K)),
             ("torch_full_array_on_gpu", lambda: _torch_topk_full(us_, ut_, K)))
    want = set(zip(*(v.tolist() for v in _torch_topk_full(us_, ut_, K)[:2])))
    for path, fn in paths:
        assert set(zip(*(v.tolist() for v in fn()[:2]))) == want, path
        us, spread = _events(fn, 10)
        emit(dict(what="bridge_topk", path=path, us=us, spread_us=spread, peak_bytes=_peak_bytes(fn), na=NS, nb=NT, d=D, k=K))
    u = torch.randn(NS, D, generator=g).to(DEV).requires_grad_(True)
    y = torch.randint(0, 5, (NS,), generator=g).to(DEV)
    ia, ib = (torch.randint(0, NS, (200,), generator=g).to(DEV) for _ in range(2))
    for path, fn in (("kernels", ops.kbl_pair_bce), ("torch_composition_on_gpu", ops._kbl_pair_bce_host)):
        run = lambda fn=fn: torch.autograd.grad(fn(u, ia, ib, y), [u])
        us, spread = _events(run, 10)
        emit(dict(what="pair_bce_with_gradient", path=path, us=us, spread_us=spread, peak_bytes=_peak_bytes(run), n=NS, d=D,
                  ma=200, mb=200))
    src, tgt = bench.make_cfg_a(ns=NS, nt=NT)
    src.train_mask = torch.ones(NS, dtype=torch.bool)
    for graph in (False, True):
        bridge, gnn, loss = _fit_stamps(src, tgt, a.epochs, graph)
        emit(dict(what="kbl_fit", captured=graph, ms_per_bridge_epoch=round(bridge, 3), ms_per_classifier_epoch=round(gnn, 3),
                  last_loss=loss, epochs=a.epochs))
    write_jsonl(a.out, lines)


if __name__ == "__main__":
    main(sys.argv[1:])
