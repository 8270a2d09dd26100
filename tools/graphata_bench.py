#!/usr/bin/env python
"""GraphATA at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a with 7,410 / 5,578 nodes, 6,775 bag-of-words
features, 5 classes, ``S = 2`` sources, hidden width 128, two layers, ``K = 10``), medians over steady-state repetitions
after a warm-up:

- each new op on the kernels against its torch composition on the same GPU (``host=True``: the reference's expressions
  on device tensors), with the peak device memory both allocate: the gate, the blend with its backward, the head loss
  with its gradient, the neighbours and the vote (``ops.cta_knn`` on normalised rows + ``ops.ata_vote`` against the
  ``[N, N]`` cosine array, ``topk`` and the gathered mean), the memory update;
- one adaptation epoch of the trainer, eager and replayed from a hipGraph, from the epoch hook's stamps, against the
  same step composed from torch ops on the same GPU: the reference's layer (two edge-wise aggregations, ``2 S + 1``
  projections per layer), ``S`` GCN classifiers, the losses, the ``[N, N]`` array, torch's Adam, the eval pass and the
  memory update.  The composed step is timed the same way -- host wall-clock stamps behind one read-back of the loss
  per epoch, the first epochs left out -- and, beside that, with HIP events.

The torch compositions are the yardsticks and run only here.  One JSON line per result, also written to ``--out``.

    python tools/graphata_bench.py [--epochs 40] [--out profiles/graphata_acm_dblp_bench.jsonl]
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops  # noqa: E402
from pygda_amd.data import Data  # noqa: E402
from pygda_amd.nn.pagerank import host_gcn_graph  # noqa: E402
from _trainer_bench import collector, events as _events, steady_ms, write_jsonl  # noqa: E402

DEV = "cuda:0"
NS, NT, H, C, S, K = 7410, 5578, 128, 5, 2, 10


def _peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _fit(sources, tgt, epochs, graph):
    m = pygda_amd.models.GraphATA(tgt.x.size(1), H, C, S, K=K, num_layers=2, device=DEV, epoch=epochs, verbose=0,
                                  use_hip_graph=graph)
    stamps = []
    m.epoch_hook = lambda e, loss, acc, secs: stamps.append((secs, loss, m._phase))
    torch.manual_seed(0)
    ops.dropout_state.counter(torch.device(DEV)).zero_()
    m.fit(sources, tgt)
    torch.cuda.synchronize()
    ada = [s for s in stamps if s[2] == "target"]
    return m, steady_ms([s[0] for s in ada], 8 if len(ada) > 12 else 1), ada[-1][1]


def _wall_ms(step, epochs, skip):
    """ms per epoch of ``step`` by the trainer's own rule: a stamp behind each epoch's read-back of its loss."""
    stamps, start = [], time.time()
    for _ in range(epochs):
        step().item()
        stamps.append(time.time() - start)
    return steady_ms(stamps, skip)


class TorchStep:
    """One adaptation epoch of the reference's lines in torch on device tensors, on a trained trainer's modules."""

    def __init__(self, m, tgt):
        self.m, self.x, self.ei, self.y = m, tgt.x.to(DEV), tgt.edge_index.to(DEV), tgt.y.to(DEV)
        row, col, norm = host_gcn_graph(tgt.edge_index.cpu(), NT, torch.float32)
        self.gcn = (row.to(DEV), col.to(DEV), norm.to(DEV))
        self.mem_fea, self.mem_cls = m.mem_fea.clone(), m.mem_cls.clone()
        params = [p for net in m.source_model_list for p in net.parameters()] + list(m.graphata.parameters())
        self.opt = torch.optim.Adam(params, lr=m.lr)

    def forward(self):
        net, (row, col, norm) = self.m.graphata, self.gcn
        x = self.x
        for i, conv in enumerate(net.convs):
            x = conv._host_forward(x, self.ei)
            if i < len(net.convs) - 1:
                x = F.relu(x)
        Z = torch.stack([torch.zeros(NT, C, device=DEV).index_add_(0, col, norm[:, None] * F.linear(x, s.cls.lin.weight)[row])
                         + s.cls.bias for s in self.m.source_model_list])
        return x, Z

    def __call__(self):
        att = self.m.graphata.cls.att
        feat, Z = self.forward()
        with torch.no_grad():
            distance = F.normalize(feat, dim=1) @ F.normalize(self.mem_fea, dim=1).T          # the [N, N] array
            _, idx_near = torch.topk(distance, dim=-1, largest=True, k=K + 1)
            pred = ops.ata_vote(idx_near, self.mem_cls, host=True)
        loss, _, _ = ops.ata_head_loss(Z, att, pred, host=True)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        with torch.no_grad():
            feat, Z = self.forward()
            ops.ata_memory_update(ops.ata_head_loss(Z, att, host=True), feat, self.mem_cls, self.mem_fea, self.m.momentum,
                                  host=True)
        return loss


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graphata_acm_dblp_bench.jsonl"))
    a = ap.parse_args(argv)
    emit, lines = collector()
    g = torch.Generator().manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(DEV)                               # noqa: E731
    shape = dict(n=NT, h=H, c=C, s=S, k=K)

    def both(what, fn, reps=10, **extra):
        for path, host in (("kernels", False), ("torch_composition_on_gpu", True)):
            run = lambda host=host: fn(host)                                                     # noqa: E731
            us, spread = _events(run, reps)
            emit(dict(what=what, path=path, us=us, spread_us=spread, peak_bytes=_peak_bytes(run), **shape, **extra))

    nr, gy = rnd(NT, H).requires_grad_(True), rnd(NT, H)
    both("gate_with_gradient", lambda host: torch.autograd.grad(ops.ata_gate(nr, host=host), [nr], gy))
    P, Q, sc = rnd(NT, S * H).requires_grad_(True), rnd(NT, H).requires_grad_(True), rnd(NT, S).requires_grad_(True)
    both("mix_with_gradient", lambda host: torch.autograd.grad(ops.ata_mix(P, Q, sc, 0.2, host=host)[0], [P, Q, sc], gy))
    Z, att = rnd(S, NT, C).requires_grad_(True), rnd(C).requires_grad_(True)
    pred = torch.randint(0, C, (NT,), generator=g).to(DEV)
    both("head_loss_with_gradient", lambda host: torch.autograd.grad(ops.ata_head_loss(Z, att, pred, host=host)[0], [Z, att]))
    feat, mem_fea = rnd(NT, H), torch.rand(NT, H, generator=g).to(DEV)
    mem_cls = torch.softmax(rnd(NT, C), dim=1)

    def vote(host):
        fn_, mn_ = F.normalize(feat, dim=1), F.normalize(mem_fea, dim=1)
        if host:
            _, idx = torch.topk(fn_ @ mn_.T, dim=-1, largest=True, k=K + 1)
        else:
            idx, _ = ops.cta_knn(fn_, mn_, K + 1)
        return ops.ata_vote(idx, mem_cls, host=host)

    assert torch.equal(vote(False).long(), vote(True))
    both("neighbours_and_vote", vote)
    logits = rnd(NT, C)
    both("memory_update", lambda host: ops.ata_memory_update(logits, feat, mem_cls, mem_fea, 0.9, host=host))

    src, tgt = bench.make_cfg_a(ns=NS, nt=NT)
    other = Data(x=src.x, edge_index=src.edge_index,
                 y=torch.randint(0, C, (NS,), generator=torch.Generator().manual_seed(1)).to(src.y.device))
    for captured in (False, True):
        m, ms, loss = _fit([src, other], tgt, a.epochs, captured)
        emit(dict(what="graphata_adaptation_epoch", path="trainer", captured=captured, ms_per_epoch=round(ms, 3),
                  last_loss=loss, epochs=a.epochs, **shape))
    step = TorchStep(m, tgt)
    us, spread = _events(step, 5, rounds=5)
    emit(dict(what="graphata_adaptation_epoch", path="torch_composition_on_gpu",
              ms_per_epoch=round(_wall_ms(step, a.epochs, 8 if a.epochs > 12 else 1), 3), epochs=a.epochs,
              ms_per_epoch_hip_events=round(us / 1e3, 3), spread_ms_hip_events=[round(v / 1e3, 3) for v in spread],
              peak_bytes=_peak_bytes(step), **shape))
    t = Data(x=tgt.x.to(DEV), edge_index=tgt.edge_index.to(DEV), y=tgt.y.to(DEV))
    dom = m._dom(t, torch.device(DEV))
    m.epoch = 1
    m._slots(parts=(4,))
    m._loss_buf = torch.zeros(1, device=DEV)
    m._hit_buf = torch.zeros(1, dtype=torch.int64, device=DEV)
    epoch = lambda: m._target_epoch(dom, 0)                                                     # noqa: E731
    emit(dict(what="graphata_adaptation_epoch", path="trainer_eager_one_epoch", peak_bytes=_peak_bytes(epoch), **shape))
    write_jsonl(a.out, lines)


if __name__ == "__main__":
    main(sys.argv[1:])
