#!/usr/bin/env python
"""SEPA at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a: 9,360 / 5,484 nodes, 6,775 bag-of-words features,
hid 128, 5 classes), HIP-event times over steady-state repetitions after a warm-up:

- the prototype term alone (target logits and features and source features in; loss_im, loss_pp, loss_sep and all
  input gradients out): ``ops.sepa_term`` against the same term composed in torch on the device from the
  ``device='cpu'`` lines.  The torch composition is the yardstick and runs only here;
- the parts of one eager epoch: the term, its PageRank (2k SpMM launches) alone, the optimizer step, and the rest
  (the encoders, forward and backward, the NLL and the log's ``predict``) as the difference;
- ms per epoch eager and captured, and the peak memory of a fit, for ``gcn``.

One JSON line per result, also written to ``--out``.

    python tools/sepa_bench.py [--epochs 24] [--out profiles/sepa_acm_dblp_bench.jsonl]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops  # noqa: E402
from pygda_amd.graph import as_graph  # noqa: E402
from _trainer_bench import collector, events as _events, steady_ms, write_jsonl  # noqa: E402

DEV = "cuda:0"
LAM = dict(lamda_im=0.2, lamda_pp=0.1, lamda_sep=1.0, tau=1.5)


def _torch_term(z, f, fs, ys, row, col, norm, C):
    """The host lines of the trainer on device tensors (torch.mm, index_add_, F.normalize, autograd)."""
    eye = torch.eye(C, device=DEV)
    prob = F.softmax(z, dim=1)
    mean_prob = prob.mean(dim=0)
    ent = -torch.sum(prob * torch.log(prob + 1e-12), dim=1)
    loss_im = torch.sum(mean_prob * torch.log(mean_prob + 1e-12)) + ent.mean()
    oh_s = eye[ys]
    sp = (torch.mm(fs.t(), oh_s) / oh_s.sum(dim=0)).t()
    pred = torch.max(prob, dim=1)[1]
    onehot = eye[pred]
    count = onehot.sum(dim=0)
    biased = (torch.mm(f.t(), onehot) / (count + 1e-12)).t()
    matrix = F.normalize((torch.mm(onehot.t(), prob) / count.clamp(min=1)[:, None]) * (1 - eye), dim=1)
    every = F.normalize(prob * matrix[pred], dim=1)
    own = biased[pred]
    x0 = torch.mm(every, biased) / torch.sum(every + 1e-12, dim=1, keepdim=True) - own
    x = x0
    for _ in range(5):
        x = 0.1 * torch.zeros_like(x0).index_add_(0, col, norm[:, None] * x[row]) + 0.9 * x0
    per_node = own + ent.unsqueeze(-1) * F.normalize(x, dim=1)
    tp = (torch.mm(per_node.t(), onehot) / (count + 1e-12)).t()
    t, s = F.normalize(tp + 1e-6, dim=1), F.normalize(sp + 1e-6, dim=1)
    ts, tt, ss = (torch.exp(torch.mm(a, b.t()) / LAM["tau"]) for a, b in ((t, s), (t, t), (s, s)))
    den = ts.sum(1) - ts.diagonal() + tt.sum(1) - tt.diagonal() + ss.sum(1) - ss.diagonal()
    loss_pp = -torch.log((ts.diagonal() / den.clamp(min=1e-6)).clamp(min=1e-6)).mean()
    u = F.normalize(sp, dim=1)
    sim = torch.exp(torch.mm(u, u.t()) / LAM["tau"])
    loss_sep = torch.log((sim.sum(1) - sim.diagonal()) / (C - 1) + 1e-8).mean()
    return LAM["lamda_im"] * loss_im + LAM["lamda_pp"] * loss_pp + LAM["lamda_sep"] * loss_sep


def _fit_ms(src, tgt, epochs, graph):
    m = pygda_amd.models.SEPA(src.x.size(1), 128, int(src.y.max()) + 1, device=DEV, epoch=epochs, verbose=0,
                              use_hip_graph=graph)
    stamps = []
    m.epoch_hook = lambda e, loss, acc, secs: stamps.append((secs, loss))
    torch.manual_seed(0)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.fit(src, tgt)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = steady_ms([s[0] for s in stamps], 8 if epochs > 12 else 1)
    return ms, peak, stamps[-1][1], m


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sepa_acm_dblp_bench.jsonl"))
    a = ap.parse_args(argv)
    emit, lines = collector()
    src, tgt = bench.make_cfg_a()
    n, ns, h, C = tgt.x.size(0), src.x.size(0), 128, 5
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(n, C, generator=g) * 2).to(DEV).requires_grad_(True)
    f = (torch.randn(n, h, generator=g) * 0.5).to(DEV).requires_grad_(True)
    fs = torch.randn(ns, h, generator=g).to(DEV).requires_grad_(True)
    ys, ys32 = src.y.to(DEV), src.y.to(DEV, torch.int32)
    ei = tgt.edge_index.to(DEV)
    graph = as_graph(ei, n, None, False, True, True, "col")
    (row, col), norm = graph.to_coo()

    def fused():
        total, _, _ = ops.sepa_term(z, f, fs, ys32, graph, LAM["lamda_im"], LAM["lamda_pp"], LAM["lamda_sep"], LAM["tau"])
        torch.autograd.grad(total, (z, f, fs))

    def composed():
        torch.autograd.grad(_torch_term(z, f, fs, ys, row, col, norm, C), (z, f, fs))

    x = torch.randn(n, h, device=DEV, requires_grad=True)

    def pagerank():
        torch.autograd.grad(ops.ppr(x, graph, 5, 0.9).sum(), x)

    fu, fu_spread = _events(fused, 20)
    co, co_spread = _events(composed, 20)
    pr, pr_spread = _events(pagerank, 20)
    emit(dict(what="sepa_prototype_term", n=n, ns=ns, h=h, classes=C, fused_fwd_bwd_us=fu, fused_spread_us=fu_spread,
              torch_fwd_bwd_us=co, torch_spread_us=co_spread, fused_launches_fwd_bwd=[18, 14],
              pagerank_fwd_bwd_us=pr, pagerank_spread_us=pr_spread, workspace_bytes=ops.sepa_bytes(n, C, h)))
    src, tgt = (pygda_amd.data.Data(x=d.x.to(DEV), edge_index=d.edge_index.to(DEV), y=d.y.to(DEV)) for d in (src, tgt))
    for captured in (False, True):
        ms, peak, loss, m = _fit_ms(src, tgt, a.epochs, captured)
        d = dict(what="sepa_epoch", gnn="gcn", captured=captured, ms_per_epoch=round(ms, 3),
                 fit_peak_mib=round(peak / 2**20, 1), last_loss=loss, epochs=a.epochs)
        if not captured:
            for p in m.gnn.parameters():
                p.grad = torch.zeros_like(p)
            opt, opt_spread = _events(m.optimizer.step, 20)
            d.update(term_us=fu, pagerank_us=pr, optimizer_us=opt, optimizer_spread_us=opt_spread,
                     encoders_nll_predict_us=round(ms * 1e3 - fu - opt, 1))
        emit(d)
    write_jsonl(a.out, lines)


if __name__ == "__main__":
    main(sys.argv[1:])
