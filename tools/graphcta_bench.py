#!/usr/bin/env python
"""GraphCTA at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a: 9,360 / 5,484 nodes, 6,775 bag-of-words features,
hid 128, 5 classes, ``loop_model=3``, ``loop_feat=4``, ``loop_adj=1``, ``K=5``), times over steady-state repetitions
after a warm-up:

- ms per pretraining epoch and per adaptation iteration (three model steps with their memory updates, four feature
  steps, one structure step, the projection), eager and captured, from the epoch hook's stamps;
- the model loss with both gradients on the kernels (``ops.cta_model_loss``: two streamed passes over ``F^ F^^T``)
  against the SAME loss composed from the host fallback in torch on the same GPU (the ``[N, N]`` array of exponentials,
  kept for the backward pass);
- the top-(K + 1) plus the test-time loss with both gradients (``ops.cta_knn``, ``ops.cta_test_time_loss``) against the
  torch composition on the same GPU (``feat mem^T``, ``topk``, the class sums).  The torch compositions are the
  yardsticks and run only here.

One JSON line per result, also written to ``--out``.

    python tools/graphcta_bench.py [--epochs 40] [--out profiles/graphcta_acm_dblp_bench.jsonl]
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
from _trainer_bench import collector, events as _events, source_free_fit_stamps, write_jsonl  # noqa: E402

DEV = "cuda:0"


def _torch_test_time(logits, feat, mem_fea, mem_cls, k1):
    """``test_time_loss`` after the forward passes as torch composes it on a device: no host read either (the selection
    by rank, as ``ops._cta_test_time_host`` takes it, on device tensors)."""
    import torch.nn.functional as F
    n, c = logits.shape
    p = F.softmax(logits, dim=1)
    pred = p.argmax(dim=1)
    ent = -(p * torch.log(p + 1e-8)).sum(dim=1)
    est_p = (ent < ent.mean()).sum().double() / n
    by_ent = torch.sort(ent.detach(), stable=True).indices
    grouped = by_ent[torch.sort(pred[by_ent], stable=True).indices]
    cnum = torch.bincount(pred, minlength=c)
    start = torch.cumsum(cnum, 0) - cnum
    rank = torch.empty(n, dtype=torch.long, device=logits.device)
    rank[grouped] = torch.arange(n, device=logits.device) - start[pred[grouped]]
    sel = (rank < (cnum.double() * est_p / 5).long()[pred]).to(logits.dtype)
    ce = (F.cross_entropy(logits, pred, reduction='none') * sel).sum() / sel.sum()
    distance = feat @ mem_fea.t()
    idx_near = torch.topk(distance, dim=-1, largest=True, k=k1).indices[:, 1:]
    nb = ((feat.unsqueeze(1) * mem_fea[idx_near]).sum(-1).sum(1) / (k1 - 1)).mean()
    same = pred.unsqueeze(-1) == mem_cls.argmax(dim=1)
    ng = ((distance * ~same).sum(1) / torch.sum(~same, dim=1)).mean()
    return ce - nb * 0.1 + ng * 0.1


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graphcta_acm_dblp_bench.jsonl"))
    a = ap.parse_args(argv)
    emit, lines = collector()
    src, tgt = bench.make_cfg_a()
    n, d, c, k1 = tgt.x.size(0), 128, 5, 6
    for graph in (False, True):
        pre, ada, loss = source_free_fit_stamps(pygda_amd.models.GraphCTA, src, tgt, a.epochs, graph)
        emit(dict(what="graphcta_fit", captured=graph, ms_per_pretraining_epoch=round(pre, 3),
                  ms_per_adaptation_iteration=round(ada, 3), last_loss=loss, epochs=a.epochs))
    g = torch.Generator().manual_seed(0)
    proto = torch.randn(c, d, generator=g)
    pred = torch.randint(0, c, (n,), generator=g)
    feat = (proto[pred] + 0.5 * torch.randn(n, d, generator=g)).to(DEV).requires_grad_(True)
    logits = (2 * torch.randn(n, c, generator=g)).to(DEV).requires_grad_(True)
    proto, pred = proto.to(DEV), pred.to(DEV)
    mem_fea = (feat.detach() + 0.3 * torch.randn(n, d, generator=g).to(DEV)).contiguous()
    mem_cls = torch.softmax(2 * torch.randn(n, c, generator=g), dim=1).to(DEV)

    def model_loss(kernels):
        fn = ops.cta_model_loss if kernels else ops._cta_model_loss_host
        return torch.autograd.grad(fn(feat, logits, proto, pred, 0.2, 0.2)[0], [feat, logits])

    def test_time(kernels):
        if kernels:
            idx, _ = ops.cta_knn(feat.detach(), mem_fea, k1)
            loss = ops.cta_test_time_loss(logits, feat, mem_fea, mem_cls, idx)[0]
        else:
            loss = _torch_test_time(logits, feat, mem_fea, mem_cls, k1)
        return torch.autograd.grad(loss, [feat, logits])

    for what, fn in (("model_loss_with_gradients", model_loss), ("knn_and_test_time_loss_with_gradients", test_time)):
        for kernels in (True, False):
            us, spread = _events(lambda: fn(kernels), 10)
            emit(dict(what=what, path="kernels" if kernels else "torch_composition_on_gpu", us=us, spread_us=spread, n=n,
                      d=d, c=c, k1=k1))
    write_jsonl(a.out, lines)


if __name__ == "__main__":
    main(sys.argv[1:])
