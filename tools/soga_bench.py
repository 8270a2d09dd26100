#!/usr/bin/env python
"""SOGA at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a: 9,360 / 5,484 nodes, 6,775 bag-of-words features,
hid 128, 5 classes, 5 negatives, two views), HIP-event times over steady-state repetitions after a warm-up:

- the adaptation term alone (target logits in; loss, its four parts and dlogits out): ``ops.soga_adapt`` against the
  same term composed in torch on the device (softmax, embedding gathers, bmm, exp / sum / log, autograd's scatter-add
  backward).  The torch composition is the yardstick and runs only here.  Measured on the tables ``soga_samples``
  draws on the uniform stand-in graph and on its power-law variant (hubs), for several segment lengths of the reverse
  index, with the longest reverse list and the segment count beside each time;
- ms per adaptation epoch eager and captured, and the share of a captured epoch that is not the term or the optimizer
  step (the encoder, forward and backward).

One JSON line per result, also written to ``--out``.

    python tools/soga_bench.py [--epochs 24] [--out profiles/soga_acm_dblp_bench.jsonl]
"""
import argparse
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops  # noqa: E402
from pygda_amd.utils.sampler import soga_samples  # noqa: E402
from _trainer_bench import collector, events as _events, steady_ms, write_jsonl  # noqa: E402

DEV = "cuda:0"


def _torch_term(z, views):
    """The reference's lines on device tensors."""
    prob = F.softmax(z, dim=-1)
    ent = torch.mean(torch.sum(-prob * torch.log(prob + 1e-5), dim=1))
    mean = prob.mean(dim=0)
    loss = ent - torch.sum(-mean * torch.log(mean + 1e-8))
    for cen, pos, neg in views:
        c, p, n = F.embedding(cen, prob), F.embedding(pos, prob).permute(0, 2, 1), F.embedding(neg, prob).permute(0, 2, 1)
        e_pos = torch.exp(torch.bmm(c, p).squeeze())
        e_neg = torch.sum(torch.exp(torch.bmm(c, n).squeeze()), dim=1)
        loss = loss + (-torch.log(e_pos / e_neg)).mean()
    return loss


def _fit_stamps(src, tgt, epochs, graph):
    m = pygda_amd.models.SOGA(src.x.size(1), 128, 5, device=DEV, epoch=epochs, verbose=0, use_hip_graph=graph)
    stamps = []
    m.epoch_hook = lambda e, loss, acc, secs: stamps.append((secs, loss, acc))
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    m.fit(src, tgt)
    torch.cuda.synchronize()
    tgt_stamps = [s for s in stamps if s[2] is None]
    ms = steady_ms([s[0] for s in tgt_stamps], 8 if epochs > 12 else 1)
    return ms, tgt_stamps[-1][1], m


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soga_acm_dblp_bench.jsonl"))
    a = ap.parse_args(argv)
    emit, lines = collector()
    C, K = 5, 5
    term_us = None
    for degrees in ("uniform", "powerlaw"):
        _, tgt = bench.make_cfg_a(degrees=degrees)
        n = tgt.x.size(0)
        random.seed(0)
        np.random.seed(0)
        views = soga_samples(tgt.edge_index, n, K)
        g = torch.Generator().manual_seed(0)
        z = (torch.randn(n, C, generator=g) * 2).to(DEV).requires_grad_(True)
        dviews = [tuple(torch.from_numpy(t).to(DEV) for t in v) for v in views]

        def composed():
            torch.autograd.grad(_torch_term(z, dviews), z)

        co, co_spread = _events(composed, 20)
        for segment in (16, 64, 256, 1 << 30):
            plan = ops.soga_plan(views, n, DEV, segment=segment)

            def fused():
                loss, _ = ops.soga_adapt(z, plan, 1.0, 1.0)
                torch.autograd.grad(loss, z)

            fu, fu_spread = _events(fused, 50)
            if degrees == "uniform" and segment == ops.SOGA_SEGMENT:
                term_us = fu
            emit(dict(what="soga_adapt_term", degrees=degrees, n=n, classes=C, negatives=K, views=2, segment=segment,
                      segments=plan.nseg, longest_reverse_list=int(np.diff(plan.rev_ptr).max()),
                      median_reverse_list=int(np.median(np.diff(plan.rev_ptr))), fused_fwd_bwd_us=fu,
                      fused_spread_us=fu_spread, torch_fwd_bwd_us=co, torch_spread_us=co_spread, fused_launches=5,
                      bytes=sum(ops.soga_bytes(n, C, n, K, 2))))
    src, tgt = bench.make_cfg_a()
    src, tgt = (pygda_amd.data.Data(x=d.x.to(DEV), edge_index=d.edge_index.to(DEV), y=d.y.to(DEV)) for d in (src, tgt))
    for captured in (False, True):
        ms, loss, m = _fit_stamps(src, tgt, a.epochs, captured)
        d = dict(what="soga_adaptation_epoch", gnn="gcn", layers=3, captured=captured, ms_per_epoch=round(ms, 3),
                 last_loss=loss, epochs=a.epochs)
        if captured:
            for p in m.soga.parameters():
                p.grad = torch.zeros_like(p)
            opt, opt_spread = _events(m.optimizer.step, 20)
            d.update(term_us=term_us, optimizer_us=opt, optimizer_spread_us=opt_spread,
                     encoder_share=round(1.0 - (term_us + opt) / (ms * 1e3), 3))
        emit(d)
    write_jsonl(a.out, lines)


if __name__ == "__main__":
    main(sys.argv[1:])
