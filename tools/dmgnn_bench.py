#!/usr/bin/env python
"""DMGNN at the DBLPv7 -> Citationv1 stand-in shapes (bench.make_cfg_a(ns=5484, es=8117, nt=8935, et=15098): 6,775
bag-of-words features, n_emb 128, 5 classes, batch_size 100), HIP-event times as medians over repeats after a warm-up:

- one step's loss (the embeddings before their ReLU, the PPMI matrices, the indices and the head parameters in; the
  loss and every gradient out): ``ops.dmgnn_prox`` + ``ops.dmgnn_heads`` against the same step composed in torch on
  the device from the ``device='cpu'`` lines (``index_select``, ``mm``, autograd) on the same inputs.  The torch
  composition is the yardstick and runs only here;
- ms per epoch eager and captured;
- predict's product ``P + PPMI @ P`` over the target domain: ``ops.dmgnn_predict`` with its achieved bytes per second
  against ``4 n ld``, next to ``probs + ppmi @ probs`` through torch on the same tensors.

One JSON line per result, also written to ``--out``.  A fused kernel that is not faster than its composition is
reported as such (``fused_faster: false``).

    python tools/dmgnn_bench.py [--epochs 6] [--out profiles/dmgnn_dblp_citation_bench.jsonl]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops  # noqa: E402
from _trainer_bench import collector, events as _events, steady_ms, write_jsonl  # noqa: E402

DEV = "cuda:0"


def _torch_step(ppmi_s, ppmi_t, pidx, rows, z, y, params, alpha, pw):
    """The host lines of the step on device tensors: the blocks by ``index_select``, ``mm`` and autograd."""
    h = z.size(0) // 2
    leaves = [p.detach().requires_grad_(True) for p in params]
    Wc, bc, W1, b1, W2, b2, W3, b3 = leaves
    z = z.detach().requires_grad_(True)
    emb = torch.relu(z)
    blocks = []
    for dom, P in enumerate((ppmi_s, ppmi_t)):
        ix = pidx[dom * h:(dom + 1) * h]
        blk = P.index_select(0, ix).index_select(1, ix) * (1 - torch.eye(h, device=DEV))
        blocks.append((1.0 / (blk.sum(1) + 1e-12))[:, None] * blk)
    prox = sum(torch.norm(emb[d * h:(d + 1) * h] - torch.mm(blocks[d], emb[d * h:(d + 1) * h])) / h for d in range(2))
    logit = F.linear(emb, Wc, bc)
    logit = logit + torch.cat((torch.mm(blocks[0], logit[:h]), torch.mm(blocks[1], logit[h:])), dim=0)
    clf = F.cross_entropy(logit[:h], y.index_select(0, rows[:h]))
    er = emb * 1.0
    er.register_hook(lambda g: -alpha * g)
    d = F.linear(F.relu(F.linear(F.relu(F.linear(er, W1, b1)), W2, b2)), W3, b3)
    dom = F.cross_entropy(d, torch.cat([torch.zeros(h, device=DEV), torch.ones(h, device=DEV)]).long())
    total = clf + dom + pw * prox
    return total, torch.autograd.grad(total, [z] + leaves)


def _fit_ms(src, tgt, epochs, graph):
    m = pygda_amd.models.DMGNN(src.x.size(1), 128, int(src.y.max()) + 1, dropout=0.5, weight_decay=1e-3, lr=1e-3,
                               device=DEV, epoch=epochs, verbose=0, use_hip_graph=graph)
    stamps = []
    m.epoch_hook = lambda e, loss, acc, secs: stamps.append((secs, loss, acc))
    torch.manual_seed(0)
    np.random.seed(0)
    m.fit(src, tgt)
    torch.cuda.synchronize()
    ms = steady_ms([s[0] for s in stamps], 2 if epochs > 3 else 1)
    return ms, stamps[-1][1], stamps[-1][2], m


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmgnn_dblp_citation_bench.jsonl"))
    a = ap.parse_args(argv)
    emit, lines = collector()
    src, tgt = bench.make_cfg_a(seed=7, ns=5484, es=8117, nt=8935, et=15098)
    ns, nt = src.x.size(0), tgt.x.size(0)
    m = None
    for captured in (False, True):
        ms, loss, acc, m = _fit_ms(src, tgt, a.epochs, captured)
        emit(dict(what="dmgnn_ms_per_epoch", requested="captured" if captured else "eager", ms_per_epoch=round(ms, 3),
                  epochs_timed=a.epochs - (2 if a.epochs > 3 else 1), steps_per_epoch=round(max(ns, nt) / 50),
                  final_loss=loss, final_acc=acc))

    # one step's loss on the fitted model's matrices and parameters
    h, e, c, pw, alpha = 50, 128, 5, 0.1, 0.7
    g = torch.Generator().manual_seed(1)
    pidx = torch.cat([torch.randperm(ns, generator=g)[:h], torch.randperm(nt, generator=g)[:h]]).to(DEV)
    rows = torch.cat([pidx[:h], pidx[h:] + ns])
    z = torch.randn(2 * h, e, generator=g).to(DEV)
    params = [p.detach() for p in m.dmgnn.head_parameters()]
    al = torch.tensor(alpha, dtype=torch.float32, device=DEV)

    def fused():
        prox, gprox, blocks = ops.dmgnn_prox(m.ppmi_s, m.ppmi_t, pidx, z, h, pw)
        return ops.dmgnn_heads(z, gprox, blocks, params, m.y_s, rows, al, prox, pw)

    def composed():
        return _torch_step(m.ppmi_s, m.ppmi_t, pidx, rows, z, m.y_s, params, alpha, pw)

    lf, lc = float(fused()[0]), float(composed()[0])
    fu, fu_spread = _events(fused, 50)
    co, co_spread = _events(composed, 50)
    emit(dict(what="dmgnn_step_loss", h=h, e=e, classes=c, fused_us=fu, fused_spread_us=fu_spread, torch_us=co,
              torch_spread_us=co_spread, fused_launches=[1, 6], fused_faster=fu < co, loss_fused=lf, loss_torch=lc))

    # predict's product over the target domain
    ld = m.ppmi_t.stride(0)
    zt = torch.randn(nt, e, generator=g).to(DEV)
    lay = m.dmgnn.node_classifier.layer
    w, b = lay.weight.detach(), lay.bias.detach()
    probs = ops.acdne_predict(zt, w, b)

    def fused_predict():
        return ops.dmgnn_predict(zt, w, b, m.ppmi_t)

    def torch_product():
        return probs + torch.mm(m.ppmi_t, probs)

    err = float((fused_predict() - torch_product()).abs().max())
    fp, fp_spread = _events(fused_predict, 20)
    tp, tp_spread = _events(torch_product, 20)
    emit(dict(what="dmgnn_predict_product", n=nt, ld=ld, classes=c, fused_us=fp, fused_spread_us=fp_spread,
              fused_includes="the softmax of relu(z) Wc^T + bc (its first launch)", algorithmic_bytes=4 * nt * ld,
              fused_gb_per_s=round(4 * nt * ld / (fp * 1e-6) / 1e9, 1), torch_us=tp, torch_spread_us=tp_spread,
              torch_gb_per_s=round(4 * nt * ld / (tp * 1e-6) / 1e9, 1), fused_faster=fp < tp, max_abs_diff=err))
    write_jsonl(a.out, lines)


if __name__ == "__main__":
    main(sys.argv[1:])
