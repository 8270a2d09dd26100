#!/usr/bin/env python
"""GTrans at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a: 9,360 / 5,484 nodes, 6,775 bag-of-words features,
hid 128, 5 classes, ``loop_feat=4``, ``loop_adj=1``), times over steady-state repetitions after a warm-up:

- ms per pretraining epoch and per adaptation iteration (four feature steps, one structure step with the Adam step
  acting, the projection), eager and captured, from the epoch hook's stamps;
- one ``test_time_loss`` evaluation with both gradients on the kernels (two ``ops.wgcn_norm``, six
  ``ops.weighted_propagate`` with their SDDMMs, ``ops.gtrans_loss``) against the SAME evaluation composed from the host
  fallbacks in torch on the same GPU (index_add scatter, autograd through gcn_norm, the cosine losses).  The torch
  composition is the yardstick and runs only here;
- ``ops.gtrans_project`` against ``perturb.project`` on device tensors (whose bisection reads a sum back per halving).

One JSON line per result, also written to ``--out``.

    python tools/gtrans_bench.py [--epochs 40] [--out profiles/gtrans_acm_dblp_bench.jsonl]
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
from pygda_amd.utils.perturb import project  # noqa: E402
from _trainer_bench import collector, events as _events, source_free_fit_stamps, write_jsonl  # noqa: E402

DEV = "cuda:0"


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtrans_acm_dblp_bench.jsonl"))
    a = ap.parse_args(argv)
    emit, lines = collector()
    src, tgt = bench.make_cfg_a()
    n, d = tgt.x.size(0), 128
    for graph in (False, True):
        pre, ada, loss = source_free_fit_stamps(pygda_amd.models.GTrans, src, tgt, a.epochs, graph, step_structure=True)
        emit(dict(what="gtrans_fit", captured=graph, ms_per_pretraining_epoch=round(pre, 3),
                  ms_per_adaptation_iteration=round(ada, 3), last_loss=loss, epochs=a.epochs))
    # one loss evaluation with both gradients: kernels against the host fallbacks on the same GPU
    ei = tgt.edge_index
    mei = ei[:, ei[0] < ei[1]]
    plan_d = ops.wgcn_plan(ei, n, mei, device=DEV)
    plan_t = ops.wgcn_plan(ei, n, mei)                     # the fallbacks index with int64: the host plan, moved
    for k, v in list(plan_t.__dict__.items()):
        if torch.is_tensor(v):
            setattr(plan_t, k, v.to(DEV))
    g = torch.Generator().manual_seed(0)
    h0 = torch.randn(n, d, generator=g).to(DEV).requires_grad_(True)
    W = (torch.randn(d, d, generator=g) / d ** 0.5).to(DEV)
    p = (torch.rand(plan_d.m, generator=g) * 0.2).to(DEV).requires_grad_(True)
    keep = (torch.rand(plan_d.ec, generator=g) >= 0.05).to(DEV)
    perm = torch.randperm(n, generator=g).to(DEV)
    w_prev = plan_d.entry_weights(plan_d.w0.to(DEV, torch.float32))

    def evaluate(kernels):
        plan = plan_d if kernels else plan_t
        norm = ops.wgcn_norm if kernels else (lambda pl, w, q, keep=None, view=0: ops._wgcn_norm_host(pl, w, q, keep))
        if kernels:
            prop = lambda x, val, view: ops.weighted_propagate(x, plan, val, None, view)
            lin = lambda x: ops.linear_nt(x, W)
            loss_fn = ops.gtrans_loss
        else:
            prop = lambda x, val, view: torch.zeros_like(x).index_add(0, plan.erow, val[:, None] * x[plan.col])
            lin = lambda x: x @ W.t()
            loss_fn = ops._gtrans_loss_host
        v1, _ = norm(plan, w_prev, p, keep=keep.float() if kernels else keep, view=0)
        v2, _ = norm(plan, w_prev, p, view=1)
        outs = []
        for x, val, view in ((h0, v1, 0), (h0, v2, 1), (h0[perm], v2, 1)):
            outs.append(prop(lin(torch.relu(prop(x, val, view))), val, view))
        loss, _ = loss_fn(*outs, -1)
        return torch.autograd.grad(loss, [h0, p])

    for kernels in (True, False):
        us, spread = _events(lambda: evaluate(kernels), 10)
        emit(dict(what="test_time_loss_with_gradients", path="kernels" if kernels else "torch_composition_on_gpu",
                  us=us, spread_us=spread, n=n, nnz=plan_d.nnz, m=plan_d.m, d=d))
    q = (torch.rand(plan_d.m, generator=g) * 0.5).to(DEV)
    budget = int(0.1 * ei.size(1) // 2)
    for kernels in (True, False):
        fn = (lambda: ops.gtrans_project(q.clone(), budget)) if kernels else (lambda: project(budget, q.clamp(min=1e-7), 1e-7))
        us, spread = _events(fn, 10)
        emit(dict(what="project", path="kernel" if kernels else "torch_on_gpu", us=us, spread_us=spread, m=plan_d.m,
                  budget=budget))
    write_jsonl(a.out, lines)


if __name__ == "__main__":
    main(sys.argv[1:])
