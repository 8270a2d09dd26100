#!/usr/bin/env python
"""SpecReg at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a with 7,410 / 5,578 nodes), times over steady-state
repetitions after a warm-up, the kernels of csrc/gda_critic3.hip against the torch composition on the same GPU:

- us per critic update at h = 128 and h = 64: ``ops.critic3_grads`` (gradients only) and ``ops.critic3_adam`` (Adam inside)
  against the reference's formulation in torch -- the ``Sequential`` forward, ``autograd.grad(create_graph=True)``,
  ``backward()`` -- without and with ``torch.optim.Adam.step()``;
- the row kernel's share of the fp32 MFMA peak (157 TF; 16 h^2 flops per row), its time read from torch's profiler;
- us of the encoder-side gap with its backward, and of ``ops.spectral_hinge`` with its backward at k = 1000, both ways;
- ms per epoch of ``SpecReg.fit`` (hidden width 128, dropout 0.1, ``ppmi=False``, ``reg_mode=True`` with the default
  thresholds, a random [1000, N] ``eivec``) with the fused-critic switch on and off, from the epoch hook's stamps.

The torch compositions are the yardsticks and run only here.  One JSON line per result, also written to ``--out``.

    python tools/specreg_bench.py [--epochs 30] [--out profiles/specreg_acm_dblp_bench.jsonl]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops  # noqa: E402
from pygda_amd.optim import Adam  # noqa: E402
from _trainer_bench import collector, events as _events, steady_ms, write_jsonl  # noqa: E402

DEV = "cuda:0"
NS, NT, K = 7410, 5578, 1000
PEAK_FP32_MFMA = 157e12


def _critic(h):
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1)).to(DEV)


def _torch_update(critic, es, et, opt=None):
    """The reference's critic iteration (specreg.py:194-200, 380-419) as the trainer's torch path runs it."""
    for p in critic.parameters():
        p.grad = None
    loss_1 = critic(es).mean() - critic(et).mean()
    x = torch.cat([es, et], dim=0).requires_grad_(True)
    out = critic(x)
    grad = torch.autograd.grad(outputs=out, inputs=x, grad_outputs=torch.ones_like(out), create_graph=True,
                               retain_graph=True, only_inputs=True)[0]
    (-loss_1 + 10 * torch.mean((grad.norm(2, dim=1) - 1) ** 2)).backward()
    if opt is not None:
        opt.step()


def _row_kernel_us(fn, reps=10):
    """Mean device time of the row kernel over ``reps`` updates, from torch's profiler; None where it reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            if "k_critic3_rows" in ev.key:
                total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                return total / max(ev.count, 1)
    except Exception as exc:                                   # the figure is a report, not a gate
        print(f"# profiler unavailable: {exc}", file=sys.stderr)
    return None


def _updates(emit, h, gen):
    es, et = torch.randn(NS, h, generator=gen).to(DEV), torch.randn(NT, h, generator=gen).to(DEV)
    flops = 16 * h * h * (NS + NT)
    critic = _critic(h)
    params = ops.critic3_params(critic)
    for p in params:
        p.grad = torch.zeros_like(p)
    loss = torch.zeros(1, device=DEV)
    out = (loss, *(p.grad for p in params))
    opt = Adam(critic.parameters(), 4e-3)
    assert ops.critic3_ok(es, critic)
    grads_only = lambda: ops.critic3_grads(es, et, params, out)
    adam_inside = lambda: ops.critic3_adam(es, et, params, opt, loss)
    tcritic = _critic(h)
    topt = torch.optim.Adam(tcritic.parameters(), 4e-3)
    for path, fn in (("kernels_grads_only", grads_only), ("kernels_adam_inside", adam_inside),
                     ("torch_composition_grads_only", lambda: _torch_update(tcritic, es, et)),
                     ("torch_composition_with_adam_step", lambda: _torch_update(tcritic, es, et, topt))):
        us, spread = _events(fn, 10)
        line = dict(what="critic_update", path=path, h=h, us=us, spread_us=spread, rows=NS + NT)
        if path.startswith("kernels"):              # the closed form's flop count says nothing about the double backward
            line["tflops_algorithmic"] = round(flops / us / 1e6, 2)
        emit(line)
    row_us = _row_kernel_us(grads_only)
    emit(dict(what="critic_row_kernel", h=h, us=None if row_us is None else round(row_us, 1), rows=NS + NT,
              fraction_of_fp32_mfma_peak=None if row_us is None else round(flops / (row_us * 1e-6) / PEAK_FP32_MFMA, 4)))
    # the gap with its backward
    gs, gt = es.clone().requires_grad_(), et.clone().requires_grad_()
    for path, fn in (("kernels", lambda: ops.critic3_gap(gs, gt, *params)),
                     ("torch_composition_on_gpu", lambda: critic(gs).mean() - critic(gt).mean())):
        us, spread = _events(lambda fn=fn: torch.autograd.grad(fn() * 0.1, [gs, gt]), 10)
        emit(dict(what="critic_gap_with_backward", path=path, h=h, us=us, spread_us=spread, rows=NS + NT))


def _torch_hinge(eivec, enc, ts, gs, tm, gm):
    x = eivec @ enc
    return F.relu((x[:-1] - x[1:]).abs() - ts).mean() * gs + F.relu(x.abs() - tm).mean() * gm


def _fit_ms(src, tgt, epochs, fused):
    m = pygda_amd.models.SpecReg(src.x.size(1), 128, 5, dropout=0.1, ppmi=False, reg_mode=True, device=DEV, epoch=epochs,
                                 verbose=0)
    m.use_fused_critic = fused
    stamps = []
    m.epoch_hook = lambda e, loss, acc, secs: stamps.append((secs, loss))
    torch.manual_seed(0)
    np.random.seed(0)
    ops.dropout_state.counter(torch.device(DEV)).zero_()     # the keep-bit stream restarts: both fits draw the same masks
    m.fit(src, tgt)
    torch.cuda.synchronize()
    return steady_ms([s[0] for s in stamps], 8 if epochs > 12 else 1), stamps[-1][1]


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specreg_acm_dblp_bench.jsonl"))
    a = ap.parse_args(argv)
    emit, lines = collector()
    gen = torch.Generator().manual_seed(0)
    for h in (128, 64):
        _updates(emit, h, gen)
    eivec = (torch.randn(K, NS, generator=gen) / NS ** 0.5).to(DEV)
    enc = torch.randn(NS, 128, generator=gen).to(DEV).requires_grad_()
    for path, fn in (("kernels", ops.spectral_hinge), ("torch_composition_on_gpu", _torch_hinge)):
        us, spread = _events(lambda fn=fn: torch.autograd.grad(fn(eivec, enc, 0.7, 0.5, 0.9, 0.5), [enc]), 10)
        emit(dict(what="spectral_hinge_with_backward", path=path, us=us, spread_us=spread, k=K, n=NS, h=128))
    src, tgt = bench.make_cfg_a(ns=NS, nt=NT)
    src.eivec, tgt.eivec = torch.randn(K, NS, generator=gen).to(DEV), torch.randn(K, NT, generator=gen).to(DEV)
    for fused in (True, False):
        ms, loss = _fit_ms(src, tgt, a.epochs, fused)
        emit(dict(what="specreg_fit", fused_critic=fused, ms_per_epoch=round(ms, 3), last_loss=loss, epochs=a.epochs, hid=128))
    write_jsonl(a.out, lines)


if __name__ == "__main__":
    main(sys.argv[1:])
