#!/usr/bin/env python
"""DGDA at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a: 9,360 / 5,484 nodes, 6,775 bag-of-words features)
with the reference's default widths (d / y / m = 64 / 256 / 128: a stacked head of 896, dec_dim 64) at hidden width
128 and random 128-wide embeddings in place of DeepWalk's: steady-state ms/epoch (two optimiser steps each), eager and
captured.  Separately, the 896-wide aggregation of the manipulated pass at N = 9,360 three ways on the same ~10 %-dense
matrix -- the bit-adjacency GEMM, ``propagate`` on that matrix as a CSR, ``torch.mm`` on the materialised fp32 matrix
-- timed with device events in windows of at least 0.15 s, the three taking turns inside every round, after a warm-up
of each; and the mask and reconstruction kernels alone.  One JSON line per result, written to ``--out`` (replaced).

    python tools/dgda_bench.py [--epochs 16] [--out profiles/dgda_acm_dblp_bench.jsonl]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops  # noqa: E402
from pygda_amd.graph import build_csr  # noqa: E402
from _trainer_bench import collector, events, steady_ms, write_jsonl  # noqa: E402

DEV = "cuda:0"


def _pair():
    src, tgt = bench.make_cfg_a()
    for d in (src, tgt):
        n = d.x.size(0)
        if int(d.edge_index.max()) + 1 != n:              # the reference's to_dense_adj needs the last node in edge_index
            d.edge_index = torch.cat([d.edge_index, torch.tensor([[n - 1, 0], [0, n - 1]])], 1)
    return src, tgt


def alternating(fns, window_s, rounds):
    """{name: (median us, [min, max], reps)}: ``_trainer_bench.events`` windows of at least ``window_s`` seconds (the
    repetitions sized from a first short window), the candidates taking turns inside every round so that a drift of
    the machine hits all of them alike."""
    reps = {k: max(10, int(window_s * 1e6 / events(fn, 5, rounds=None)) + 1) for k, fn in fns.items()}
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            out[name].append(events(fn, reps[name], rounds=None))
    return {k: (round(statistics.median(v), 1), [round(min(v), 1), round(max(v), 1)], reps[k]) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.15, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dgda_acm_dblp_bench.jsonl"))
    args = ap.parse_args()
    emit, lines = collector()
    src, tgt = _pair()
    gen = torch.Generator().manual_seed(1)
    emb = (torch.randn(src.x.size(0), 128, generator=gen), torch.randn(tgt.x.size(0), 128, generator=gen))
    m = pygda_amd.models.DGDA(src.x.size(1), 128, 5, device=DEV, epoch=args.epochs, verbose=0, pretrained_emb=emb)
    per = {}
    U = m.epochs_per_graph
    for graphed in (False, True):
        stamps = []
        m.use_hip_graph = graphed
        m.epoch_hook = lambda e, l, a, sec: stamps.append((time.perf_counter(), l))
        torch.manual_seed(200)
        ops.dropout_state.counter(torch.device(DEV)).zero_()     # the same Philox stream for both fits: the same losses
        torch.cuda.reset_peak_memory_stats()
        m.fit(src, tgt)
        torch.cuda.synchronize()
        per[graphed] = (steady_ms([s[0] for s in stamps], U), stamps[-1][1], torch.cuda.max_memory_allocated() / 2**20)
    emit(dict(what="dgda_epoch", eager_ms_per_epoch=per[False][0], captured_ms_per_epoch=per[True][0],
              epochs_per_graph=U, epochs=args.epochs, last_loss_eager=per[False][1], last_loss_captured=per[True][1],
              peak_allocated_mib_eager=per[False][2], peak_allocated_mib_captured=per[True][2],
              features_mib=(src.x.numel() + tgt.x.numel()) * 4 / 2**20))
    del m

    n, c = src.x.size(0), 896
    labels = ops.AsnLabels(src.edge_index.to(DEV), n)
    bits = ops.dgda_manip_bits(labels, 0.1, 0.1)
    torch.manual_seed(0)
    h = torch.randn(n, c, device=DEV)
    bias = torch.randn(c, device=DEV)
    dense = bits.dense()
    dense += torch.eye(n, device=DEV)                                       # the diagonal at weight 2
    dense *= bits.dis[:, None]
    dense *= bits.dis[None, :]
    row, col = dense.nonzero(as_tuple=True)
    g = build_csr(torch.stack([col, row]), n, dense[row, col], add_self_loops=False, normalize=False)
    g.static = True
    fns = {"bit_gemm": lambda: ops.dgda_bit_propagate(h, bits, bias),
           "propagate_csr": lambda: ops.propagate(h, g, 1, bias),
           "torch_mm_fp32": lambda: torch.addmm(bias, dense, h)}
    ref = fns["torch_mm_fp32"]()
    err = {k: float((fns[k]() - ref).abs().max() / ref.abs().max()) for k in ("bit_gemm", "propagate_csr")}
    t = alternating(fns, args.window, args.rounds)
    flop = 2.0 * n * n * c
    emit(dict(what="dgda_aggregation_896", nodes=n, width=c, nnz=int(row.numel()), density=row.numel() / (n * n),
              bit_gemm_us=t["bit_gemm"][0], bit_gemm_spread=t["bit_gemm"][1],
              propagate_csr_us=t["propagate_csr"][0], propagate_csr_spread=t["propagate_csr"][1],
              torch_mm_fp32_us=t["torch_mm_fp32"][0], torch_mm_fp32_spread=t["torch_mm_fp32"][1],
              bit_gemm_dense_equivalent_tflops=flop / t["bit_gemm"][0] * 1e-6,
              bit_matrix_mib=bits.bits.numel() * 4 / 2**20, fp32_matrix_mib=n * n * 4 / 2**20,
              max_rel_diff_vs_torch_mm=err, reps={k: v[2] for k, v in t.items()}, rounds=args.rounds))
    del dense, g, ref

    z = (0.2 * torch.randn(n, 64, device=DEV)).requires_grad_(True)

    def recon():
        ops.dgda_recon_loss(z, bits).backward()

    t = alternating({"manip_bits": lambda: ops.dgda_manip_bits(labels, 0.1, 0.1, out=bits), "recon_bits": recon},
                    args.window, args.rounds)
    emit(dict(what="dgda_mask_and_recon", nodes=n, k=64, manip_bits_us=t["manip_bits"][0],
              manip_bits_spread=t["manip_bits"][1], recon_bits_fwd_bwd_us=t["recon_bits"][0],
              recon_bits_spread=t["recon_bits"][1], reps={k: v[2] for k, v in t.items()}, rounds=args.rounds))
    write_jsonl(args.out, lines, stamp=False)


if __name__ == "__main__":
    main()
