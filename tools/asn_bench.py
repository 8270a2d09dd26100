#!/usr/bin/env python
"""ASN at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a: 9,360 / 5,484 nodes, 6,775 bag-of-words features)
with the settings of the reference's benchmark script (benchmark/node/asn.py: hid 64, hid_dim_vae 5, adv_dim 10,
dropout 0.1, lr 1e-3, weight decay 0, step 3): process_graph per domain, steady-state ms/epoch, eager and captured (log stamps from the first
replay's last epoch to the end; the captured log is read once per replay), and the reconstruction term alone at the source's shape (z [9,360, 10]): the fused kernel's us per launch from HIP
events against the same term composed densely in torch on the device (mm + binary_cross_entropy_with_logits +
backward).  One JSON line per result, also written to ``--out``.

    python tools/asn_bench.py [--epochs 24] [--out profiles/asn_acm_dblp_bench.jsonl]
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
from _trainer_bench import collector, events, steady_ms, write_jsonl  # noqa: E402

DEV = "cuda:0"


def _pair():
    src, tgt = bench.make_cfg_a()
    for d in (src, tgt):
        n = d.x.size(0)
        if int(d.edge_index.max()) + 1 != n:              # the reference's to_dense_adj needs the last node in edge_index
            d.edge_index = torch.cat([d.edge_index, torch.tensor([[n - 1, 0], [0, n - 1]])], 1)
    return src, tgt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=24)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    emit, lines = collector()
    src, tgt = _pair()
    m = pygda_amd.models.ASN(src.x.size(1), 64, 5, 5, dropout=0.1, adv_dim=10, lr=1e-3, weight_decay=0.0, step=3,
                             device=DEV, epoch=args.epochs, verbose=0)
    pg = {}
    for name, d in (("source", src), ("target", tgt)):
        ops.asn_ppmi_graph(d.edge_index.to(DEV), d.x.size(0), 3)              # warm the kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = ops.asn_ppmi_graph(d.edge_index.to(DEV), d.x.size(0), 3)
        torch.cuda.synchronize()
        pg[f"{name}_ms"] = 1e3 * (time.perf_counter() - t0)
        pg[f"{name}_nodes"], pg[f"{name}_nnz"] = d.x.size(0), int(g.rowptr[-1])
    emit(dict(what="asn_process_graph", **pg))

    per = {}
    U = m.epochs_per_graph
    for graphed in (False, True):
        stamps = []
        m.use_hip_graph = graphed
        m.epoch_hook = lambda e, l, a, sec: stamps.append((time.perf_counter(), l))
        torch.manual_seed(200)
        m.fit(src, tgt)
        # steady state: from the log of epoch U - 1 (after the first replay) to the last log, E - U epochs
        per[graphed] = (steady_ms([s[0] for s in stamps], U), stamps[-1][1])
    emit(dict(what="asn_epoch", eager_ms_per_epoch=per[False][0], captured_ms_per_epoch=per[True][0],
                      epochs_per_graph=m.epochs_per_graph, epochs=args.epochs, last_loss_eager=per[False][1],
                      last_loss_captured=per[True][1], peak_allocated_mib=torch.cuda.max_memory_allocated() / 2**20))

    n, k = src.x.size(0), 10
    labels = ops.AsnLabels(src.edge_index.to(DEV), n)
    torch.manual_seed(0)
    z = (0.5 * torch.randn(n, k, device=DEV)).requires_grad_(True)

    def fused():
        loss = ops.asn_recon_loss(z, labels)
        loss.backward()

    y = labels.dense().to(DEV)
    pw = torch.tensor([[labels.pos_weight]], device=DEV)

    def dense():
        loss = labels.norm * F.binary_cross_entropy_with_logits(torch.mm(z, z.t()), y, pos_weight=pw)
        loss.backward()

    chunks = pygda_amd._lib.lib().gda_asn_recon_chunks(n)
    us_f = events(fused, args.reps, rounds=None)
    us_d = events(dense, args.reps, rounds=None)
    emit(dict(what="asn_recon_term", nodes=n, k=k, pairs=n * n, chunks=chunks, fused_us=us_f,
                      torch_dense_us=us_d, speedup=us_d / us_f))
    write_jsonl(args.out, lines, stamp=False, mode="a")


if __name__ == "__main__":
    main()
