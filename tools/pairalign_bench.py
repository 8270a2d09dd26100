#!/usr/bin/env python
"""PairAlign at the ACMv9 -> DBLPv7 stand-in shapes (bench.make_cfg_a: 9,360 / 5,484 nodes, 6,775 bag-of-words features,
5 classes) at hidden width 128, ``cls_dim`` 128, a ``train_mask`` over 80 % of the source: steady-state ms/epoch of the
epochs between two re-weightings, eager and captured; one re-weighting event split into its kernels (device events),
its device-to-host copies, the two host solves and the upload + refresh; and the class-pair statistic kernel against
the torch composition of the same sums on the same card (per-edge outer products + ``index_add_``, fp32 and float64) --
the candidates taking turns inside every round, in windows of at least 0.15 s, after a warm-up of each.  One JSON line
per result, written to ``--out`` (replaced).

    python tools/pairalign_bench.py [--epochs 33] [--out profiles/pairalign_acm_dblp_bench.jsonl]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import pygda_amd  # noqa: E402
from pygda_amd import ops  # noqa: E402
from pygda_amd.qp import solve_simplex_ls  # noqa: E402
from _trainer_bench import collector, write_jsonl  # noqa: E402
from dgda_bench import alternating  # noqa: E402

DEV = "cuda:0"


def _edge_torch(z, ei, cls, K, dtype):
    n, c = z.shape
    zd = z.to(dtype)
    outer = torch.einsum("bi,bj->bij", zd[ei[0]], zd[ei[1]]).reshape(-1, c * c)
    return torch.zeros(K * K, c * c, dtype=dtype, device=z.device).index_add_(0, cls[ei[0]] * K + cls[ei[1]], outer)


def _host_ms(fn, reps=5):
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=33)
    ap.add_argument("--window", type=float, default=0.15, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairalign_acm_dblp_bench.jsonl"))
    args = ap.parse_args()
    emit, lines = collector()
    src, tgt = bench.make_cfg_a()
    src.train_mask = torch.rand(src.x.size(0), generator=torch.Generator().manual_seed(1)) < 0.8
    src.edge_weight = tgt.edge_weight = None
    C = 5
    per = {}
    for graphed in (False, True):
        # no re-weighting inside the timed fit: the epochs between two of them are what repeats
        m = pygda_amd.models.PairAlign(src.x.size(1), 128, C, device=DEV, epoch=args.epochs, verbose=0, edge_rw=True,
                                       label_rw=True, weight_CE_src=True, ew_start=10 ** 9, lw_start=10 ** 9,
                                       use_hip_graph=graphed)
        stamps = []
        m.epoch_hook = lambda e, l, a, sec: stamps.append((time.perf_counter(), l))
        torch.manual_seed(200)
        m.fit(src, tgt)
        torch.cuda.synchronize()
        # the log line of epoch e is written once the group that holds epoch e + 1 has run (the accuracy comes from that
        # forward): between the lines of two epochs that end a group lie exactly b - a epochs, eager or captured
        U = m.epochs_per_graph
        a, b = 2 * U - 1, ((args.epochs - 1) // U - 1) * U - 1
        assert b > a, "--epochs must cover at least four replays"
        per[graphed] = ((stamps[b][0] - stamps[a][0]) / (b - a) * 1e3, stamps[-1][1])
    emit(dict(what="pairalign_epoch", eager_ms_per_epoch=per[False][0], captured_ms_per_epoch=per[True][0],
              epochs_per_graph=m.epochs_per_graph, epochs=args.epochs, last_loss_eager=per[False][1],
              last_loss_captured=per[True][1]))

    # one re-weighting event on the fitted model's logits
    s, t = m._s, m._t
    with torch.no_grad():
        ps, pt = m._forward(s), m._forward(t)
    rw = (torch.rand(C, C, device=DEV) + 0.5).contiguous()
    kern = alternating({"edge_stats_src": lambda: ops.pa_edge_stats(ps, m._edge_plan_s),
                        "edge_stats_tgt": lambda: ops.pa_edge_stats(pt, m._edge_plan_t),
                        "softmax_sums": lambda: ops.pa_softmax_sums(ps, pt, m._soft_plan),
                        "refresh_both_sides": lambda: ops.pa_refresh(s.pg, s.y, rw),
                        "extra_forwards": lambda: (m._forward(s), m._forward(t))}, args.window, args.rounds)
    C_hat, muhat = m._edge_stats(ps, pt)
    P_s, P_t = ops.pa_softmax_sums(ps, pt, m._soft_plan)
    cov = (P_s.t() / s.n).cpu().numpy()
    yhat = (P_t[0] / t.n).cpu().numpy()
    t0 = time.perf_counter()
    w = solve_simplex_ls(C_hat, muhat, m._mu_edge, m.ls_lambda)
    t1 = time.perf_counter()
    solve_simplex_ls(cov, yhat, m._mu_label, m.lw_lambda)
    t2 = time.perf_counter()
    emit(dict(what="pairalign_reweighting_event", source_edges=m._E_s, target_edges=m._E_t,
              kernels_us={k: v[0] for k, v in kern.items()}, kernels_spread={k: v[1] for k, v in kern.items()},
              stats_and_copy_ms=_host_ms(lambda: m._edge_stats(ps, pt)),
              whole_update_ew_ms=_host_ms(lambda: m.update_ew(ps, pt)),
              whole_update_lw_ms=_host_ms(lambda: m.update_lw(ps, pt)),
              host_solve_edge_ms=(t1 - t0) * 1e3, host_solve_label_ms=(t2 - t1) * 1e3, edge_program_n=C * C,
              edge_solution_zeros=int((w == 0).sum()), reps={k: v[2] for k, v in kern.items()}, rounds=args.rounds))

    ei = s.edge_index
    fns = {"pa_edge_stats": lambda: ops.pa_edge_stats(ps, m._edge_plan_s),
           "torch_index_add_fp32": lambda: _edge_torch(ps, ei, s.y, C, torch.float32),
           "torch_index_add_fp64": lambda: _edge_torch(ps, ei, s.y, C, torch.float64)}
    ref = fns["torch_index_add_fp64"]().view(C, C, C, C).permute(0, 2, 1, 3)
    err = float((fns["pa_edge_stats"]() - ref).abs().max() / ref.abs().max())
    tt = alternating(fns, args.window, args.rounds)
    emit(dict(what="pairalign_edge_stats_vs_torch", nodes=s.n, edges=m._E_s, classes=C,
              work_items=m._edge_plan_s.n_items, segments=m._edge_plan_s.n_seg,
              **{k + "_us": v[0] for k, v in tt.items()}, **{k + "_spread": v[1] for k, v in tt.items()},
              max_rel_diff_vs_torch_fp64=err, torch_fp32_temporaries_mib=m._E_s * (C * C + 2 * C) * 4 / 2 ** 20,
              reps={k: v[2] for k, v in tt.items()}, rounds=args.rounds))
    write_jsonl(args.out, lines, stamp=False)


if __name__ == "__main__":
    main()
