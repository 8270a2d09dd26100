"""Regenerate the GraphCTA fixtures (``graphcta_fit_a.npz``, ``graphcta_fit_b.npz``, ``graphcta_fit_c.npz``) by RUNNING THE REFERENCE's
``pygda/models/graphcta.py`` on the PyG stub (build container only, needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_graphcta [--out DIR]

The pair: ``_gtrans_semantics.gtrans_pair`` (300 source / 260 target nodes; the target has a duplicate edge, a
directed-only edge, an explicit self loop and an isolated node), 16 class-informative features, 3 classes, hidden width
16, 2 layers, ``epoch=12`` (12 pretraining epochs, 4 adaptation iterations), ``loop_model=2``, ``loop_feat=2``,
``loop_adj=1``, ``dropout=0`` and ``lr=0.05``; fixture a: ``K=5`` and the defaults otherwise, fixture b: ``K=2``,
``tau=0.5``, ``lamb=0.5``, ``make_undirected=False``, fixture c: b's settings with ``make_undirected=True``.
THE REFERENCE DOES NOT FINISH FIXTURE b's FIT, on any of the eight data seeds of this pair generator (each is run and its
message printed): with ``make_undirected=False`` ``sample_final_edges`` allows exactly ``n_perturbations`` changed edges,
its first round flips that many pairs, and every ``gtrans_pair`` target carries a duplicate edge (weight 2, folded to 0)
and one-way edges on top, so its own range assertion stops it after the twenty sampling rounds.  (That is a property of
these pairs, not of the reference: on a symmetric target without duplicates the assertion has no slack to lose and the
fit ends.)  Fixture b therefore records everything up to there -- the iterations and all twenty rounds -- with the
assertion's message (``stopped``) and empty ``edge_index`` / ``edge_weight`` / ``logits``; fixture c records the complete
fit of the same settings on the symmetrised graph.
Recorded per fixture: the graph pair; the seeds (torch 717, ``random`` 718, ``np.random`` 719), the initial state and the
feature memory drawn after it; the pretraining losses and accuracies; the loss and the contrast part of every model step
with its pseudo labels; the loss of every ``test_time_loss`` call (the twenty of the final sampling behind the
iterations') with its arg-max, its selected rows (bit-packed) and its neighbour sets (int16); the flip weights and the raw
edge weights after every iteration, with the coalesced edge list they belong to; the final ``new_feat``, ``edge_index``,
``edge_weight`` and ``predict``'s logits; and the same fit in float64 from the same initial state (``f64/...``).

A fixture walks its short list of data seeds and takes the first in which the float32 and the float64 run agree on
every discrete decision: the source accuracies, the pseudo labels, the arg-max predictions, the selected sets, the
neighbour sets and the final edge list.  The discrete decisions are stored for the calls of the iterations and the
first call of the final sampling (the nineteen after it see the same features and memory).  The seed taken (``data_seed``) and the smallest gap seen at a decision boundary
(``gap``: arg-max, entropy against its mean, entropy rank, neighbour rank relative to ``max|f| max|m|``; float32 and
float64 run) are recorded.  What the reference does for ``loop_adj=2`` is printed.  Runs on one CPU thread, so that a
rerun reproduces the files bit for bit."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _graphcta_semantics, _gtrans_semantics, _ref_loader
from .make_golden import HERE, np_

EPOCHS, SEEDS = 12, (717, 718, 719)
LOOP_MODEL, LOOP_FEAT, LOOP_ADJ, C = 2, 2, 1, 3
DATA_SEEDS = (531, 631, 731, 831, 931, 1031, 1131, 1231)
CONFIGS = {"graphcta_fit_a.npz": dict(K=5),
           "graphcta_fit_b.npz": dict(K=2, tau=0.5, lamb=0.5, make_undirected=False),
           "graphcta_fit_c.npz": dict(K=2, tau=0.5, lamb=0.5)}
DISCRETE = ("accs", "model_pred", "tt_pred", "tt_sel", "tt_near", "edge_index", "stopped")


def per_iteration(r, iters):
    calls = r["adj_calls"]
    idx = [it * (LOOP_ADJ + 1) + LOOP_ADJ for it in range(iters)]
    return np.stack([calls[i][0] for i in idx]), calls[0][1], np.stack([calls[i][2] for i in idx])


def fx_graphcta(ref, out_dir, name, extra):
    kw = dict(in_dim=16, hid_dim=16, num_classes=C, num_layers=2, lr=0.05, dropout=0., loop_model=LOOP_MODEL,
              loop_feat=LOOP_FEAT, loop_adj=LOOP_ADJ, **extra)
    iters = EPOCHS // (LOOP_FEAT + LOOP_ADJ)
    taken = None
    for seed in DATA_SEEDS:
        s, t = _gtrans_semantics.gtrans_pair(seed, C)
        r = _graphcta_semantics.run_fit(ref, s, t, kw, EPOCHS, SEEDS)
        r64 = _graphcta_semantics.run_fit(ref, s, t, kw, EPOCHS, SEEDS, torch.float64, init=r["init"], mem0=r["mem0"])
        same = all(np.shape(r[k]) == np.shape(r64[k]) and bool(np.all(np.asarray(r[k]) == np.asarray(r64[k])))
                   for k in DISCRETE)
        print(f"  {name} seed {seed}: discrete decisions equal {same}, smallest gaps {r['gap']:.2e} {r64['gap']:.2e}"
              + (f", the reference stops with AssertionError: {r['stopped']}" if r["stopped"] else ""))
        if same and taken is None:
            taken = (seed, s, t, r, r64)
        if taken is not None and extra.get("make_undirected", True):
            break                                # (a make_undirected=False fixture runs every seed: see the docstring)
    if taken is None:
        raise SystemExit(f"{name}: no seed of {DATA_SEEDS} meets the conditions")
    seed, s, t, r, r64 = taken
    assert bool(r["stopped"]) == (not extra.get("make_undirected", True))
    assert np.isfinite(r["steps"]).all() and len(r["steps"]) == iters * (LOOP_FEAT + LOOP_ADJ) + 20
    assert len(r["model"]) == iters * LOOP_MODEL
    keep = iters * (LOOP_FEAT + LOOP_ADJ) + 1
    out = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), tgt_x=np_(t.x), tgt_ei=np_(t.edge_index),
               tgt_y=np_(t.y), seeds=np.array(SEEDS, dtype=np.int64), data_seed=np.int64(seed), mem0=r["mem0"],
               stopped=np.str_(r["stopped"]),
               gap=np.array([r["gap"], r64["gap"]]), K=np.int64(extra["K"]), tau=np.float64(extra.get("tau", 0.2)),
               lamb=np.float64(extra.get("lamb", 0.2)), make_undirected=np.bool_(extra.get("make_undirected", True)),
               model_pred=r["model_pred"].astype(np.int8), tt_pred=r["tt_pred"][:keep].astype(np.int8),
               tt_sel=np.packbits(r["tt_sel"][:keep], axis=1), tt_near=r["tt_near"][:keep].astype(np.int16))
    out.update({"init/" + k2: v for k2, v in r["init"].items()})
    for pre, rr in (("", r), ("f64/", r64)):
        p_it, ei_c, w_it = per_iteration(rr, iters)
        out.update({pre + "src_losses": rr["src_losses"], pre + "accs": rr["accs"], pre + "model": rr["model"],
                    pre + "steps": rr["steps"], pre + "p_iter": p_it, pre + "w_iter": w_it, pre + "coalesced_ei": ei_c,
                    pre + "new_feat": rr["new_feat"], pre + "edge_index": rr["edge_index"],
                    pre + "edge_weight": rr["edge_weight"], pre + "logits": rr["logits"]})
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}  ({os.path.getsize(path) / 1024:.1f} KiB)")
    return s, t, kw


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    torch.set_num_threads(1)                     # one thread: the CPU reductions run in one order, run after run
    ref = _graphcta_semantics.load_graphcta(_ref_loader.load_reference())
    for name, extra in CONFIGS.items():
        s, t, kw = fx_graphcta(ref, a.out, name, extra)
    kw = dict(kw, make_undirected=True)
    print("loop_adj=2 in the reference:", _graphcta_semantics.probe_loop_adj(ref, s, t, kw, EPOCHS, SEEDS) or "runs to the end")


if __name__ == "__main__":
    main(sys.argv[1:])
