"""Regenerate the GraphATA fixtures (``graphata_fit_a.npz``, ``graphata_fit_b.npz``, ``graphata_fit_c.npz``) by RUNNING
THE REFERENCE's ``pygda/models/graphata.py`` on the PyG stub (build container only, needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_graphata [--out DIR]

The graphs: ``_graphata_semantics.graphata_graphs`` -- ``S`` sources of ``_gtrans_semantics.gtrans_pair`` (300 nodes)
from different data seeds and one target (260 nodes; a duplicate edge, a directed-only edge, an explicit self loop and
an isolated node), 16 features, 3 classes, hidden width 16, ``lr=0.05``, ``epoch=6`` (pretraining epochs per source and
adaptation epochs).  Fixture a: ``S=2``, two layers, ``K=5``, the default momentum, no dropout; fixture b: ``S=3``, one
layer, ``K=2``, ``momentum=0.5``, no dropout; fixture c: a's settings with ``dropout=0.5`` (the device draws its keep bits
from another stream: c is for the host fit and for eager against captured).

THE INITIAL STATE IS PUT ON A GRID OF 1/64 before the fit (every floating tensor of the source models and of
GraphATABase; the reference's own initialisers draw it first) and stored as small integers.  Both precisions and the
port start from exactly that state and from the float32 run's ``torch.rand`` feature memory.

Recorded per fixture, with a float64 twin run (``f64/...``): the graphs; the seeds (torch 827 before ``init_model``,
``random`` 828, ``np.random`` 829, torch 830 after ``init_model``, torch 831 after ``GraphATABase``); the initial state and
the memory; the pretraining losses and accuracies per source; per adaptation epoch the loss, ``ent`` / ``div`` / ``ce``,
the pseudo labels, the sorted neighbour sets, the sparsemax support sizes of the train-mode pass (per layer, the head
last) and the target accuracy; the final ``mem_cls`` / ``mem_fea`` and ``predict``'s output.

A fixture walks its short list of data seeds and takes the first on which the float32 and the float64 run agree on
every discrete figure: pseudo labels, neighbour sets, support sizes (train and eval pass), accuracies, the arg-max of
``predict``.  The seed taken and the smallest gaps seen (at a neighbour boundary or ``|z - tau|`` of a sparsemax; at a
vote, from the second epoch on -- in the first every vote is a tie that goes to class 0) are recorded, float32 then
float64.  Fixture a also carries known answers of the reference's ``SparsemaxFunction`` (``spx/...``).  Runs on one CPU
thread, so that a rerun reproduces the files bit for bit."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _graphata_semantics as sem, _ref_loader
from .make_golden import HERE, np_

EPOCHS, SEEDS = 6, (827, 828, 829, 830, 831)
DATA_SEEDS = (541, 641, 741, 841, 941, 1041)
CONFIGS = {"graphata_fit_a.npz": dict(S=2, num_layers=2, K=5, momentum=0.9, dropout=0.0),
           "graphata_fit_b.npz": dict(S=3, num_layers=1, K=2, momentum=0.5, dropout=0.0),
           "graphata_fit_c.npz": dict(S=2, num_layers=2, K=5, momentum=0.9, dropout=0.5)}
DISCRETE = ("pred", "near", "supp", "supp_eval", "accs", "src_accs")
C = 3


def quantised(v):
    if not np.issubdtype(v.dtype, np.floating):
        return v
    q = np.round(v.astype(np.float64) * sem.GRID)
    assert np.array_equal(q / sem.GRID, v.astype(np.float64)), "the state is not on the grid"
    return q.astype(np.int8 if np.abs(q).max(initial=0) < 128 else np.int16)


def fx(ref, out_dir, name, cfg):
    kw = dict(in_dim=16, hid_dim=16, num_classes=C, num_src_domains=cfg["S"], K=cfg["K"], momentum=cfg["momentum"],
              num_layers=cfg["num_layers"], dropout=cfg["dropout"], lr=0.05, epoch=EPOCHS)
    taken = None
    for seed in DATA_SEEDS:
        sources, t = sem.graphata_graphs(seed, C, cfg["S"])
        r = sem.run_fit(ref, sources, t, kw, SEEDS)
        r64 = sem.run_fit(ref, sources, t, kw, SEEDS, torch.float64, init=r["init"], mem0=r["mem0"])
        same = all(np.array_equal(r[k], r64[k]) for k in DISCRETE) and \
            np.array_equal(r["logits"].argmax(1), r64["logits"].argmax(1))
        print(f"  {name} seed {seed}: discrete figures equal {same}, gap {r['gap']:.2e} {r64['gap']:.2e}, "
              f"vote gap {r['vote_gap']:.2e} {r64['vote_gap']:.2e}")
        if same:
            taken = (seed, sources, t, r, r64)
            break
    if taken is None:
        raise SystemExit(f"{name}: no seed of {DATA_SEEDS} meets the conditions")
    seed, sources, t, r, r64 = taken
    assert np.isfinite(r["losses"]).all() and np.isfinite(r["logits"]).all()
    out = dict(tgt_x=np_(t.x), tgt_ei=np_(t.edge_index).astype(np.int16), tgt_y=np_(t.y).astype(np.int8),
               seeds=np.array(SEEDS, dtype=np.int64), data_seed=np.int64(seed), epochs=np.int64(EPOCHS),
               lr=np.float64(kw["lr"]), S=np.int64(cfg["S"]), num_layers=np.int64(cfg["num_layers"]), K=np.int64(cfg["K"]),
               momentum=np.float64(cfg["momentum"]), dropout=np.float64(cfg["dropout"]), grid=np.float64(sem.GRID),
               gap=np.array([r["gap"], r64["gap"]]), vote_gap=np.array([r["vote_gap"], r64["vote_gap"]]),
               mem0=r["mem0"], pred=r["pred"].astype(np.int8), near=r["near"].astype(np.int16),
               supp=r["supp"].astype(np.int8))
    for i, s in enumerate(sources):
        out.update({f"src{i}_x": np_(s.x), f"src{i}_ei": np_(s.edge_index).astype(np.int16),
                    f"src{i}_y": np_(s.y).astype(np.int8)})
    out.update({"init/" + k: quantised(v) for k, v in r["init"].items()})
    for pre, rr in (("", r), ("f64/", r64)):
        out.update({pre + k: rr[k] for k in ("src_losses", "src_accs", "losses", "accs", "parts", "mem_cls", "logits")})
        out[pre + "mem_fea"] = rr["mem_fea"].astype(np.float32) if pre == "" else rr["mem_fea"]
    if name == "graphata_fit_a.npz":
        out.update(sem.sparsemax_answers(ref))
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    torch.set_num_threads(1)                     # one thread: the CPU reductions run in one order, run after run
    ref = sem.load_graphata(_ref_loader.load_reference())
    for name, cfg in CONFIGS.items():
        fx(ref, a.out, name, cfg)


if __name__ == "__main__":
    main(sys.argv[1:])
