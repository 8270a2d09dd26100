"""Regenerate the SEPA fixtures (``sepa_fit3_*.npz``) by RUNNING THE REFERENCE's ``pygda/models/sepa.py`` and
``pygda/nn/gnn_base.py`` on the PyG stub (build container only, needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_sepa [--out DIR]

The pair: 300 source / 260 target nodes, 16 class-informative features (``_sepa_semantics.sepa_pair``), hidden width
16, 2 layers, lr 4e-3.  Recorded per configuration: the graph pair; the initial state dict (torch seed 517); a 3-epoch
fit -- per-epoch losses, source accuracies and the four loss parts (``parts[:, 0..3]`` = loss_im, loss_pp, loss_sep,
nll), the final parameters, ``predict``'s logits for both domains; per epoch the target ``pred``, the count of predicted
classes (``n_pred``) and the smallest top-2 gap of the target probabilities (``gaps``); and the same fit in float64 from
the same initial state (``f64/...``).

``pred`` is an arg-max, so a fit is comparable across arithmetic only if no node sits on a class boundary.  A
configuration therefore walks its short list of data seeds and takes the first in which the float32 and the float64 run
have the same ``pred`` in every epoch, the smallest gap is at least ``MIN_GAP``, and (where the configuration asks for
it) some class is predicted by no node in some epoch; the seed taken is recorded (``data_seed``).  Runs on one CPU
thread, so that a rerun reproduces the files bit for bit."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _ref_loader, _sepa_semantics
from .make_golden import HERE, np_

EPOCHS, INIT_SEED, MIN_GAP = 3, 517, 1e-4
SEEDS = (511, 611, 711, 811, 911, 1011, 1111, 1211)
# name -> (gnn, classes, True: some epoch has an unpredicted class / False: every class predicted in every epoch / None)
CONFIGS = {"sepa_fit3_gcn.npz": ("gcn", 3, False), "sepa_fit3_gat.npz": ("gat", 5, None),
           "sepa_fit3_gin_empty.npz": ("gin", 5, True)}


def _try(ref, gnn, c, seed):
    s, t = _sepa_semantics.sepa_pair(seed, c)
    kw = dict(in_dim=16, hid_dim=16, num_classes=c, num_layers=2, lr=4e-3, gnn=gnn)
    r = _sepa_semantics.run_fit(ref, s, t, kw, EPOCHS, INIT_SEED)
    r64 = _sepa_semantics.run_fit(ref, s, t, kw, EPOCHS, INIT_SEED, torch.float64, init=r["init"])
    return s, t, r, r64


def fx_sepa(ref, out_dir, name, gnn, c, want_empty):
    for seed in SEEDS:
        s, t, r, r64 = _try(ref, gnn, c, seed)
        same = bool((r["pred"] == r64["pred"]).all())
        gap = min(r["gaps"].min(), r64["gaps"].min())
        empty = bool((r["n_pred"] < c).any())
        all_used = bool((r["n_pred"] == c).all())
        print(f"  {name} seed {seed}: pred equal {same}, smallest gap {gap:.2e}, classes predicted {r['n_pred'].tolist()}")
        if same and gap >= MIN_GAP and (want_empty is None or (empty if want_empty else all_used)):
            break
    else:
        raise SystemExit(f"{name}: no seed of {SEEDS} meets the conditions")
    assert same and gap >= MIN_GAP and np.isfinite(r["losses"]).all()
    out = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), tgt_x=np_(t.x), tgt_ei=np_(t.edge_index),
               tgt_y=np_(t.y), init_seed=np.int64(INIT_SEED), data_seed=np.int64(seed), gnn=np.array(gnn),
               num_classes=np.int64(c))
    out.update({"init/" + k: v for k, v in r["init"].items()})
    out.update({"final/" + k: v.astype(np.float32) for k, v in r["final"].items()})
    for k in ("losses", "accs", "parts", "pred", "n_pred", "gaps", "src_logits", "tgt_logits"):
        out[k] = r[k]
    out.update({"f64/final/" + k: v for k, v in r64["final"].items()})
    for k in ("losses", "parts", "pred", "gaps", "src_logits", "tgt_logits"):
        out["f64/" + k] = r64[k]
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    torch.set_num_threads(1)                     # one thread: the CPU reductions run in one order, run after run
    ref = _sepa_semantics.load_sepa(_ref_loader.load_reference())
    for name, (gnn, c, want_empty) in CONFIGS.items():
        fx_sepa(ref, a.out, name, gnn, c, want_empty)


if __name__ == "__main__":
    main(sys.argv[1:])
