"""Regenerate the SOGA fixtures (``soga_fit3_*.npz``) by RUNNING THE REFERENCE's ``pygda/models/soga.py``,
``pygda/nn/soga_base.py`` and ``pygda/utils/sampler.py`` on the PyG stub (build container only, needs the reference
checkout and networkx):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_soga [--out DIR]

The pair: 300 source / 260 target nodes (``_soga_semantics.soga_pair``: sepa_pair's graphs and one isolated target
node), 16 class-informative features, hidden width 16, 2 layers, lr 4e-3, 5 negatives, both lambdas 1.  Recorded per
configuration: the graph pair; the three seeds (torch 617, ``random`` 618, ``np.random`` 619); the initial state dict;
both views' three tables (``tables/...``); a fit of 3 pretraining and 3 adaptation epochs -- the pretraining losses,
source accuracies and the smallest top-2 gap of the source logits per epoch (``src_losses``, ``accs``, ``gaps``), the
adaptation losses and their parts (``parts[:, 0..3]`` = loss, IM, NCE_struct, NCE_neigh), the final parameters,
``predict``'s logits for both domains; and the same fit in float64 from the same initial state (``f64/...``).

``accs`` is a count of arg-maxes, so a fit is comparable across arithmetic only if no source node sits on a class
boundary.  A configuration therefore walks its short list of data seeds and takes the first in which the float32 and the
float64 run have the same accuracies and the smallest gap of both is at least ``MIN_GAP``; the seed taken is recorded
(``data_seed``).  Runs on one CPU thread, so that a rerun reproduces the files bit for bit."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _ref_loader, _soga_semantics
from .make_golden import HERE, np_

EPOCHS, SEEDS, MIN_GAP = 3, (617, 618, 619), 1e-4
DATA_SEEDS = (521, 621, 721, 821, 921, 1021, 1121, 1221)
CONFIGS = {"soga_fit3_gcn.npz": ("gcn", 3), "soga_fit3_gin.npz": ("gin", 5), "soga_fit3_gat.npz": ("gat", 5)}


def fx_soga(ref, out_dir, name, gnn, c):
    kw = dict(in_dim=16, hid_dim=16, num_classes=c, num_layers=2, lr=4e-3, gnn=gnn)
    for seed in DATA_SEEDS:
        s, t = _soga_semantics.soga_pair(seed, c)
        r = _soga_semantics.run_fit(ref, s, t, kw, EPOCHS, SEEDS)
        r64 = _soga_semantics.run_fit(ref, s, t, kw, EPOCHS, SEEDS, torch.float64, init=r["init"])
        same = bool((r["accs"] == r64["accs"]).all())
        gap = min(r["gaps"].min(), r64["gaps"].min())
        print(f"  {name} seed {seed}: accuracies equal {same}, smallest gap {gap:.2e}")
        if same and gap >= MIN_GAP:
            break
    else:
        raise SystemExit(f"{name}: no seed of {DATA_SEEDS} meets the conditions")
    assert np.isfinite(r["src_losses"]).all() and np.isfinite(r["tgt_losses"]).all()
    for k, v in r["tables"].items():
        assert np.array_equal(v, r64["tables"][k]), k
    out = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), tgt_x=np_(t.x), tgt_ei=np_(t.edge_index),
               tgt_y=np_(t.y), seeds=np.array(SEEDS, dtype=np.int64), data_seed=np.int64(seed), gnn=np.array(gnn),
               num_classes=np.int64(c))
    out.update({"init/" + k: v for k, v in r["init"].items()})
    out.update({"tables/" + k: v for k, v in r["tables"].items()})
    out.update({"final/" + k: v.astype(np.float32) for k, v in r["final"].items()})
    for k in ("src_losses", "accs", "gaps", "tgt_losses", "parts", "src_logits", "tgt_logits"):
        out[k] = r[k]
    out.update({"f64/final/" + k: v for k, v in r64["final"].items()})
    for k in ("src_losses", "accs", "gaps", "tgt_losses", "parts", "src_logits", "tgt_logits"):
        out["f64/" + k] = r64[k]
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    torch.set_num_threads(1)                     # one thread: the CPU reductions run in one order, run after run
    ref = _soga_semantics.load_soga(_ref_loader.load_reference())
    for name, (gnn, c) in CONFIGS.items():
        fx_soga(ref, a.out, name, gnn, c)


if __name__ == "__main__":
    main(sys.argv[1:])
