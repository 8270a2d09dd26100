"""Regenerate the KBL fixtures (``kbl_fit_a.npz``, ``kbl_fit_b.npz``, ``kbl_fit_c.npz``) by RUNNING THE REFERENCE's
``pygda/models/kbl.py`` on the PyG stub (build container only, needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_kbl [--out DIR]

The pair: ``_kbl_semantics.kbl_pair`` -- ``_gtrans_semantics.gtrans_pair`` (300 source / 260 target nodes, 16
class-informative features) with a source ``train_mask`` that leaves out every fifth node and disjoint ``val`` / ``test``
masks.  ``num_epoch=6`` bridge epochs are passed to ``KBLBase`` (``KBL.init_model`` writes 400; everything else of that
call is restated as it is: width 64, two layers, ``norm_mode='None'``, ``source_clf=True``), ``epoch=4`` classifier
epochs with ``lr=0.01`` and the default weight decay.  Fixture a: 3 classes (the two-of-three class draw runs),
``k_cross=20``, ``k_within=6``; fixture b: 2 classes, ``k_cross=7``, ``k_within=0``; fixture c: a's settings.
IN FIXTURES a AND b ``torch.nn.functional.dropout`` IS REPLACED, for the duration of the reference's fit, by one that
passes ``p=0`` (``_kbl_semantics.run_fit``, ``live_dropout=False``): the device draws its keep bits from another stream,
so a device fit can only be compared without dropout.  Fixture c runs the reference's dropout as it is, for the host fit.

THE INITIAL STATE IS PUT ON A GRID OF 1/64 before the fit (every floating tensor; the reference's own initialisers
draw it first) and stored as small integers: 90 000 parameters in float32 would be three times the size of everything
else.  Both precisions and the port start from exactly that state.

Recorded per fixture: the graph pair with its masks; the seeds (torch 727 before ``init_model``, ``random`` 728,
``np.random`` 729, torch 730 after ``init_model``); the initial state; the two index lists of every bridge epoch (the
40000 pairs are their Cartesian product, which the generator checks); the five stage-1 losses per epoch in the order
``train_adv_few_shot`` returns them (sim, d, ae, g, recons); the BatchNorm running statistics after stage 1; the bridge
edges in ``topk`` order with their values; the within-domain edges of both domains with their values and flat indices;
the merged undirected edge list; the stage-3 losses and accuracies; ``predict``'s output on the target; and the same
run in float64 from the same initial state (``f64/...``).

A fixture walks its short list of data seeds and takes the first on which the float32 and the float64 run agree on
every discrete decision: the pairs, the accuracies, the bridge edges in order, the within-domain edges and the merged
edge list.  The seed taken (``data_seed``) and the gap between the k-th and the (k+1)-th cosine at the ``k_cross``
boundary (``gap``: float32 run, float64 run) are recorded.  Runs on one CPU thread, so that a rerun reproduces the
files bit for bit."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _kbl_semantics, _ref_loader
from .make_golden import HERE, np_

NUM_EPOCH, EPOCHS, SEEDS = 6, 4, (727, 728, 729, 730)
DATA_SEEDS = (541, 641, 741, 841, 941, 1041)
CONFIGS = {"kbl_fit_a.npz": dict(c=3, k_cross=20, k_within=6, live_dropout=False),
           "kbl_fit_b.npz": dict(c=2, k_cross=7, k_within=0, live_dropout=False),
           "kbl_fit_c.npz": dict(c=3, k_cross=20, k_within=6, live_dropout=True)}
DISCRETE = ("ia", "ib", "accs", "cross_row", "cross_col", "merged_ei")


def quantised(v):
    if not np.issubdtype(v.dtype, np.floating):
        return v
    q = np.round(v.astype(np.float64) * _kbl_semantics.GRID)
    assert np.array_equal(q / _kbl_semantics.GRID, v.astype(np.float64)), "the state is not on the grid"
    return q.astype(np.int8 if np.abs(q).max(initial=0) < 128 else np.int16)


def fx_kbl(ref, out_dir, name, cfg):
    c, live = cfg["c"], cfg["live_dropout"]
    kw = dict(in_dim=16, hid_dim=16, num_classes=c, k_cross=cfg["k_cross"], k_within=cfg["k_within"], lr=0.01,
              epoch=EPOCHS)
    taken = None
    for seed in DATA_SEEDS:
        s, t = _kbl_semantics.kbl_pair(seed, c)
        r = _kbl_semantics.run_fit(ref, s, t, kw, NUM_EPOCH, SEEDS, live_dropout=live)
        r64 = _kbl_semantics.run_fit(ref, s, t, kw, NUM_EPOCH, SEEDS, torch.float64, init=r["init"], live_dropout=live)
        same = all(np.array_equal(r[k], r64[k]) for k in DISCRETE) and len(r["within"]) == len(r64["within"]) and \
            all(np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) for a, b in zip(r["within"], r64["within"]))
        print(f"  {name} seed {seed}: discrete decisions equal {same}, gap at k_cross {r['gap']:.2e} {r64['gap']:.2e}")
        if same:
            taken = (seed, s, t, r, r64)
            break
    if taken is None:
        raise SystemExit(f"{name}: no seed of {DATA_SEEDS} meets the conditions")
    seed, s, t, r, r64 = taken
    assert np.isfinite(r["stage1"]).all() and np.isfinite(r["logits"]).all() and len(r["losses"]) == EPOCHS
    out = dict(src_x=np_(s.x), src_ei=np_(s.edge_index).astype(np.int16), src_y=np_(s.y).astype(np.int8),
               tgt_x=np_(t.x), tgt_ei=np_(t.edge_index).astype(np.int16), tgt_y=np_(t.y).astype(np.int8),
               train_mask=np_(s.train_mask), val_mask=np_(s.val_mask), test_mask=np_(s.test_mask),
               seeds=np.array(SEEDS, dtype=np.int64), data_seed=np.int64(seed), num_epoch=np.int64(NUM_EPOCH),
               epochs=np.int64(EPOCHS), lr=np.float64(kw["lr"]), k_cross=np.int64(cfg["k_cross"]),
               k_within=np.int64(cfg["k_within"]), live_dropout=np.bool_(live), gap=np.array([r["gap"], r64["gap"]]),
               grid=np.float64(_kbl_semantics.GRID), ia=r["ia"].astype(np.int16), ib=r["ib"].astype(np.int16),
               cross_row=r["cross_row"].astype(np.int16), cross_col=r["cross_col"].astype(np.int16),
               merged_ei=r["merged_ei"].astype(np.int16))
    out.update({"init/" + k2: quantised(v) for k2, v in r["init"].items()})
    for d, (ei, _, flat) in zip(("src", "tgt"), r["within"]):
        out.update({f"within_{d}_ei": ei.astype(np.int16), f"within_{d}_flat": flat.astype(np.int64)})
    for pre, rr in (("", r), ("f64/", r64)):
        out.update({pre + "stage1": rr["stage1"], pre + "cross_val": rr["cross_val"], pre + "losses": rr["losses"],
                    pre + "accs": rr["accs"], pre + "logits": rr["logits"]})
        out.update({pre + "running/" + k2: v for k2, v in rr["running"].items()})
        for d, (_, val, _) in zip(("src", "tgt"), rr["within"]):
            out[pre + f"within_{d}_val"] = val
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    torch.set_num_threads(1)                     # one thread: the CPU reductions run in one order, run after run
    ref = _kbl_semantics.load_kbl(_ref_loader.load_reference())
    for name, cfg in CONFIGS.items():
        fx_kbl(ref, a.out, name, cfg)


if __name__ == "__main__":
    main(sys.argv[1:])
