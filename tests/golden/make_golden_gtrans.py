"""Regenerate the GTrans fixtures (``gtrans_fit_plain.npz``, ``gtrans_fit_margin.npz``, and ``gtrans_perturb.npz``) by
RUNNING THE REFERENCE's ``pygda/models/gtrans.py`` and ``pygda/utils/perturb.py`` on the PyG stub (build container
only, needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_gtrans [--out DIR]

The pair: ``_gtrans_semantics.gtrans_pair`` (300 source / 260 target nodes; the target has a duplicate edge, a
directed-only edge, an explicit self loop and an isolated node), 16 class-informative features, 3 classes, hidden width
16, 2 layers, ``ratio=0.1``, ``loop_feat=2``, ``loop_adj=1``, ``epoch=12`` (12 pretraining epochs, 4 adaptation
iterations) and ``lr=0.05``.
Recorded per fixture: the graph pair; the seeds (torch 717, ``random`` 718, ``np.random`` 719) and the initial state; every
edge keep mask (bit-packed, with its length) and permutation in call order, the final sampling's included; the pretraining
losses and accuracies; the loss and both parts of every ``test_time_loss`` call; the flip weights and the raw edge weights
after every iteration, with the coalesced edge list they belong to; the final ``new_feat``, ``edge_index``,
``edge_weight`` and ``predict``'s logits; and the same fit in float64 from the same initial state (``f64/...``).

In the reference as it stands ``optimizer_adj`` never sees a gradient (see ``_gtrans_semantics``), so the flip weights
stay at 1e-7 and ``topk`` in the final sampling runs over ties: no entry exceeds 1e-7 and the gap between the
``n_perturbations``-th and the next entry is 0 in every run, whatever the data (both are recorded: ``top_gap``,
``above_floor``).  A gap condition on the fixture cannot be met by the reference, so the fixtures record what torch's
CPU ``topk`` returns over the ties, and a fixture walks its short list of data seeds only for the first in which the
float32 and the float64 run agree on the source accuracies and on that set; the seed taken is recorded
(``data_seed``).  ``gtrans_perturb.npz`` holds ``project`` and ``get_modified_adj`` on crafted inputs.  Runs on one CPU
thread, so that a rerun reproduces the files bit for bit."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _gtrans_semantics, _ref_loader
from .make_golden import HERE, np_

EPOCHS, SEEDS = 12, (717, 718, 719)
LOOP_FEAT, LOOP_ADJ, C = 2, 1, 3
DATA_SEEDS = (531, 631, 731, 831, 931, 1031, 1131, 1231)
CONFIGS = {"gtrans_fit_plain.npz": -1, "gtrans_fit_margin.npz": 0.3}


def topk_facts(p, k):
    order = np.argsort(-p, kind="stable")
    gap = float(p[order[k - 1]] - p[order[k]]) if k < p.size else float("inf")
    return set(order[:k].tolist()), gap, int((p > 1e-7).sum())


def per_iteration(r, iters):
    calls = r["adj_calls"]
    idx = [it * (LOOP_ADJ + 1) + LOOP_ADJ for it in range(iters)]
    return (np.stack([calls[i][0] for i in idx]), calls[0][1], np.stack([calls[i][2] for i in idx]),
            calls[iters * (LOOP_ADJ + 1) - 1][0])


def fx_gtrans(ref, out_dir, name, margin):
    kw = dict(in_dim=16, hid_dim=16, num_classes=C, num_layers=2, lr=0.05, ratio=0.1, loop_feat=LOOP_FEAT,
              loop_adj=LOOP_ADJ, margin=margin)
    iters = EPOCHS // (LOOP_FEAT + LOOP_ADJ)
    for seed in DATA_SEEDS:
        s, t = _gtrans_semantics.gtrans_pair(seed, C)
        k = int(kw["ratio"] * t.edge_index.shape[1] // 2)
        r = _gtrans_semantics.run_fit(ref, s, t, kw, EPOCHS, SEEDS)
        r64 = _gtrans_semantics.run_fit(ref, s, t, kw, EPOCHS, SEEDS, torch.float64, init=r["init"])
        p32, p64 = per_iteration(r, iters)[3], per_iteration(r64, iters)[3]
        (set32, gap32, pos32), (set64, gap64, pos64) = topk_facts(p32, k), topk_facts(p64, k)
        same = bool((r["accs"] == r64["accs"]).all()) and set32 == set64
        print(f"  {name} seed {seed}: accuracies and top-{k} equal {same}, gaps {gap32:.2e} {gap64:.2e}, "
              f"entries above 1e-7: {pos32} {pos64}")
        if same:
            break
    else:
        raise SystemExit(f"{name}: no seed of {DATA_SEEDS} meets the conditions")
    assert np.isfinite(r["steps"]).all() and len(r["perms"]) == len(r64["perms"]) == EPOCHS // 3 * 3 + 20
    assert all(np.array_equal(a, b) for a, b in zip(r["masks"], r64["masks"]))
    assert all(np.array_equal(a, b) for a, b in zip(r["perms"], r64["perms"]))
    out = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), tgt_x=np_(t.x), tgt_ei=np_(t.edge_index),
               tgt_y=np_(t.y), seeds=np.array(SEEDS, dtype=np.int64), data_seed=np.int64(seed), margin=np.float64(margin),
               n_perturbations=np.int64(k), top_gap=np.array([gap32, gap64]), above_floor=np.array([pos32, pos64]),
               perms=np.stack(r["perms"]).astype(np.int16), mask_len=np.array([m.size for m in r["masks"]], dtype=np.int64),
               masks=np.concatenate([np.packbits(m) for m in r["masks"]]))
    out.update({"init/" + k2: v for k2, v in r["init"].items()})
    for pre, rr in (("", r), ("f64/", r64)):
        p_it, ei_c, w_it, _ = per_iteration(rr, iters)
        steps = np.concatenate([rr["steps"][:, None], rr["parts"]], axis=1)
        out.update({pre + "src_losses": rr["src_losses"], pre + "accs": rr["accs"], pre + "steps": steps,
                    pre + "p_iter": p_it, pre + "w_iter": w_it, pre + "coalesced_ei": ei_c,
                    pre + "new_feat": rr["new_feat"], pre + "edge_index": rr["edge_index"],
                    pre + "edge_weight": rr["edge_weight"], pre + "logits": rr["logits"]})
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    torch.set_num_threads(1)                     # one thread: the CPU reductions run in one order, run after run
    ref = _gtrans_semantics.load_gtrans(_ref_loader.load_reference())
    path = os.path.join(a.out, "gtrans_perturb.npz")
    np.savez_compressed(path, **_gtrans_semantics.crafted(ref))
    print(f"wrote gtrans_perturb.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")
    for name, margin in CONFIGS.items():
        fx_gtrans(ref, a.out, name, margin)


if __name__ == "__main__":
    main(sys.argv[1:])
