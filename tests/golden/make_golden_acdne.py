"""Regenerate the ACDNE fixtures (``acdne_graph.npz``, ``acdne_fit3.npz``) by RUNNING THE REFERENCE's
``pygda/nn/acdne_base.py`` and ``pygda/models/acdne.py`` on the PyG stub (``to_dense_adj``).  Build container only
(needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_acdne [--out DIR]

The pair: 160 source / 130 target nodes, 24 features, 3 classes; node 7 of each domain isolated (not the last, which
``to_dense_adj`` would drop) and one duplicate edge.  ``batch_size = 40``: 20 rows per domain and step, 8 steps per
epoch, both domains wrap within an epoch.

SHIM (stated as the issue asks): under numpy >= 2 (NEP 50) ``a_k / k`` in ``agg_tran_prob_mat`` is float64 for
step >= 2, ``A_ppmi`` / ``X_nei`` follow, and the reference's first ``predict`` fails on a dtype mismatch.  The fit
runs with ``process_graph``'s two outputs cast to float32 (what numpy 1.x value-based casting gives up to rounding
inside process_graph).  The un-shimmed float64 outputs are recorded too (``ppmi64_*`` / ``xnei64_*``).

Recorded: process_graph of the source graph at step 1, 2, 3 (float64 and the float32 cast), ``batch_ppmi`` for given
indices, the initial state dict (torch seed 411), the per-epoch losses and accuracies of a 3-epoch fit (np seed 412),
its final parameters and both ``predict`` outputs, and the same fit restated in float64 (``_acdne_semantics``)."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _acdne_semantics, _pyg_stub, _ref_loader
from .make_golden import HERE, np_, sd_arrays

KW = dict(in_dim=24, hid_dim=16, num_classes=3, n_emb=12, pair_weight=0.1, step=3, dropout=0.0, lr=0.01,
          weight_decay=0.001, batch_size=40)


def load_acdne(ref=None):
    ref = ref or _ref_loader.load_reference()
    ab = _ref_loader._load("pygda.nn.acdne_base", "pygda/nn/acdne_base.py")
    sys.modules["pygda.nn"].ACDNEBase = ab.ACDNEBase
    am = _ref_loader._load("pygda.models.acdne", "pygda/models/acdne.py")
    ref.ACDNEBase, ref.ACDNE = ab.ACDNEBase, am.ACDNE
    return ref


def _graph(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    keep = (src != dst) & (src != 7) & (dst != 7)
    src, dst = src[keep], dst[keep]
    src, dst = torch.cat([src, dst, torch.tensor([n - 1, 0])]), torch.cat([dst, src, torch.tensor([0, n - 1])])
    src, dst = torch.cat([src, src[:1]]), torch.cat([dst, dst[:1]])          # one duplicate edge
    return torch.stack([src, dst]).long()


def acdne_pair(seed=401, ns=160, nt=130, f=24, c=3):
    g = torch.Generator().manual_seed(seed)
    xs = (torch.rand(ns, f, generator=g) < 0.15).float()
    xt = (torch.rand(nt, f, generator=g) < 0.2).float()
    ys = torch.randint(0, c, (ns,), generator=g)
    yt = torch.randint(0, c, (nt,), generator=g)
    return (_pyg_stub.Data(x=xs, edge_index=_graph(ns, 360, seed + 1), y=ys),
            _pyg_stub.Data(x=xt, edge_index=_graph(nt, 300, seed + 2), y=yt))


def _fit(ref, s, t):
    import pygda.models.acdne as amod
    m = ref.ACDNE(device="cpu", epoch=3, verbose=0, **KW)
    rec, log = {}, []
    init = m.init_model

    def init_rec(**k):
        net = init(**k)
        rec.update(sd_arrays(net, "init/"))
        return net

    pg = m.process_graph

    def pg32(data):
        a, x = pg(data)
        return a.astype(np.float32), x.astype(np.float32)

    m.init_model, m.process_graph = init_rec, pg32
    orig = amod.logger
    amod.logger = lambda **k: log.append((k["loss"], k["source_train_acc"]))
    try:
        torch.manual_seed(411)
        np.random.seed(412)
        m.fit(s, t)
    finally:
        amod.logger = orig
    sp, _ = m.predict(s, train=True)
    tp, _ = m.predict(t)
    rec.update(sd_arrays(m.acdne, "final/"))
    rec.update(losses=np.array([l for l, _ in log], dtype=np.float64), accs=np.array([a for _, a in log]),
               src_prob=np_(sp), tgt_prob=np_(tp))
    return rec


def fx_acdne(ref, out_dir):
    s, t = acdne_pair()
    pair = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), tgt_x=np_(t.x), tgt_ei=np_(t.edge_index),
                tgt_y=np_(t.y))
    graph = dict(pair)
    m = ref.ACDNE(device="cpu", verbose=0, **dict(KW, step=1))
    for step in (1, 2, 3):
        m.step = step
        a, x = m.process_graph(s)
        graph[f"ppmi64_s{step}"], graph[f"xnei64_s{step}"] = a, x
        graph[f"ppmi32_s{step}"], graph[f"xnei32_s{step}"] = a.astype(np.float32), x.astype(np.float32)
    m.step = 3
    a_t, _ = m.process_graph(t)
    rng = np.random.RandomState(413)
    bi_s, bi_t = rng.permutation(160)[:20], rng.permutation(130)[:20]
    bs, bt = m.batch_ppmi(40, bi_s, bi_t, graph["ppmi32_s3"], a_t.astype(np.float32))
    graph.update(bidx_s=bi_s, bidx_t=bi_t, bppmi_s=bs, bppmi_t=bt)
    _save(out_dir, "acdne_graph", **graph)
    fit = _fit(ref, s, t)
    init = {k[len("init/"):]: v for k, v in fit.items() if k.startswith("init/")}
    sem = _acdne_semantics.fit(dict(x=np_(s.x), ei=np_(s.edge_index), y=np_(s.y)),
                               dict(x=np_(t.x), ei=np_(t.edge_index), y=np_(t.y)), init, KW["hid_dim"], KW["n_emb"],
                               KW["num_classes"], KW["step"], KW["pair_weight"], KW["lr"], KW["weight_decay"], 3,
                               KW["batch_size"], 412)
    fit.update({"f64/" + k: v for k, v in sem.items() if not k.startswith(("ppmi", "xnei"))})
    _save(out_dir, "acdne_fit3", **pair, **fit)


def _save(out_dir, name, **arrays):
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {name}.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    fx_acdne(load_acdne(), a.out)


if __name__ == "__main__":
    main(sys.argv[1:])
