"""Regenerate the PairAlign fixture (``pairalign_fit.npz``) by RUNNING THE REFERENCE's ``pygda/models/pa.py`` on the PyG
stub with the injections of ``_pairalign_semantics`` (build container only, needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_pairalign [--out DIR]

The pair: 50 source / 40 target nodes, 16 features (the first four carry the class), 4 classes, ``num_neigh=[-1, -1]``,
a ``train_mask`` with some rows false.  Each graph has an isolated node that is not the last (node 5), one duplicate
edge, one directed-only edge and one explicit self loop.  The ordered class pair (0, 3) has target edges but no source
edge (``beta`` is ``inf`` there before the reference's fix-up) and the pair (3, 1) has edges in neither graph (``nan``).

Fit ``GS``: hidden 16, ``cls_dim`` 8, dropout 0, 12 epochs, ``ew_freq=3``, ``lw_freq=4``, ``label_rw = edge_rw =
weight_CE_src = True`` -- the edge weights move after epochs 2, 5, 8, 11, the label weights after 3, 7, 11 (both after
11).  Fit ``GCN``: 6 epochs, ``backbone='GCN'``, ``label_rw=True``, ``weight_CE_src=False`` (the scalar-mean loss).

Recorded per fit (``GS/...``, ``GCN/...``): the initial state dict, per-epoch losses and source accuracies, after every
epoch ``ew``, ``lw`` and ``edge_weight``, of EVERY program the reference solved (it solves the label program at every
epoch) the epoch, the inputs ``cov``, ``m``, ``mu``, ``lam`` and the solution ``x``, the final parameters, ``predict`` on
both domains and ``y_hat``; once, ``true_ew`` / ``true_lw`` / ``true_beta``.

No float64 rerun of ``pa.py`` is recorded: its ``.float()`` casts and the float32 selector matrices it multiplies the
logits by (``torch.sparse.mm`` refuses mixed dtypes) do not allow one.  The float64 yardstick of the device tests is the
project's host path run in double, which ``tests/test_pairalign_host.py`` pins to this float32 record first."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _pairalign_semantics, _pyg_stub, _ref_loader
from .make_golden import HERE, np_

C, F_IN = 4, 16
COMMON = dict(in_dim=F_IN, hid_dim=16, num_classes=C, cls_dim=8, dropout=0.0, lr=0.02, weight_decay=1e-4, ew_freq=3,
              lw_freq=4, label_rw=True, edge_rw=True)
FITS = dict(GS=(dict(COMMON, backbone="GS", weight_CE_src=True), 12),
            GCN=(dict(COMMON, backbone="GCN", weight_CE_src=False), 6))
INIT_SEED = 441
ABSENT_IN_SOURCE, ABSENT_IN_BOTH = (0, 3), (3, 1)


def _graph(n, y, seed, drop):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n, (3 * n,), generator=g), torch.randint(0, n, (3 * n,), generator=g)
    keep = (src != dst) & (src != 5) & (dst != 5)
    src, dst = src[keep], dst[keep]
    src, dst = torch.cat([src, dst]), torch.cat([dst, src])                     # undirected part
    a, b = int(torch.nonzero(y == 1)[0]), int(torch.nonzero(y == 2)[0])
    src = torch.cat([src, torch.tensor([n - 1, 0, a, b, src[0].item()])])      # last node, directed-only a -> b,
    dst = torch.cat([dst, torch.tensor([0, n - 1, b, b, dst[0].item()])])      # self loop b -> b, one duplicate
    ok = torch.ones_like(src, dtype=torch.bool)
    for p, q in drop:
        ok &= ~((y[src] == p) & (y[dst] == q))
    return torch.stack([src[ok], dst[ok]]).long()


def pairalign_pair(seed=451, ns=50, nt=40):
    g = torch.Generator().manual_seed(seed)
    ys = torch.cat([torch.arange(C), torch.randint(0, C, (ns - C,), generator=g)])
    yt = torch.cat([torch.arange(C), torch.randint(0, C, (nt - C,), generator=g)])
    xs = torch.rand(ns, F_IN, generator=g) + 1.5 * torch.nn.functional.one_hot(ys, F_IN)
    xt = torch.rand(nt, F_IN, generator=g) + 1.2 * torch.nn.functional.one_hot(yt, F_IN)
    mask = torch.rand(ns, generator=g) < 0.7
    mask[:C] = True                                                             # every class is trained on
    s = _pyg_stub.Data(x=xs, edge_index=_graph(ns, ys, seed + 1, [ABSENT_IN_SOURCE, ABSENT_IN_BOTH]), y=ys,
                       train_mask=mask)
    t = _pyg_stub.Data(x=xt, edge_index=_graph(nt, yt, seed + 2, [ABSENT_IN_BOTH]), y=yt)

    def count(d, pair):
        return int(((d.y[d.edge_index[0]] == pair[0]) & (d.y[d.edge_index[1]] == pair[1])).sum())

    assert count(s, ABSENT_IN_SOURCE) == 0 and count(t, ABSENT_IN_SOURCE) > 0
    assert count(s, ABSENT_IN_BOTH) == 0 and count(t, ABSENT_IN_BOTH) == 0
    assert not bool(mask.all()) and 5 not in s.edge_index and 5 not in t.edge_index
    return s, t


def fx_pairalign(ref, out_dir):
    s, t = pairalign_pair()
    out = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), src_mask=np_(s.train_mask), tgt_x=np_(t.x),
               tgt_ei=np_(t.edge_index), tgt_y=np_(t.y), init_seed=np.int64(INIT_SEED))
    for tag, (kw, epochs) in FITS.items():
        r = _pairalign_semantics.run_fit(ref, s, t, kw, epochs, INIT_SEED)
        out.update({f"{tag}/init/{k}": v for k, v in r["init"].items()})
        out.update({f"{tag}/final/{k}": v for k, v in r["final"].items()})
        for k in ("losses", "accs", "ew", "lw", "edge_weight", "src_logits", "tgt_logits", "y_hat"):
            out[f"{tag}/{k}"] = r[k]
        for i, (kind, epoch, cov, m, mu, lam, x) in enumerate(r["solves"]):
            out[f"{tag}/solve/{i}/kind"] = np.array(kind)
            out[f"{tag}/solve/{i}/epoch"] = np.int64(epoch)
            out.update({f"{tag}/solve/{i}/cov": cov, f"{tag}/solve/{i}/m": m, f"{tag}/solve/{i}/mu": mu,
                        f"{tag}/solve/{i}/lam": np.float64(lam), f"{tag}/solve/{i}/x": x})
        out[f"{tag}/n_solves"] = np.int64(len(r["solves"]))
        if tag == "GS":
            out.update(true_ew=r["true_ew"], true_lw=r["true_lw"], true_beta=r["true_beta"])
    path = os.path.join(out_dir, "pairalign_fit.npz")
    np.savez_compressed(path, **out)
    print(f"wrote pairalign_fit.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    fx_pairalign(_pairalign_semantics.load_pairalign(_ref_loader.load_reference()), a.out)


if __name__ == "__main__":
    main(sys.argv[1:])
