"""Regenerate the DGDA fixture (``dgda_fit3.npz``) by RUNNING THE REFERENCE's ``pygda/nn/dgda_base.py`` and
``pygda/models/dgda.py`` on the PyG stub with the injections of ``_dgda_semantics`` (build container only, needs the
reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_dgda [--out DIR]

The pair is ASN's: 50 source / 40 target nodes, 16 features, 3 classes; each graph has an isolated node that is not
the last (node 5), one duplicate edge, one directed-only edge and one explicit self loop.  Hidden width 16,
``d / y / m`` = 4 / 6 / 5 and ``dec_dim`` 8 (the stacked head is 30 wide, not a multiple of 4), dropout 0, 8-wide
embeddings in place of DeepWalk's.

Recorded: the embeddings, the initial state dict (torch seed 433), a 3-epoch fit -- the 36 ``eps`` draws in call
order, both ``nadj`` of every epoch as ``drop_edges`` returned them (``np.packbits`` of the 0/1 matrix, row-major), the
per-epoch losses and source accuracies, the final parameters --, two successive ``predict`` calls for the target with
the stored adjacency's diagonal after them, and the same fit run in float64 with the same draws (``f64/...``)."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _dgda_semantics, _ref_loader
from .make_golden import HERE, np_
from .make_golden_asn import asn_pair

KW = dict(in_dim=16, hid_dim=16, num_classes=3, dropout=0.0, dec_dim=8, d_dim=4, y_dim=6, m_dim=5, lr=1e-3,
          weight_decay=5e-4, edge_drop_rate=0.1, edge_add_rate=0.1)
EPOCHS, INIT_SEED, EMB_DIM = 3, 433, 8


def fx_dgda(ref, out_dir):
    s, t = asn_pair()
    g = torch.Generator().manual_seed(435)
    emb = (0.5 * torch.randn(s.x.size(0), EMB_DIM, generator=g), 0.5 * torch.randn(t.x.size(0), EMB_DIM, generator=g))
    out = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), tgt_x=np_(t.x), tgt_ei=np_(t.edge_index),
               tgt_y=np_(t.y), emb_s=np_(emb[0]), emb_t=np_(emb[1]), init_seed=np.int64(INIT_SEED))
    r = _dgda_semantics.run_fit(ref, s, t, emb, KW, EPOCHS, INIT_SEED)
    out.update({"init/" + k: v for k, v in r["init"].items()})
    out.update({"final/" + k: v for k, v in r["final"].items()})
    out.update(losses=r["losses"], accs=r["accs"], tgt_logits_1=r["tgt_logits_1"], tgt_logits_2=r["tgt_logits_2"],
               t_adj_diag=r["t_adj_diag"])
    for k, e in enumerate(r["eps"]):
        out[f"eps/{k}"] = e
    for k, a in enumerate(r["nadj"]):
        assert set(np.unique(a)) <= {0.0, 1.0}
        out[f"nadj/{k // 2}/{'st'[k % 2]}"] = np.packbits(a.astype(bool))
    r64 = _dgda_semantics.run_fit(ref, s, t, emb, KW, EPOCHS, INIT_SEED, torch.float64, eps_feed=r["eps"],
                                  nadj_feed=r["nadj"])
    out.update({"f64/final/" + k: v for k, v in r64["final"].items()})
    out.update({"f64/losses": r64["losses"], "f64/tgt_logits_1": r64["tgt_logits_1"],
                "f64/tgt_logits_2": r64["tgt_logits_2"]})
    path = os.path.join(out_dir, "dgda_fit3.npz")
    np.savez_compressed(path, **out)
    print(f"wrote dgda_fit3.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    fx_dgda(_dgda_semantics.load_dgda(_ref_loader.load_reference()), a.out)


if __name__ == "__main__":
    main(sys.argv[1:])
