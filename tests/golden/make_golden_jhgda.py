"""Regenerate the JHGDA fixtures (``jhgda_fit3.npz``, ``jhgda_fit3_sparse_share.npz``) by RUNNING THE REFERENCE's
``pygda/nn/jhgda_base.py``, ``pygda/nn/gmm_clustering.py`` and ``pygda/models/jhgda.py`` on the PyG stub with the two
shims of ``_jhgda_semantics`` (build container only, needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_jhgda [--out DIR]

The pair: 300 source / 260 target nodes (pooled widths 60 / 12 / 2 and 52 / 10 / 2), 16 features, 3 classes; each
graph has one duplicate edge, one directed-only edge and one explicit self loop.  Recorded per configuration (the
defaults; ``sparse=True, share=True``): the initial state dict (torch seed 517); a 3-epoch fit -- per-epoch losses,
their label_matching sums (``lm``, an argmax count) and source accuracies, the final parameters, ``predict``'s logits
for both domains; and the same fit in float64 from the same initial state (``f64/...``).  Runs on one CPU thread, so
that a rerun reproduces the files bit for bit."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _jhgda_semantics, _pyg_stub, _ref_loader
from .make_golden import HERE, np_

KW = dict(in_dim=16, hid_dim=16, num_classes=3, num_layers=3, lr=4e-3)
CONFIGS = {"jhgda_fit3.npz": dict(), "jhgda_fit3_sparse_share.npz": dict(sparse=True, share=True)}
EPOCHS, INIT_SEED = 3, 517


def _graph(n, seed):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n, (2 * n,), generator=g), torch.randint(0, n, (2 * n,), generator=g)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    src, dst = torch.cat([src, dst]), torch.cat([dst, src])
    src = torch.cat([src, torch.tensor([n - 1, 3, 8, src[0].item()])])      # directed-only n-1 -> 0 and 3 -> 8,
    dst = torch.cat([dst, torch.tensor([0, 8, 8, dst[0].item()])])          # self loop 8 -> 8, one duplicate
    return torch.stack([src, dst]).long()


def jhgda_pair(seed=511, ns=300, nt=260, f=16, c=3):
    g = torch.Generator().manual_seed(seed)
    xs, xt = torch.rand(ns, f, generator=g), torch.rand(nt, f, generator=g)
    ys, yt = torch.randint(0, c, (ns,), generator=g), torch.randint(0, c, (nt,), generator=g)
    return (_pyg_stub.Data(x=xs, edge_index=_graph(ns, seed + 1), y=ys),
            _pyg_stub.Data(x=xt, edge_index=_graph(nt, seed + 2), y=yt))


def fx_jhgda(ref, out_dir, name, extra):
    s, t = jhgda_pair()
    kw = dict(KW, **extra)
    out = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), tgt_x=np_(t.x), tgt_ei=np_(t.edge_index),
               tgt_y=np_(t.y), init_seed=np.int64(INIT_SEED))
    r = _jhgda_semantics.run_fit(ref, s, t, kw, EPOCHS, INIT_SEED)
    out.update({"init/" + k: v for k, v in r["init"].items()})
    out.update({"final/" + k: v.astype(np.float32) for k, v in r["final"].items()})
    out.update(losses=r["losses"], lm=r["lm"], accs=r["accs"], src_logits=r["src_logits"], tgt_logits=r["tgt_logits"])
    r64 = _jhgda_semantics.run_fit(ref, s, t, kw, EPOCHS, INIT_SEED, torch.float64)
    out.update({"f64/final/" + k: v for k, v in r64["final"].items()})
    out.update({"f64/losses": r64["losses"], "f64/src_logits": r64["src_logits"], "f64/tgt_logits": r64["tgt_logits"]})
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **out)
    print(f"wrote {name}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    torch.set_num_threads(1)                     # one thread: the CPU reductions run in one order, run after run
    ref = _jhgda_semantics.load_jhgda(_ref_loader.load_reference())
    for name, extra in CONFIGS.items():
        fx_jhgda(ref, a.out, name, extra)


if __name__ == "__main__":
    main(sys.argv[1:])
