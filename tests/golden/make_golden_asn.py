"""Regenerate the ASN fixture (``asn_fit3.npz``) by RUNNING THE REFERENCE's ``pygda/nn/asn_base.py`` and
``pygda/models/asn.py`` on the PyG stub with the torch-sparse ``GCNConv`` shim of ``_asn_semantics`` (build container
only, needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_asn [--out DIR]

The pair: 50 source / 40 target nodes, 16 features, 3 classes.  Each graph has an isolated node that is not the last
(node 5), one duplicate edge, one directed-only edge and one explicit self loop (a diagonal label of 2).

Recorded: both domains' PPMI adjacency as the reference's float32 CSR (``ppmi_{s,t}_crow / _col / _val``) and its
float64 dense form before the cast (``ppmi64_{s,t}``); the initial state dict (torch seed 431); a 3-epoch fit with the
hidden, decoder and discriminator dropout at 0 -- the 24 ``eps`` draws in call order, the per-epoch losses and source
accuracies, the final parameters, ``predict``'s logits for both domains; and the same fit run in float64 with the
same ``eps`` (``f64/...``)."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _asn_semantics, _pyg_stub, _ref_loader
from .make_golden import HERE, np_

KW = dict(in_dim=16, hid_dim=16, hid_dim_vae=5, num_classes=3, step=3, dropout=0.0, lambda_r=1.0, lambda_d=0.1,
          lambda_f=0.001, adv_dim=10, weight_decay=5e-4, lr=1e-2)
EPOCHS, INIT_SEED = 3, 431


def _graph(n, seed):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n, (2 * n,), generator=g), torch.randint(0, n, (2 * n,), generator=g)
    keep = (src != dst) & (src != 5) & (dst != 5)
    src, dst = src[keep], dst[keep]
    src, dst = torch.cat([src, dst]), torch.cat([dst, src])                     # undirected part
    src = torch.cat([src, torch.tensor([n - 1, 0, 3, 8, src[0].item()])])      # last node, directed-only 3 -> 8,
    dst = torch.cat([dst, torch.tensor([0, n - 1, 8, 8, dst[0].item()])])      # self loop 8 -> 8, one duplicate
    return torch.stack([src, dst]).long()


def asn_pair(seed=421, ns=50, nt=40, f=16, c=3):
    g = torch.Generator().manual_seed(seed)
    xs, xt = torch.rand(ns, f, generator=g), torch.rand(nt, f, generator=g)
    ys, yt = torch.randint(0, c, (ns,), generator=g), torch.randint(0, c, (nt,), generator=g)
    return (_pyg_stub.Data(x=xs, edge_index=_graph(ns, seed + 1), y=ys),
            _pyg_stub.Data(x=xt, edge_index=_graph(nt, seed + 2), y=yt))


def fx_asn(ref, out_dir):
    s, t = asn_pair()
    out = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), tgt_x=np_(t.x), tgt_ei=np_(t.edge_index),
               tgt_y=np_(t.y), init_seed=np.int64(INIT_SEED))
    r = _asn_semantics.run_fit(ref, s, t, KW, EPOCHS, INIT_SEED)
    for dom, a in (("s", r["ppmi_s"]), ("t", r["ppmi_t"])):
        out[f"ppmi_{dom}_crow"], out[f"ppmi_{dom}_col"] = np_(a.crow_indices()), np_(a.col_indices())
        out[f"ppmi_{dom}_val"] = np_(a.values())
    m = ref.ASN(device="cpu", verbose=0, **KW)
    out["ppmi64_s"], out["ppmi64_t"] = _asn_semantics.scaled_ppmi64(m, s), _asn_semantics.scaled_ppmi64(m, t)
    out.update({"init/" + k: v for k, v in r["init"].items()})
    out.update({"final/" + k: v for k, v in r["final"].items()})
    out.update(losses=r["losses"], accs=r["accs"],
               src_logits=r["src_logits"], tgt_logits=r["tgt_logits"])
    for k, e in enumerate(r["eps"]):
        out[f"eps/{k}"] = e
    r64 = _asn_semantics.run_fit(ref, s, t, KW, EPOCHS, INIT_SEED, torch.float64, eps_feed=r["eps"])
    out.update({"f64/final/" + k: v for k, v in r64["final"].items()})
    out.update({"f64/losses": r64["losses"], "f64/src_logits": r64["src_logits"], "f64/tgt_logits": r64["tgt_logits"]})
    path = os.path.join(out_dir, "asn_fit3.npz")
    np.savez_compressed(path, **out)
    print(f"wrote asn_fit3.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    fx_asn(_asn_semantics.load_asn(_ref_loader.load_reference()), a.out)


if __name__ == "__main__":
    main(sys.argv[1:])
