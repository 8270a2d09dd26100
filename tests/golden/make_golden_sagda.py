"""Regenerate the SAGDA fixtures (``faconv.npz``, ``sagda_fit3_l1.npz``, ``sagda_fit3_l2.npz``) by RUNNING THE
REFERENCE's ``pygda/nn/sagda_base.py`` and ``pygda/models/sagda.py`` on the PyG stub plus the FAConv stand-in of
``_faconv_semantics.py`` (its numbered assumptions F1-F7).  Build container only (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_sagda [--out DIR] [name ...]
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import _faconv_semantics, _ref_loader
from .make_golden import HERE, _domain_pair, _pair_arrays, _zero_dropout, grads, make_graph, np_, sd_arrays


def load_sagda(ref=None):
    """The reference namespace of ``_ref_loader.load_reference()`` plus ``SAGDABase`` / ``SAGDA``, the reference's
    files executed against ``torch_geometric.nn.FAConv`` = the stand-in."""
    ref = ref or _ref_loader.load_reference()
    sys.modules["torch_geometric.nn"].FAConv = _faconv_semantics.FAConv
    sab = _ref_loader._load("pygda.nn.sagda_base", "pygda/nn/sagda_base.py")
    sys.modules["pygda.nn"].SAGDABase = sab.SAGDABase
    sg = _ref_loader._load("pygda.models.sagda", "pygda/models/sagda.py")
    ref.SAGNN, ref.SrcGNN, ref.SAGDABase, ref.SAGDA = sab.SAGNN, sab.SrcGNN, sab.SAGDABase, sg.SAGDA
    return ref


def _save(out_dir, name, **arrays):
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {name}.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")


# graphs with existing self loops, duplicate edges, directed edges and an isolated node (the last one)
FACONV_CASES = {"w12": (40, 12, 90, 201), "w8": (30, 8, 70, 202)}


def fx_faconv(ref, out_dir):
    """One FAConv layer (stand-in) called as SAGNN calls it, conv(x, x, edge_index): output and the gradients of x,
    att_l and att_r under a random upstream gradient."""
    arrs = {}
    for name, (n, f, e, seed) in FACONV_CASES.items():
        ei = make_graph(n, e, seed, undirected=False, self_loops=3, dups=4, isolated=True)
        g = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(n, f, generator=g).requires_grad_(True)
        gy = torch.randn(n, f, generator=g)
        torch.manual_seed(seed + 2)
        conv = _faconv_semantics.FAConv(f)
        out = conv(x, x, ei)
        out.backward(gy)
        arrs.update({f"{name}/edge_index": np_(ei), f"{name}/x": np_(x), f"{name}/gy": np_(gy), f"{name}/out": np_(out),
                     f"{name}/gx": np_(x.grad), f"{name}/att_l": np_(conv.att_l.weight),
                     f"{name}/att_r": np_(conv.att_r.weight), f"{name}/g_att_l": np_(conv.att_l.weight.grad),
                     f"{name}/g_att_r": np_(conv.att_r.weight.grad)})
    _save(out_dir, "faconv", **arrs)


def fx_sagda_fit(ref, out_dir):
    """SAGDA.fit for three epochs, num_layers 1 and 2, ppmi=True, every Dropout zeroed: per-epoch loss and source
    accuracy, the initial and final parameters, the last step's gradients (the shared conv weights listed three times
    by the optimiser, sagda.py:249), predict(t), predict(s, source=True), and the PPMI graphs the reference walked."""
    import pygda.models.sagda as smod
    s, t = _domain_pair(211, ns=60, nt=50, f=12, c=3)
    for layers in (1, 2):
        losses, accs = [], []
        orig = smod.logger
        smod.logger = lambda **kw_: (losses.append(kw_["loss"]), accs.append(kw_["source_train_acc"]))
        init_arrays = {}
        try:
            m = ref.SAGDA(12, 8, 3, num_layers=layers, ppmi=True, adv_dim=6, lr=0.01, weight_decay=0.003,
                          device="cpu", epoch=3, verbose=0)
            init = m.init_model

            def init_zero(**k):
                net = init(**k)
                _zero_dropout(net)
                init_arrays.update(sd_arrays(net, "init/"))
                return net

            m.init_model = init_zero
            torch.manual_seed(212)
            np.random.seed(213)
            m.fit(s, t)
            arrs = dict(_pair_arrays(s, t), seed=np.int64(212), np_seed=np.int64(213), num_layers=np.int64(layers),
                        losses=np.array(losses, dtype=np.float64), accs=np.array(accs, dtype=np.float64))
            arrs.update(grads(m.sagda, "grad/"))
            logits, labels = m.predict(t)
            slogits, slabels = m.predict(s, source=True)
        finally:
            smod.logger = orig
        arrs.update(init_arrays)
        arrs.update(tgt_logits=np_(logits), tgt_labels=np_(labels), src_logits=np_(slogits), src_labels=np_(slabels))
        for name in ("source", "target"):
            for li, conv in enumerate(m.sagda.ppmi_encoder.conv_layers):
                if name in conv.cache_dict:
                    ei, w = conv.cache_dict[name]
                    arrs[f"ppmi/{name}/{li}/edge_index"], arrs[f"ppmi/{name}/{li}/weight"] = np_(ei), np_(w)
        arrs.update(sd_arrays(m.sagda, "final/"))
        _save(out_dir, f"sagda_fit3_l{layers}", **arrs)


FIXTURES = {"faconv": fx_faconv, "sagda_fit": fx_sagda_fit}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("names", nargs="*")
    a = ap.parse_args(argv)
    ref = load_sagda()
    for name in (a.names or list(FIXTURES)):
        FIXTURES[name](ref, a.out)


if __name__ == "__main__":
    main(sys.argv[1:])
