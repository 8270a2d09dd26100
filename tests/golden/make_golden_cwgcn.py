"""Regenerate the CWGCN fixtures (``cwgcn_fit3_{gcn,sage,gat,gin}.npz``, ``cwgcn_fit3_mb.npz``,
``cwgcn_graph_fit3_b{0,6}.npz``) by RUNNING THE REFERENCE's ``pygda/nn/cwgcn_base.py`` and ``pygda/models/cwgcn.py``
on the PyG stub (``_pyg_stub``: its numbered assumptions; PyG's ``Data`` answers ``None`` for ``batch``, which node-mode
``predict`` reads, :390).  Dropout is 0 (the trainer's default).  Build container only (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_cwgcn [--out DIR] [name ...]

Per run: the per-epoch losses and accuracies of both stages (2 x 3 + 3 log lines), the initial parameters, the
parameters at the end of stage 1 and at the end of the fit, the requires_grad flags after the freeze, the last
stage-1 batch's ``x_list[1]`` and ``weight`` and the source statistics stage 2 used, and ``predict`` on the target and
the source."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _pyg_stub, _ref_loader
from .make_golden import HERE, _dataset_arrays, _domain_pair, _graph_dataset, _pair_arrays, make_graph, np_, sd_arrays


def load_cwgcn(ref=None):
    ref = ref or _ref_loader.load_reference()
    if not hasattr(_pyg_stub.Data, "batch"):
        _pyg_stub.Data.batch = None
    cwb = _ref_loader._load("pygda.nn.cwgcn_base", "pygda/nn/cwgcn_base.py")
    sys.modules["pygda.nn"].CWGCNBase = cwb.CWGCNBase
    cw = _ref_loader._load("pygda.models.cwgcn", "pygda/models/cwgcn.py")
    ref.CWGCNBase, ref.CWGCN = cwb.CWGCNBase, cw.CWGCN
    return ref


def _save(out_dir, name, **arrays):
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {name}.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")


def _run(ref, src, tgt, seed, predict=True, **kw):
    """One recorded fit: the reference's logger, print, init_model, forward_model and get_src_mean_std wrapped."""
    import pygda.models.cwgcn as cmod
    log, rec = [], {}
    m = ref.CWGCN(device="cpu", epoch=3, verbose=0, **kw)
    init = m.init_model

    def init_rec(**k):
        net = init(**k)
        rec.update(sd_arrays(net, "init/"))
        forward = net.forward

        def forward_rec(*a, **kw_):
            out = forward(*a, **kw_)
            if net.training:                      # the last one of stage 2: its target batch's x_list[1]
                rec["last_t1"] = np_(out[1][1])
            return out

        net.forward = forward_rec
        return net

    fwd = m.forward_model

    def fwd_rec(data):
        out = fwd(data)
        rec["last_x1"], rec["last_weight"] = np_(out[3][1]), np_(out[2])
        rec["last_logits"], rec["last_y"], rec["last_closs"] = np_(out[1]), np_(data.y), np_(out[0])
        rec["_x1_ptr"] = out[3][1].data_ptr()
        return out

    stats = m.get_src_mean_std

    def stats_rec(emb, w):
        out = stats(emb, w)
        if emb.data_ptr() == rec["_x1_ptr"]:                   # the layer-1 call (:312), not layer 0's (:311)
            rec["mean_s"], rec["std_s"] = np_(out[0]), np_(out[1])
        return out

    def print_rec(*a, **k):
        if a and str(a[0]).startswith("Step 2"):
            rec.update(sd_arrays(m.gnn, "stage1/"))

    m.init_model, m.forward_model, m.get_src_mean_std = init_rec, fwd_rec, stats_rec
    orig_logger, orig_print = cmod.logger, getattr(cmod, "print", None)
    cmod.logger = lambda **k: log.append((k["loss"], k.get("source_train_acc", k.get("target"))))
    cmod.print = print_rec
    try:
        torch.manual_seed(seed)
        m.fit(src, tgt)
        rec.pop("_x1_ptr")
        arrs = dict(rec, seed=np.int64(seed), losses=np.array([l for l, _ in log], dtype=np.float64),
                    accs=np.array([a for _, a in log], dtype=np.float64))
        arrs["requires_grad"] = np.array([p.requires_grad for _, p in m.gnn.named_parameters()], dtype=np.bool_)
        if predict:
            logits, labels = m.predict(tgt)
            slogits, slabels = m.predict(src, source=True)
            arrs.update(tgt_logits=np_(logits), tgt_labels=np_(labels), src_logits=np_(slogits),
                        src_labels=np_(slabels))
    finally:
        cmod.logger = orig_logger
        if orig_print is None:
            del cmod.print
        else:
            cmod.print = orig_print
    arrs.update(sd_arrays(m.gnn, "final/"))
    return arrs


def fx_cwgcn_node(ref, out_dir):
    """Node mode, full batch, every backbone: 12 -> 8 -> 8 -> 3 on a 60 / 50-node pair (a sparser one for gin)."""
    s, t = _domain_pair(311, ns=60, nt=50, f=12, c=3)
    for k, gnn in enumerate(("gcn", "sage", "gat", "gin")):
        if gnn == "gin":
            # GIN sums its neighbours unnormalised: on the pair's ~23-neighbour rows the logits grow until every sample
            # weight but one underflows and the source std is rounding noise; a sparser pair keeps the fixture
            # well conditioned
            s, t = _domain_pair(311, ns=60, nt=50, f=12, c=3)
            s.edge_index, t.edge_index = make_graph(60, 50, 312, True, 1, 0), make_graph(50, 50, 313, True, 1, 0)
        arrs = _run(ref, s, t, 321 + k, in_dim=12, hid_dim=8, num_classes=3, gnn=gnn, lr=0.01, weight_decay=0.001)
        _save(out_dir, f"cwgcn_fit3_{gnn}", **_pair_arrays(s, t), **arrs)


def fx_cwgcn_minibatch(ref, out_dir):
    """Node mode, gcn, fan-out -1, batch size 16 on 60 / 50 nodes: 4 batches per domain, every row of a batch in the
    loss (seeds and their 2-hop neighbourhoods)."""
    s, t = _domain_pair(331, ns=60, nt=50, f=12, c=3)
    arrs = _run(ref, s, t, 341, in_dim=12, hid_dim=8, num_classes=3, gnn="gcn", lr=0.01, weight_decay=0.001,
                batch_size=16)
    _save(out_dir, "cwgcn_fit3_mb", **_pair_arrays(s, t), batch_size=np.int64(16), **arrs)


def fx_cwgcn_graph(ref, out_dir):
    """Graph mode, gcn: every graph of a domain in one batch, and batches of six graphs (DataLoader(shuffle=True): the
    shuffles draw from the CPU generator).  predict() is recorded for the one-batch run only (it shuffles too)."""
    # two classes: with six graphs per batch every source batch holds both (the reference raises on one that does not)
    # (12 source graphs: a last batch of ONE graph would give 1 - sum w^2 = 0, NaN source statistics)
    src, tgt = _graph_dataset(351, 12, c=2), _graph_dataset(352, 10, c=2)
    base = dict(_dataset_arrays("src", src), **_dataset_arrays("tgt", tgt))
    for bs in (0, 6):
        arrs = _run(ref, src, tgt, 361, predict=bs == 0, in_dim=10, hid_dim=8, num_classes=2, gnn="gcn",
                    mode="graph", lr=0.01, weight_decay=0.001, batch_size=bs)
        _save(out_dir, f"cwgcn_graph_fit3_b{bs}", **base, batch_size=np.int64(bs), **arrs)


FIXTURES = {"cwgcn_node": fx_cwgcn_node, "cwgcn_minibatch": fx_cwgcn_minibatch, "cwgcn_graph": fx_cwgcn_graph}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("names", nargs="*")
    a = ap.parse_args(argv)
    ref = load_cwgcn()
    for name in (a.names or list(FIXTURES)):
        FIXTURES[name](ref, a.out)


if __name__ == "__main__":
    main(sys.argv[1:])
