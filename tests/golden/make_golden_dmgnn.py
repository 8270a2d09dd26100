"""Regenerate the DMGNN fixture (``dmgnn_fit3.npz``) by RUNNING THE REFERENCE's ``pygda/models/dmgnn.py`` on its
``pygda/nn/acdne_base.py`` and the PyG stub (``to_dense_adj``).  Build container only (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_dmgnn [--out DIR]

The pair and the hyper-parameters are ACDNE's (``make_golden_acdne.acdne_pair`` / ``KW``): 160 source / 130 target
nodes, node 7 of each domain isolated, ``batch_size = 40``, 8 steps per epoch, both domains wrap within an epoch.

SHIM (stated as the issue asks): under numpy >= 2 (NEP 50) ``process_graph`` returns float64 and the reference's
``predict`` then fails in ``torch.mm`` on ``mat1 and mat2 must have the same dtype``.  The fit runs with
``process_graph``'s two outputs cast to float32 (ACDNE's shim: what numpy 1.x value-based casting gives up to rounding
inside process_graph).

Recorded: the pair, the initial state dict (torch seed ``TORCH_SEED``), the per-epoch losses and accuracies of a
3-epoch fit (numpy seed ``NP_SEED``), the source output of every epoch's log line, the final parameters, both
``predict`` outputs (``P + PPMI P``), the same fit restated in float64 (``_dmgnn_semantics``, ``f64/``), and one step
on the final network at given indices (``step/``): the embeddings, the two ``batch_ppmi`` blocks, both
``nei_prox_loss`` values and the propagated logits.

CONDITION asserted here, on the CPU: the accuracy comparison of the tests is exact, so no fp32 near-tie may decide an
``argmax(P + PPMI P)``.  In the float64 restatement, for every row of every epoch's source output and of the two final
outputs, the gap between the two largest entries exceeds 100 times the largest |reference fp32 - float64| of that
output."""
import argparse
import os
import sys

import numpy as np
import torch

from . import _dmgnn_semantics, _ref_loader
from .make_golden import HERE, np_, sd_arrays
from .make_golden_acdne import KW, acdne_pair, load_acdne

# ACDNE's seeds 411 / 412 do not meet the condition (epoch 2: smallest top-2 gap 6.453e-05 against 100 x 3.042e-06);
# 421 / 422 do (smallest gap 3.880e-03 against errors below 3.4e-06) and are recorded in the fixture as ``seeds``.
TORCH_SEED, NP_SEED = 421, 422


def load_dmgnn(ref=None):
    ref = load_acdne(ref)
    dm = _ref_loader._load("pygda.models.dmgnn", "pygda/models/dmgnn.py")
    ref.DMGNN = dm.DMGNN
    return ref


def _fit(ref, s, t):
    import pygda.models.dmgnn as dmod
    m = ref.DMGNN(device="cpu", epoch=3, verbose=0, **KW)
    rec, log, epoch_out = {}, [], []
    init = m.init_model

    def init_rec(**k):
        net = init(**k)
        rec.update(sd_arrays(net, "init/"))
        return net

    pg = m.process_graph

    def pg32(data):
        a, x = pg(data)
        return a.astype(np.float32), x.astype(np.float32)

    predict = m.predict

    def predict_rec(data, train=False):
        out, y = predict(data, train=train)
        if train:
            epoch_out.append(np_(out))
        return out, y

    m.init_model, m.process_graph, m.predict = init_rec, pg32, predict_rec
    orig = dmod.logger
    dmod.logger = lambda **k: log.append((k["loss"], k["source_train_acc"]))
    try:
        torch.manual_seed(TORCH_SEED)
        np.random.seed(NP_SEED)
        m.fit(s, t)
    finally:
        dmod.logger = orig
    m.predict = predict
    epoch_src_out = np.stack(epoch_out)
    sp, _ = m.predict(s, train=True)
    tp, _ = m.predict(t)
    rec.update(sd_arrays(m.dmgnn, "final/"))
    rec.update(losses=np.array([l for l, _ in log], dtype=np.float64), accs=np.array([a for _, a in log]),
               epoch_src_out=epoch_src_out, src_out=np_(sp), tgt_out=np_(tp),
               seeds=np.array([TORCH_SEED, NP_SEED]))
    # one step of the final network at given indices: rows and PPMI indices coincide (no wrap)
    rng = np.random.RandomState(413)
    ns, half = s.x.shape[0], int(KW["batch_size"] / 2)
    bi_s, bi_t = rng.permutation(ns)[:half], rng.permutation(t.x.shape[0])[:half]
    a_s, a_t = m.batch_ppmi(KW["batch_size"], bi_s, bi_t, m.ppmi_s, m.ppmi_t)
    a_s, a_t = torch.FloatTensor(a_s), torch.FloatTensor(a_t)
    rows = torch.tensor(np.concatenate([bi_s, bi_t + ns]))
    m.dmgnn.eval()
    with torch.no_grad():
        emb, logit, _ = m.dmgnn(m.whole_xs_xt_stt[rows], m.whole_xs_xt_stt_nei[rows], 1)
        prox = torch.stack([m.nei_prox_loss(emb[:half], a_s), m.nei_prox_loss(emb[half:], a_t)])
        logit = logit + torch.cat((torch.mm(a_s, logit[:half]), torch.mm(a_t, logit[half:])), dim=0)
    rec.update({"step/idx_s": bi_s, "step/idx_t": bi_t, "step/a_s": np_(a_s), "step/a_t": np_(a_t),
                "step/emb": np_(emb), "step/prox": np_(prox), "step/logits": np_(logit)})
    return rec


def check_gaps(fit):
    """The condition of the module docstring; raises with the figures when it does not hold."""
    for k in ("epoch_src_out", "src_out", "tgt_out"):
        f64, ref32 = fit["f64/" + k], fit[k].astype(np.float64)
        f64, ref32 = f64.reshape(-1, *f64.shape[-2:]), ref32.reshape(-1, *ref32.shape[-2:])
        for e in range(f64.shape[0]):
            err = np.abs(ref32[e] - f64[e]).max()
            top = np.sort(f64[e], axis=1)
            gap = (top[:, -1] - top[:, -2]).min()
            print(f"{k}[{e}]: smallest top-2 gap {gap:.3e}, largest |ref32 - f64| {err:.3e}")
            assert gap > 100 * err, (f"{k}[{e}]: the smallest top-2 gap {gap:.3e} is within 100 x {err:.3e}: an fp32 "
                                     "near-tie could decide an argmax; choose other seeds")


def fx_dmgnn(ref, out_dir):
    s, t = acdne_pair()
    pair = dict(src_x=np_(s.x), src_ei=np_(s.edge_index), src_y=np_(s.y), tgt_x=np_(t.x), tgt_ei=np_(t.edge_index),
                tgt_y=np_(t.y))
    fit = _fit(ref, s, t)
    init = {k[len("init/"):]: v for k, v in fit.items() if k.startswith("init/")}
    sem = _dmgnn_semantics.fit(dict(x=np_(s.x), ei=np_(s.edge_index), y=np_(s.y)),
                               dict(x=np_(t.x), ei=np_(t.edge_index), y=np_(t.y)), init, KW["hid_dim"], KW["n_emb"],
                               KW["num_classes"], KW["step"], KW["pair_weight"], KW["lr"], KW["weight_decay"], 3,
                               KW["batch_size"], NP_SEED)
    fit.update({"f64/" + k: v for k, v in sem.items()})
    check_gaps(fit)
    path = os.path.join(out_dir, "dmgnn_fit3.npz")
    np.savez_compressed(path, **pair, **fit)
    print(f"wrote dmgnn_fit3.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args(argv)
    fx_dmgnn(load_dmgnn(), a.out)


if __name__ == "__main__":
    main(sys.argv[1:])
