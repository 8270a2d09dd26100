"""DGDA fixture support: the drivers that run the reference's own ``dgda.py`` / ``dgda_base.py`` on the PyG stub (build
container only, via ``make_golden_dgda``), and what is injected around them.

INJECTED (``_pyg_stub.py`` is not edited):
- ``DWPretrain``: PyG's ``Node2Vec`` is not installed, so the reference's DeepWalk cannot run.  ``GivenEmbeddings`` has
  its interface and returns embeddings chosen by the fixture; the trainer under test receives the same ones through
  ``pretrained_emb``.
- ``to_dense_adj``: the stub's version with the dtype of the run (the float64 rerun needs a float64 adjacency).
- in the float64 rerun only, ``F.binary_cross_entropy_with_logits`` receives its target in the input's dtype
  (``DGDA_loss`` builds the domain labels with ``.float()``).

RECORDED by wrapping, not by editing: ``GNN_VGAE_Encoder.repara`` (the ``eps`` of every call, or the given ones fed
back), ``DGDA.drop_edges`` (the ``nadj`` it returns, or the given ones fed back), ``DGDA.init_model`` (the initial state,
dropout as configured) and the module's ``logger``."""
import types

import numpy as np
import torch

from . import _pyg_stub


class GivenEmbeddings:
    table = {}

    def __init__(self, data, *a, **k):
        self.data = data

    def fit(self):
        pass

    def get_embedding(self):
        return GivenEmbeddings.table[id(self.data)]


def load_dgda(ref):
    import sys
    from . import _ref_loader
    db = _ref_loader._load("pygda.nn.dgda_base", "pygda/nn/dgda_base.py")
    nn_pkg = sys.modules["pygda.nn"]
    nn_pkg.DGDABase, nn_pkg.DWPretrain = db.DGDABase, GivenEmbeddings
    dm = _ref_loader._load("pygda.models.dgda", "pygda/models/dgda.py")
    ref.DGDABase, ref.DGDA, ref.dgda_base, ref.dgda_module = db.DGDABase, dm.DGDA, db, dm
    return ref


def run_fit(ref, s, t, emb, kw, epochs, init_seed, dtype=torch.float32, eps_feed=None, nadj_feed=None):
    """The reference's ``DGDA.fit`` and two ``predict`` calls.  Records ``eps`` and ``nadj`` as drawn (feeds None) or
    feeds the given ones.  ``dtype`` float64 runs the same lines in double."""
    dm, db = ref.dgda_module, ref.dgda_base
    s = _pyg_stub.Data(x=s.x.to(dtype), edge_index=s.edge_index, y=s.y)
    t = _pyg_stub.Data(x=t.x.to(dtype), edge_index=t.edge_index, y=t.y)
    GivenEmbeddings.table = {id(s): emb[0].to(dtype), id(t): emb[1].to(dtype)}
    m = ref.DGDA(device="cpu", epoch=epochs, verbose=0, **kw)
    rec, log, eps, nadj = {}, [], [], []
    efeed = list(eps_feed) if eps_feed is not None else None
    nfeed = list(nadj_feed) if nadj_feed is not None else None
    init = m.init_model

    def init_rec(**k):
        net = init(**k)
        rec["init"] = {k2: v.detach().to(torch.float32).numpy().copy() for k2, v in net.state_dict().items()}
        return net.to(dtype)

    def repara(self, mu, lv):
        if not self.training:
            return mu
        e = torch.randn_like(lv) if efeed is None else torch.as_tensor(efeed.pop(0), dtype=lv.dtype)
        eps.append(e.detach().to(torch.float32).numpy().copy())
        return mu + e * torch.exp(lv)

    drop = m.drop_edges

    def drop_rec(adj, drop_rate=0.0, add_rate=0.0):
        if nfeed is not None:
            out = torch.as_tensor(nfeed.pop(0), dtype=adj.dtype).clone()
        else:
            out, _ = drop(adj, drop_rate, add_rate)
        nadj.append(out.detach().to(torch.float32).numpy().copy())
        return out, None

    def to_dense_adj(edge_index, *a, **k):
        return _pyg_stub.to_dense_adj(edge_index, *a, **k).to(dtype)

    real_f = dm.F
    shim = types.SimpleNamespace(**{k: getattr(real_f, k) for k in dir(real_f) if not k.startswith("__")})
    shim.binary_cross_entropy_with_logits = lambda input, target, **k: \
        real_f.binary_cross_entropy_with_logits(input, target.to(input.dtype), **k)
    m.init_model, m.drop_edges = init_rec, drop_rec
    old = (db.GNN_VGAE_Encoder.repara, dm.logger, dm.to_dense_adj, dm.F)
    db.GNN_VGAE_Encoder.repara = repara
    dm.logger = lambda **k: log.append((k["loss"], k["source_train_acc"]))
    dm.to_dense_adj = to_dense_adj
    if dtype == torch.float64:
        dm.F = shim
    try:
        torch.manual_seed(init_seed)
        m.fit(s, t)
        p1, _ = m.predict(t)
        p2, _ = m.predict(t)
    finally:
        db.GNN_VGAE_Encoder.repara, dm.logger, dm.to_dense_adj, dm.F = old
    final = {k: v.detach().double().numpy().copy() for k, v in m.dgda.state_dict().items()}
    return dict(init=rec["init"], final=final, eps=eps, nadj=nadj,
                losses=np.array([l for l, _ in log], dtype=np.float64),
                accs=np.array([a for _, a in log], dtype=np.float64),
                tgt_logits_1=p1.detach().double().numpy(), tgt_logits_2=p2.detach().double().numpy(),
                t_adj_diag=m.t_adj.diagonal().detach().double().numpy().copy())
