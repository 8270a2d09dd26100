"""SOGA fixture support: the driver that runs the reference's own ``pygda/models/soga.py`` on ``pygda/nn/soga_base.py``
and ``pygda/utils/sampler.py`` (build container only, via ``make_golden_soga``; needs networkx, which the reference's
sampler imports).

TWO SHIMS beside ``_pyg_stub``: a ``torch_geometric.utils.convert`` module whose ``to_networkx`` builds the ``DiGraph``
PyG builds (nodes ``0 .. N-1`` first, then the edges in ``edge_index`` order), and a ``Data`` with ``clone()``, which
``train_target`` calls.  ``SOGA.fit`` then runs unchanged for the four backbones in float32 and float64.

What is recorded per epoch is observed from OUTSIDE the instance: ``NCE_loss``, ``ent`` and ``div`` are wrapped on the
instance (their return values are noted, nothing is altered), a forward hook on the network's ``cce`` notes the
smallest top-2 gap of the source logits, the module's ``logger`` is replaced by a recorder, and ``init_model`` is
wrapped so that the float32 and the float64 run start from one float32 state."""
import random
import sys
import types

import numpy as np
import torch

from . import _pyg_stub


class Data(_pyg_stub.Data):
    def clone(self):
        return Data(x=self.x.clone(), edge_index=self.edge_index.clone(), y=self.y.clone())


def _to_networkx(data, *args, **kwargs):
    import networkx as nx
    G = nx.DiGraph()
    G.add_nodes_from(range(data.num_nodes))
    for u, v in data.edge_index.t().tolist():
        G.add_edge(u, v)
    return G


def load_soga(ref):
    from . import _ref_loader
    if "torch_geometric.utils.convert" not in sys.modules:
        conv = types.ModuleType("torch_geometric.utils.convert")
        conv.to_networkx = _to_networkx
        sys.modules["torch_geometric.utils.convert"] = conv
        sys.modules["torch_geometric.utils"].convert = conv
    smp = _ref_loader._load("pygda.utils.sampler", "pygda/utils/sampler.py")
    U, NN = sys.modules["pygda.utils"], sys.modules["pygda.nn"]
    U.RandomWalker, U.Negative_Sampler = smp.RandomWalker, smp.Negative_Sampler
    base = _ref_loader._load("pygda.nn.soga_base", "pygda/nn/soga_base.py")
    NN.SOGABase = base.SOGABase
    sm = _ref_loader._load("pygda.models.soga", "pygda/models/soga.py")
    ref.SOGA, ref.SOGABase, ref.soga_module = sm.SOGA, base.SOGABase, sm
    return ref


def soga_pair(seed, c):
    """``_sepa_semantics.sepa_pair``'s 300-node source and its target on 259 nodes (one duplicate edge, one
    directed-only edge and one explicit self loop each) plus ONE ISOLATED target node, 259: 260 target nodes."""
    from ._sepa_semantics import sepa_pair
    s, t = sepa_pair(seed, c, nt=259)
    g = torch.Generator().manual_seed(seed + 3)
    x = torch.cat([t.x, torch.randn(1, t.x.size(1), generator=g)])
    y = torch.cat([t.y, torch.randint(0, c, (1,), generator=g)])
    return (Data(x=s.x, edge_index=s.edge_index, y=s.y), Data(x=x, edge_index=t.edge_index, y=y))


def run_fit(ref, s, t, kw, epochs, seeds, dtype=torch.float32, init=None):
    """The reference's ``SOGA.fit`` and both ``predict``s under the three ``seeds`` (torch, ``random``,
    ``np.random``).  ``dtype`` float64 runs the same lines under ``torch.set_default_dtype(torch.float64)`` with float64
    features; ``init`` (a float32 state dict) is loaded into the fresh network, so both precisions start alike."""
    smod = ref.soga_module
    m = ref.SOGA(device="cpu", epoch=epochs, verbose=0, **kw)
    rec, src_log, tgt_log, gaps = {}, [], [], []
    parts = dict(nce=[], ent=[], div=[])
    make = m.init_model

    def init_rec(**k):
        old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float32)
        try:
            net = make(**k)
        finally:
            torch.set_default_dtype(old)
        if init is not None:
            net.load_state_dict({k2: torch.as_tensor(v) for k2, v in init.items()})
        rec["init"] = {k2: v.detach().numpy().copy() for k2, v in net.state_dict().items()}
        net = net.to(dtype)

        def gap_hook(mod, inp, out):
            top = inp[0].detach().topk(2, dim=1).values
            gaps.append(float((top[:, 0] - top[:, 1]).min()))

        net.cce.register_forward_hook(gap_hook)
        return net

    m.init_model = init_rec

    def noting(fn, key):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            parts[key].append(float(out.detach()))
            return out
        return wrapped

    m.NCE_loss, m.ent, m.div = noting(m.NCE_loss, "nce"), noting(m.ent, "ent"), noting(m.div, "div")

    def log(**k):
        if "source_train_acc" in k:
            src_log.append((float(k["loss"]), float(k["source_train_acc"])))
        else:
            tgt_log.append(float(k["loss"].detach()))

    old_log, old_dtype = smod.logger, torch.get_default_dtype()
    smod.logger = log
    if dtype == torch.float64:
        s = Data(x=s.x.double(), edge_index=s.edge_index, y=s.y)
        t = Data(x=t.x.double(), edge_index=t.edge_index, y=t.y)
    try:
        torch.set_default_dtype(dtype)
        torch.manual_seed(seeds[0])
        random.seed(seeds[1])
        np.random.seed(seeds[2])
        m.fit(s, t)
        tgt_logits, _ = m.predict(t)
        m.target_loader = m.source_loader            # predict reads the target loader: the source's logits through it
        src_logits, _ = m.predict(s)
    finally:
        smod.logger = old_log
        torch.set_default_dtype(old_dtype)
    net = m.soga
    tables = {}
    for view in ("struct", "neigh"):
        for name in ("center_nodes", "positive_samples", "negative_samples"):
            tables[f"{name}_{view}"] = getattr(net, f"{name}_{view}").numpy().astype(np.int64).copy()
    nce = np.array(parts["nce"], dtype=np.float64).reshape(epochs, 2)
    im = np.array(parts["ent"], dtype=np.float64) - np.array(parts["div"], dtype=np.float64)
    final = {k: v.detach().double().numpy().copy() for k, v in net.state_dict().items()}
    return dict(init=rec["init"], final=final, tables=tables,
                src_losses=np.array([l for l, _ in src_log], dtype=np.float64),
                accs=np.array([a for _, a in src_log], dtype=np.float64), gaps=np.array(gaps, dtype=np.float64),
                tgt_losses=np.array(tgt_log, dtype=np.float64),
                parts=np.stack([np.array(tgt_log, dtype=np.float64), im, nce[:, 0], nce[:, 1]], axis=1),
                src_logits=src_logits.detach().double().numpy(), tgt_logits=tgt_logits.detach().double().numpy())
