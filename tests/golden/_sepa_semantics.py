"""SEPA fixture support: the driver that runs the reference's own ``pygda/models/sepa.py`` on ``pygda/nn/gnn_base.py``
(build container only, via ``make_golden_sepa``).

NO SHIM is needed: ``_pyg_stub`` already provides ``torch_geometric.nn.conv.MessagePassing`` and
``torch_geometric.nn.conv.gcn_conv.gcn_norm``, which is all ``PageRank`` takes from PyG, and ``SEPA.fit`` runs on it
unchanged for the four backbones in float32 and float64.

What is recorded per epoch is observed from OUTSIDE the instance: ``cls_im``, ``proto_alignment``, ``seperate_center``
and ``obtain_target_prototype`` are wrapped on the instance (their return values and the probabilities they receive are
noted, nothing is altered), the module's ``F`` is replaced by a forwarding proxy that notes what ``nll_loss`` returns,
and ``init_model`` is wrapped so that the float32 and the float64 run start from one float32 state."""
import types

import numpy as np
import torch

from . import _pyg_stub


def load_sepa(ref):
    from . import _ref_loader
    sm = _ref_loader._load("pygda.models.sepa", "pygda/models/sepa.py")
    ref.SEPA, ref.PageRank, ref.sepa_module = sm.SEPA, sm.PageRank, sm
    return ref


def sepa_pair(seed, c, ns=300, nt=260, f=16):
    """Class-informative features (``centre[y] + noise``, the target shifted by 0.3) on make_golden_jhgda's graphs
    (one duplicate edge, one directed-only edge and one explicit self loop each)."""
    from .make_golden_jhgda import _graph
    g = torch.Generator().manual_seed(seed)
    cent = torch.randn(c, f, generator=g)
    ys, yt = torch.randint(0, c, (ns,), generator=g), torch.randint(0, c, (nt,), generator=g)
    xs = cent[ys] + torch.randn(ns, f, generator=g)
    xt = cent[yt] + 0.3 + torch.randn(nt, f, generator=g)
    return (_pyg_stub.Data(x=xs, edge_index=_graph(ns, seed + 1), y=ys),
            _pyg_stub.Data(x=xt, edge_index=_graph(nt, seed + 2), y=yt))


def run_fit(ref, s, t, kw, epochs, init_seed, dtype=torch.float32, init=None):
    """The reference's ``SEPA.fit`` and both ``predict``s.  ``dtype`` float64 runs the same lines under
    ``torch.set_default_dtype(torch.float64)`` with float64 features; ``init`` (a float32 state dict) is loaded into the
    fresh backbone, so that both precisions start from the same state."""
    smod = ref.sepa_module
    m = ref.SEPA(device="cpu", epoch=epochs, verbose=0, **kw)
    rec, log = {}, []
    parts = dict(im=[], pp=[], sep=[], nll=[])
    preds, gaps = [], []
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
        return net.to(dtype)

    m.init_model = init_rec

    def noting(fn, key, pick=lambda r: r):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            parts[key].append(float(pick(out).detach()))
            return out
        return wrapped

    m.cls_im = noting(m.cls_im, "im", lambda r: r[0])
    m.proto_alignment = noting(m.proto_alignment, "pp")
    m.seperate_center = noting(m.seperate_center, "sep")
    otp = m.obtain_target_prototype

    def otp_rec(prob, feat, edge_index, ent):
        top = prob.detach().topk(2, dim=1).values
        gaps.append(float((top[:, 0] - top[:, 1]).min()))
        preds.append(torch.max(prob.detach(), dim=1)[1].numpy().copy())
        return otp(prob, feat, edge_index, ent)

    m.obtain_target_prototype = otp_rec
    real_f = smod.F
    proxy = types.SimpleNamespace(**{k: getattr(real_f, k) for k in ("softmax", "normalize", "relu")})
    proxy.nll_loss = noting(real_f.nll_loss, "nll")
    old_log = smod.logger
    smod.logger = lambda **k: log.append((k["loss"], k["source_train_acc"]))
    smod.F = proxy
    old_dtype = torch.get_default_dtype()
    if dtype == torch.float64:
        s = _pyg_stub.Data(x=s.x.double(), edge_index=s.edge_index, y=s.y)
        t = _pyg_stub.Data(x=t.x.double(), edge_index=t.edge_index, y=t.y)
    try:
        torch.set_default_dtype(dtype)
        torch.manual_seed(init_seed)
        m.fit(s, t)
        src_logits, _ = m.predict(s)
        tgt_logits, _ = m.predict(t)
    finally:
        smod.logger, smod.F = old_log, real_f
        torch.set_default_dtype(old_dtype)
    final = {k: v.detach().double().numpy().copy() for k, v in m.gnn.state_dict().items()}
    pred = np.stack(preds).astype(np.int64)
    return dict(init=rec["init"], final=final, losses=np.array([l for l, _ in log], dtype=np.float64),
                accs=np.array([a for _, a in log], dtype=np.float64),
                parts=np.array([parts[k] for k in ("im", "pp", "sep", "nll")], dtype=np.float64).T.copy(),
                pred=pred, n_pred=np.array([np.unique(p).size for p in pred], dtype=np.int64),
                gaps=np.array(gaps, dtype=np.float64), src_logits=src_logits.detach().double().numpy(),
                tgt_logits=tgt_logits.detach().double().numpy())
