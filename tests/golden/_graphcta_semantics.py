"""GraphCTA fixture support: the driver that runs the reference's own ``pygda/models/graphcta.py`` on
``pygda/utils/perturb.py`` and ``pygda/nn/gnn_base.py`` (build container only, via ``make_golden_graphcta``).

ONE SHIM beside ``_pyg_stub`` and ``_gtrans_semantics`` (whose ``coalesce`` and ``Data`` are reused):

* ``torch_geometric.nn.SimpleConv(aggr='mean')``: ``forward(x, edge_index)`` gives every node the mean of ``x`` over the
  sources of its listed in-edges, one term per listed edge (a duplicate counts twice), 0 for a node without one; no
  weights, no root term (PyG's ``combine_root=None``).  It is installed into the stub's modules at load time.

WHAT THE REFERENCE DOES WITH THE FLIP WEIGHTS is what its GTrans does (see ``_gtrans_semantics``): ``optimizer_adj`` holds
the tensor ``fit`` creates, the loop works on ``perturbed_edge_weight.detach()`` and on what ``project`` returns, so
``optimizer_adj.step()`` finds no gradient; the flip weights stay at 1e-7 (``p_iter`` in the fixtures records it).
``loop_adj=2`` is run once by the generator and what happens is printed (:func:`probe_loop_adj`).

What is recorded is observed from OUTSIDE the instance: ``test_time_loss`` and ``instance_proto_alignment`` are wrapped
on the instance and ``get_modified_adj`` in the module's namespace (return values and arguments are noted, nothing is
altered), the module's ``logger`` is replaced by a recorder (and its ``tqdm`` by the plain iterator), the model steps' losses are read from what ``fit`` prints,
``torch.rand`` is wrapped for the duration of the fit so that the float64 run starts from the float32 run's feature
memory, ``Tensor.float`` means the default dtype during the float64 run (``fit`` multiplies the memory by
``one_hot(...).float()``), and ``init_model`` is wrapped so that both start from one float32 state.  The discrete decisions inside
``test_time_loss`` (arg-max, selected rows, neighbours) are not visible from outside: the wrapper repeats the call's two
forward passes on the reference's own network, without gradient, and takes them with the reference's expressions."""
import contextlib
import io
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

from . import _gtrans_semantics
from ._gtrans_semantics import Data, coalesce


class SimpleConv(torch.nn.Module):
    def __init__(self, aggr='sum', combine_root=None):
        super().__init__()
        assert aggr == 'mean' and combine_root is None
        self.aggr = aggr

    def forward(self, x, edge_index, edge_weight=None):
        assert edge_weight is None
        src, dst = edge_index[0], edge_index[1]
        cnt = torch.zeros(x.size(0), dtype=x.dtype).index_add_(0, dst, torch.ones(dst.numel(), dtype=x.dtype))
        return torch.zeros_like(x).index_add_(0, dst, x[src]) / cnt.clamp(min=1).unsqueeze(-1)


def load_graphcta(ref):
    from . import _ref_loader
    sys.modules["torch_sparse"].coalesce = coalesce
    sys.modules["torch_geometric.data"].Data = Data
    sys.modules["torch_geometric.nn"].SimpleConv = SimpleConv
    pert = _ref_loader._load("pygda.utils.perturb", "pygda/utils/perturb.py")
    gm = _ref_loader._load("pygda.models.graphcta", "pygda/models/graphcta.py")
    ref.GraphCTA, ref.graphcta_module, ref.perturb = gm.GraphCTA, gm, pert
    return ref


def choices(m, feat, edge_index, edge_weight, mem_fea, mem_cls):
    """The discrete decisions of one ``test_time_loss`` call, with the reference's expressions on its own network:
    ``(pred [N], selected [N], the K neighbours' sorted indices [N, K], the smallest gap at a decision boundary)``."""
    with torch.no_grad():
        net = m.graphcta
        net.eval()
        feat_output = net.feat_bottleneck(feat, edge_index, edge_weight)
        cls_output = net.feat_classifier(feat_output, edge_index, edge_weight)
        softmax_out = F.softmax(cls_output, dim=1)
        _, predict = torch.max(softmax_out, 1)
        mean_ent = m.entropy(softmax_out)
        est_p = (mean_ent < mean_ent.mean()).sum().item() / mean_ent.size(0)
        predict = predict.numpy()
        train_idx = np.zeros(predict.shape, dtype=bool)
        top2 = torch.sort(softmax_out, dim=1, descending=True).values
        gap = min(float((top2[:, 0] - top2[:, 1]).min()), float((mean_ent - mean_ent.mean()).abs().min()))
        for c in range(m.num_classes):
            c_idx = np.where(predict == c)[0]
            val, idx_ = torch.sort(mean_ent[c_idx])
            q = int(len(idx_) * est_p / 5)
            train_idx[c_idx[idx_[:q].numpy()]] = True
            if 0 < q < len(idx_):
                gap = min(gap, float(val[q] - val[q - 1]))
        distance = torch.sort(feat_output @ mem_fea.T, dim=-1, descending=True)
        scale = float(feat_output.norm(dim=1).max() * mem_fea.norm(dim=1).max())
        near = distance.indices[:, 1:m.K + 1]
        gap = min(gap, float((distance.values[:, 0] - distance.values[:, 1]).min()) / scale,
                  float((distance.values[:, m.K] - distance.values[:, m.K + 1]).min()) / scale)
        return predict.copy(), train_idx, np.sort(near.numpy(), axis=1), gap


def run_fit(ref, s, t, kw, epochs, seeds, dtype=torch.float32, init=None, mem0=None):
    """The reference's ``GraphCTA.fit`` and ``predict`` under the three ``seeds``.  ``dtype`` float64 runs the same lines
    under ``torch.set_default_dtype(torch.float64)`` with float64 features; ``init`` (a float32 state dict) and ``mem0``
    (the float32 run's ``torch.rand`` draw) make both precisions start alike.  A fit that ``sample_final_edges`` stops
    with its own range assertion is recorded up to there: ``stopped`` holds the message, the final edge list, its weights
    and the logits are empty."""
    gm = ref.graphcta_module
    m = ref.GraphCTA(device="cpu", epoch=epochs, verbose=0, **kw)
    rec, src_log, tt, model, adj_calls = {}, [], [], [], []
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
    ttl, ipa = m.test_time_loss, m.instance_proto_alignment

    def ttl_rec(feat, edge_index, edge_weight, mem_fea, mem_cls):
        out = ttl(feat, edge_index, edge_weight, mem_fea, mem_cls)
        tt.append((float(out.detach()),) + choices(m, feat.detach(), edge_index, edge_weight.detach(), mem_fea, mem_cls))
        return out

    def ipa_rec(feat, center, pred):
        cl, weight = ipa(feat, center, pred)
        model.append((float(cl.detach()), pred.numpy().copy()))
        return cl, weight

    m.test_time_loss, m.instance_proto_alignment = ttl_rec, ipa_rec

    def adj_rec(fn):
        def wrapped(mei, pw, *a, **k):
            ei, w = fn(mei, pw, *a, **k)
            adj_calls.append((pw.detach().numpy().copy(), ei.numpy().copy(), w.detach().double().numpy().copy()))
            return ei, w
        return wrapped

    def log(**k):
        src_log.append((float(k["loss"]), float(k["source_train_acc"])))

    draw = torch.rand

    def rand_rec(*size, **k):
        out = draw(*size, dtype=torch.float32) if mem0 is None else torch.as_tensor(mem0)
        rec["mem0"] = out.numpy().copy()
        return out.to(dtype)

    old = (gm.logger, gm.get_modified_adj, torch.get_default_dtype(), gm.tqdm)
    gm.logger, gm.get_modified_adj, gm.tqdm = log, adj_rec(gm.get_modified_adj), (lambda it: it)
    torch.rand = rand_rec
    to_float = torch.Tensor.float
    if dtype == torch.float64:
        # fit's one_hot(...).float() meets a float64 memory in torch.mm: in the float64 run .float() is the default dtype
        torch.Tensor.float = lambda self, *a, **k: self.to(torch.get_default_dtype())
        s = Data(x=s.x.double(), edge_index=s.edge_index, y=s.y)
        t = Data(x=t.x.double(), edge_index=t.edge_index, y=t.y)
    printed = io.StringIO()
    try:
        torch.set_default_dtype(dtype)
        torch.manual_seed(seeds[0])
        random.seed(seeds[1])
        np.random.seed(seeds[2])
        stopped, logits = "", None
        with contextlib.redirect_stdout(printed), contextlib.redirect_stderr(io.StringIO()):
            try:
                m.fit(s, t)
                logits, _ = m.predict(t)
            except AssertionError as e:                       # sample_final_edges' own range check: everything before
                stopped = str(e)                              # it -- the iterations, the twenty sampling rounds -- ran
    finally:
        gm.logger, gm.get_modified_adj, gm.tqdm = old[0], old[1], old[3]
        torch.rand = draw
        torch.Tensor.float = to_float
        torch.set_default_dtype(old[2])
    model_losses = [float(line.split(": ")[1]) for line in printed.getvalue().splitlines() if line.startswith("Model: ")]
    assert len(model_losses) == len(model)
    return dict(init=rec["init"], mem0=rec["mem0"], adj_calls=adj_calls,
                src_losses=np.array([l for l, _ in src_log], dtype=np.float64),
                accs=np.array([a for _, a in src_log], dtype=np.float64),
                model=np.array([[l, cl] for l, (cl, _) in zip(model_losses, model)], dtype=np.float64),
                model_pred=np.stack([p for _, p in model]), steps=np.array([c[0] for c in tt], dtype=np.float64),
                tt_pred=np.stack([c[1] for c in tt]), tt_sel=np.stack([c[2] for c in tt]),
                tt_near=np.stack([c[3] for c in tt]), gap=min(c[4] for c in tt),
                new_feat=m.new_feat.detach().double().numpy().copy(), stopped=stopped,
                edge_index=np.zeros((2, 0), dtype=np.int64) if stopped else m.edge_index.numpy().copy(),
                edge_weight=np.zeros(0) if stopped else m.edge_weight.detach().double().numpy().copy(),
                logits=np.zeros((0, m.num_classes)) if stopped else logits.detach().double().numpy().copy())


def probe_loop_adj(ref, s, t, kw, epochs, seeds):
    """Whether the reference can run ``loop_adj=2``: ``None`` when the fit ends, else the error it stops with."""
    try:
        run_fit(ref, s, t, dict(kw, loop_adj=2), epochs, seeds)
    except Exception as e:                                    # noqa: BLE001 -- whatever it raises is the finding
        return f"{type(e).__name__}: {e}"
    return None
