"""GraphATA fixture support: the driver that runs the reference's own ``pygda/models/graphata.py`` on
``pygda/nn/graphata_base.py``, ``pygda/nn/node_centric_conv.py`` and ``pygda/nn/gnn_base.py`` (build container only, via
``make_golden_graphata``).

ONE SHIM beside ``_pyg_stub`` (which is left as it is), installed at load time -- what ``node_centric_conv.py`` imports
and the stub lacks:

* ``torch_geometric.nn.conv.SimpleConv``: ``_graphcta_semantics.SimpleConv`` (the mean over the listed in-edges, a
  duplicate counts twice, 0 for a node without one);
* ``torch_geometric.nn.conv.MessagePassing``: the stub's class with a ``propagate`` that hands ``message`` every
  ``<name>_i`` / ``<name>_j`` argument as PyG does -- the keyword ``<name>`` gathered at the edge's target / source
  (the stub's own ``propagate`` knows ``x_i`` / ``x_j`` only, and NodeCentricConv's message takes ``gamma_i``);
* ``torch_scatter.scatter`` (imported, never called by these files): the sum scatter;
* a ``Data`` whose ``batch`` is None, as PyG's answers for a single graph (``predict`` passes it on).

What is recorded is observed from OUTSIDE: ``init_model`` is wrapped on the instance and ``GraphATABase`` in the
trainer module's namespace (both build in float32, put every floating tensor of the state on a grid of 1/64 or load a
given state, note it, convert to the run's dtype and re-seed torch's generator, so that the port can draw the same
dropout masks after loading the same state); ``torch.rand`` is wrapped for the duration of the fit so that the float64
run starts from the float32 run's feature memory; the module's ``logger`` is replaced by a recorder; the module's name
``F`` is replaced by a proxy of ``torch.nn.functional`` that notes the arguments of ``F.normalize`` (the bottleneck's
output and the feature memory of every epoch) and of ``F.cross_entropy`` (the train-mode logits and the pseudo labels)
and alters nothing; ``_threshold_and_support`` is wrapped in ``node_centric_conv``'s namespace (support sizes and the
gap ``min |z - tau|``).  The memory banks are local variables of ``fit``: the recorder keeps its own pair, moved at
every log line by the reference's expressions on the reference's own network in eval mode (the weights are those of
the eval pass the reference just ran), and checks its feature memory against the one ``F.normalize`` sees next epoch."""
import contextlib
import inspect
import io
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

from . import _pyg_stub
from ._graphcta_semantics import SimpleConv
from ._gtrans_semantics import Data as _Data, coalesce

GRID = 64.0


class Data(_Data):
    batch = None              # PyG's Data answers None for the batch vector of a single graph; predict reads it


class MessagePassing(_pyg_stub.MessagePassing):
    def propagate(self, edge_index, size=None, **kwargs):
        assert self.flow == 'source_to_target'
        n = kwargs['x'].size(0)
        src, dst = edge_index[0], edge_index[1]
        margs = {}
        for name in inspect.signature(self.message).parameters:
            if name.endswith('_j'):
                margs[name] = kwargs[name[:-2]].index_select(0, src)
            elif name.endswith('_i'):
                margs[name] = kwargs[name[:-2]].index_select(0, dst)
            else:
                margs[name] = kwargs.get(name)
        msg = self.message(**margs)
        out = torch.zeros((n,) + tuple(msg.shape[1:]), dtype=msg.dtype).index_add_(0, dst, msg)
        if self.aggr == 'mean':
            cnt = torch.zeros(n, dtype=msg.dtype).index_add_(0, dst, torch.ones(dst.numel(), dtype=msg.dtype))
            out = out / cnt.clamp(min=1).view(-1, 1)
        return out


def scatter(src, index, dim=0, out=None, dim_size=None, reduce='sum'):
    assert reduce in ('sum', 'add')
    return _pyg_stub.scatter_add(src, index, dim, out, dim_size)


def load_graphata(ref):
    from . import _ref_loader
    sys.modules["torch_sparse"].coalesce = coalesce
    sys.modules["torch_geometric.data"].Data = Data
    sys.modules["torch_geometric.nn"].SimpleConv = SimpleConv
    conv = sys.modules["torch_geometric.nn.conv"]
    conv.SimpleConv, conv.MessagePassing = SimpleConv, MessagePassing
    sys.modules["torch_scatter"].scatter = scatter
    _ref_loader._load("pygda.utils.perturb", "pygda/utils/perturb.py")
    ncc = _ref_loader._load("pygda.nn.node_centric_conv", "pygda/nn/node_centric_conv.py")
    gb = _ref_loader._load("pygda.nn.graphata_base", "pygda/nn/graphata_base.py")
    sys.modules["pygda.nn"].GraphATABase = gb.GraphATABase
    gm = _ref_loader._load("pygda.models.graphata", "pygda/models/graphata.py")
    ref.GraphATA, ref.graphata_module, ref.ncc_module, ref.graphata_base = gm.GraphATA, gm, ncc, gb
    return ref


def graphata_graphs(seed, c, num_sources):
    """``num_sources`` source graphs of ``_gtrans_semantics.gtrans_pair`` from different data seeds and one target."""
    from ._gtrans_semantics import gtrans_pair
    pairs = [gtrans_pair(seed + 7 * i, c) for i in range(num_sources)]
    plain = lambda d: Data(x=d.x, edge_index=d.edge_index, y=d.y)                                        # noqa: E731
    return [plain(s) for s, _ in pairs], plain(pairs[0][1])


def on_grid(state):
    return {k: (torch.round(v * GRID) / GRID if v.is_floating_point() else v.clone()) for k, v in state.items()}


def sparsemax_answers(ref):
    """Known answers of the reference's ``SparsemaxFunction`` (dim 1, float64): inputs, outputs, a fixed cotangent and
    its gradient, for ``S = 1``, a full tie, one dominant entry and generic rows."""
    g = torch.Generator().manual_seed(5)
    grid = lambda *shape: torch.round(torch.randn(*shape, generator=g, dtype=torch.float64) * 64) / 64   # noqa: E731
    cases = dict(single=grid(4, 1), tie=torch.tensor([[0.5] * 4, [-1.25] * 4, [0.0] * 4], dtype=torch.float64),
                 dominant=torch.tensor([[3.0, 0.5, 1.0], [-2.0, 0.25, -1.5], [0.0, -1.5, -1.125]], dtype=torch.float64),
                 generic3=grid(8, 3), generic8=grid(5, 8))
    out = {}
    for name, a in cases.items():
        x = a.clone().requires_grad_(True)
        y = ref.ncc_module.sparsemax(x.clone(), 1)                       # (forward shifts its argument in place)
        cot = grid(*a.shape)
        (gx,) = torch.autograd.grad(y, x, cot)
        out.update({f"spx/{name}/in": a.numpy(), f"spx/{name}/out": y.detach().numpy(), f"spx/{name}/cot": cot.numpy(),
                    f"spx/{name}/grad": gx.numpy()})
    return out


def run_fit(ref, sources, t, kw, seeds, dtype=torch.float32, init=None, mem0=None):
    """The reference's ``GraphATA.fit`` and ``predict`` under ``seeds`` (torch before ``init_model``, ``random``,
    ``np.random``, torch after ``init_model``, torch after ``GraphATABase``).  ``dtype`` float64 runs the same lines under
    ``torch.set_default_dtype(torch.float64)`` with float64 features; ``init`` (a float32 state) and ``mem0`` (the
    float32 run's ``torch.rand`` draw) make both precisions start alike."""
    gm, ncc = ref.graphata_module, ref.ncc_module
    m = ref.GraphATA(device="cpu", verbose=0, **kw)
    K, C, mu = m.K, m.num_classes, m.momentum
    rec = dict(init={}, src_log=[[] for _ in sources], tgt_log=[], epochs=[], supp=[], gap=[np.inf], quiet=False,
               norm_calls=0, vote_gap=[np.inf])
    mem = {}
    make, Base = m.init_model, gm.GraphATABase

    def settle(net, prefix, seed):
        state = on_grid(net.state_dict()) if init is None else \
            {k: torch.as_tensor(init[prefix + k]) for k in net.state_dict()}
        net.load_state_dict(state)
        rec["init"].update({prefix + k: v.detach().numpy().copy() for k, v in net.state_dict().items()})
        net.to(dtype)
        torch.manual_seed(seed)

    def in_float32(fn, **k):
        old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float32)
        try:
            return fn(**k)
        finally:
            torch.set_default_dtype(old)

    def init_rec(**k):
        models = in_float32(make, **k)
        for i, net in enumerate(models):
            settle(net, f"src{i}/", seeds[3])
        return models

    def base_rec(**k):
        net = in_float32(Base, **k)
        settle(net, "ata/", seeds[4])
        return net

    m.init_model = init_rec
    draw = torch.rand

    def rand_rec(*size, **k):
        out = draw(*size, dtype=torch.float32)                # always drawn: the dropout masks behind it depend on it
        out = out if mem0 is None else torch.as_tensor(mem0)
        rec["mem0"] = out.numpy().copy()
        mem["fea"] = out.to(dtype)
        mem["cls"] = torch.ones(out.size(0), C, dtype=dtype) / C
        return out.to(dtype)

    class FProxy:
        def __getattr__(self, name):
            return getattr(F, name)

        def normalize(self, x, dim=1):
            rec["norm_calls"] += 1
            if rec["norm_calls"] % 2:
                rec["feat"] = x.detach().clone()
            else:
                assert torch.equal(x, mem["fea"]), "the recorder's feature memory left the reference's"
                rec["mem_seen"] = x.detach().clone()
            return F.normalize(x, dim=dim)

        def cross_entropy(self, cls_output, preds):
            with torch.no_grad():
                softmax_out = F.softmax(cls_output, dim=1)
                ent = torch.mean(torch.sum(-softmax_out * torch.log(softmax_out + 1e-8), dim=1))
                mean_softmax = softmax_out.mean(dim=0)
                div = torch.sum(mean_softmax * torch.log(mean_softmax + 1e-5))
                ce = F.cross_entropy(cls_output, preds)
                distance = F.normalize(rec["feat"], dim=1) @ F.normalize(rec["mem_seen"], dim=1).T
                dist = torch.sort(distance, dim=-1, descending=True)
                rec["gap"].append(min(float((dist.values[:, 0] - dist.values[:, 1]).min()),
                                      float((dist.values[:, K] - dist.values[:, K + 1]).min())))
                near = torch.topk(distance, dim=-1, largest=True, k=K + 1)[1][:, 1:]       # the reference's own line:
                #                                    a zero row (dropout) ties with every row, and topk breaks the tie
                if len(rec["epochs"]) > 0:                     # epoch 0: every row of the class memory ties
                    top2 = torch.sort(torch.mean(mem["cls"][near], dim=1), dim=1, descending=True).values
                    rec["vote_gap"].append(float((top2[:, 0] - top2[:, 1]).min()))
                rec["epochs"].append(dict(parts=[float(ent), float(div), float(ce)], pred=preds.numpy().copy(),
                                          near=np.sort(near.numpy(), axis=1)))
            return F.cross_entropy(cls_output, preds)

    tas = ncc._threshold_and_support

    def tas_rec(input, dim=0):
        tau, supp = tas(input, dim=dim)
        if not rec["quiet"]:
            rec["supp"].append(supp.squeeze(dim).numpy().copy())
            rec["gap"].append(float((input - tau).abs().min()))
        return tau, supp

    def log(**k):
        if "source_train_acc" in k:
            rec["src_log"][sum(len(l) >= m.epoch for l in rec["src_log"])].append(
                (float(k["loss"]), float(k["source_train_acc"])))
            return
        rec["tgt_log"].append((float(k["loss"]), float(k["target"])))
        rec["quiet"] = True                                   # the eval pass the reference just ran, once more
        with torch.no_grad():
            net = m.graphata
            assert not net.training
            feat_output = net.feat_bottleneck(t.x, t.edge_index)
            cls_output = net.feat_classifier(feat_output, t.edge_index)
            softmax_out = F.softmax(cls_output, dim=1)
            outputs_target = softmax_out ** 2 / ((softmax_out ** 2).sum(dim=0))
            mem["cls"] = (1.0 - mu) * mem["cls"] + mu * outputs_target.clone()
            mem["fea"] = (1.0 - mu) * mem["fea"] + mu * feat_output.clone()
        rec["quiet"] = False

    if dtype == torch.float64:
        sources = [Data(x=s.x.double(), edge_index=s.edge_index, y=s.y) for s in sources]
        t = Data(x=t.x.double(), edge_index=t.edge_index, y=t.y)
    old = (gm.logger, gm.GraphATABase, gm.F, ncc._threshold_and_support, torch.get_default_dtype())
    gm.logger, gm.GraphATABase, gm.F, ncc._threshold_and_support = log, base_rec, FProxy(), tas_rec
    torch.rand = rand_rec
    try:
        torch.set_default_dtype(dtype)
        torch.manual_seed(seeds[0])
        random.seed(seeds[1])
        np.random.seed(seeds[2])
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            m.fit(sources, t)
            rec["quiet"] = True
            logits, _ = m.predict(t)
    finally:
        gm.logger, gm.GraphATABase, gm.F, ncc._threshold_and_support = old[:4]
        torch.rand = draw
        torch.set_default_dtype(old[4])
    E, L1, n = m.epoch, m.num_layers + 1, t.x.size(0)
    assert len(rec["epochs"]) == E and len(rec["tgt_log"]) == E and len(rec["supp"]) == 3 * L1 * E
    supp = np.stack(rec["supp"]).reshape(E, 3, L1, n)
    return dict(init=rec["init"], mem0=rec["mem0"],
                src_losses=np.array([[l for l, _ in log_] for log_ in rec["src_log"]], dtype=np.float64),
                src_accs=np.array([[a for _, a in log_] for log_ in rec["src_log"]], dtype=np.float64),
                losses=np.array([l for l, _ in rec["tgt_log"]], dtype=np.float64),
                accs=np.array([a for _, a in rec["tgt_log"]], dtype=np.float64),
                parts=np.array([e["parts"] for e in rec["epochs"]], dtype=np.float64),
                pred=np.stack([e["pred"] for e in rec["epochs"]]), near=np.stack([e["near"] for e in rec["epochs"]]),
                supp=supp[:, 0], supp_eval=supp[:, 1], gap=min(rec["gap"]), vote_gap=min(rec["vote_gap"]),
                mem_cls=mem["cls"].double().numpy().copy(), mem_fea=mem["fea"].double().numpy().copy(),
                logits=logits.detach().double().numpy().copy())
