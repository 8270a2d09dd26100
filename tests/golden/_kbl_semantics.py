"""KBL fixture support: the driver that runs the reference's own ``pygda/models/kbl.py`` on ``pygda/nn/kbl_base.py`` and
``pygda/nn/gnn_base.py`` (build container only, via ``make_golden_kbl``).

THREE ADDITIONS beside ``_pyg_stub`` (which is left as it is), installed at load time:

* ``Data.coalesce()``: the edge list sorted by (row, col) with duplicates dropped, in place, returning the object (PyG's
  ``Data.coalesce``); ``Data.num_features``: the width of ``x``.
* ``import torch_geometric`` as a top-level name: ``kbl_base.py`` writes ``torch_geometric.utils.coalesce(edge_index)``
  and ``torch_geometric.data.Data(...)``.  The name it sees is a namespace holding those two -- ``coalesce`` with one
  argument returns the edge list alone, as PyG's does (the stub's own returns a pair, for tdss.py).

What is recorded is observed from OUTSIDE: ``init_model`` is wrapped on the instance (it restates the reference's
``KBLBase(...)`` call with ``num_epoch`` replaced, builds the model in float32, puts every floating tensor of its state
on a grid of 1/64 -- so that the fixture can hold it as small integers --, optionally loads a given state, notes it,
converts it to the run's dtype and re-seeds torch's generator, so that the port can draw the same dropout masks after
loading the same state); ``PairEnumerator.sampling``, ``BridgedGraph.train_adv_few_shot``, ``gen_bridged_graph`` and
the two ``add_topk_sim_*_edges_full`` are wrapped in the class (arguments and return values are noted, nothing is
altered; the cross-domain one is called a second time with ``k + 1`` for the gap at the boundary); the module's
``logger`` is replaced by a recorder; ``Tensor.float`` means the default dtype during the float64 run (the pair
targets are ``(y_i == y_j).float()``).  With ``live_dropout=False`` ``torch.nn.functional.dropout`` is replaced, for the
duration of the fit, by one that passes ``p=0``."""
import contextlib
import io
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

from . import _pyg_stub

GRID = 64.0


class Data(_pyg_stub.Data):
    @property
    def num_features(self):
        return self.x.size(1)

    def coalesce(self):
        self.edge_index = coalesce(self.edge_index)
        return self


def coalesce(edge_index, num_nodes=None):
    n = _pyg_stub.maybe_num_nodes(edge_index, num_nodes)
    key = torch.unique(edge_index[0] * n + edge_index[1])
    return torch.stack([key // n, key % n])


def load_kbl(ref):
    from . import _ref_loader
    sys.modules["torch_geometric.data"].Data = Data
    kb = _ref_loader._load("pygda.nn.kbl_base", "pygda/nn/kbl_base.py")
    kb.torch_geometric = types.SimpleNamespace(utils=types.SimpleNamespace(coalesce=coalesce),
                                               data=types.SimpleNamespace(Data=Data))
    sys.modules["pygda.nn"].KBLBase = kb.KBLBase
    km = _ref_loader._load("pygda.models.kbl", "pygda/models/kbl.py")
    ref.KBL, ref.kbl_module, ref.kbl_base = km.KBL, km, kb
    return ref


def kbl_pair(seed, c):
    """``_gtrans_semantics.gtrans_pair``'s graphs with a source ``train_mask`` that leaves out every fifth node and
    disjoint ``val`` / ``test`` masks over the nodes it leaves out."""
    from ._gtrans_semantics import gtrans_pair
    s, t = gtrans_pair(seed, c)
    i = torch.arange(s.x.size(0))
    masks = dict(train_mask=i % 5 != 4, val_mask=i % 10 == 4, test_mask=i % 10 == 9)
    return Data(x=s.x, edge_index=s.edge_index, y=s.y, **masks), Data(x=t.x, edge_index=t.edge_index, y=t.y)


def on_grid(state):
    return {k: (torch.round(v * GRID) / GRID if v.is_floating_point() else v.clone()) for k, v in state.items()}


def run_fit(ref, s, t, kw, num_epoch, seeds, dtype=torch.float32, init=None, live_dropout=False):
    """The reference's ``KBL.fit`` and ``predict`` under ``seeds`` (torch before ``init_model``, ``random``,
    ``np.random``, torch after ``init_model``).  ``dtype`` float64 runs the same lines under
    ``torch.set_default_dtype(torch.float64)`` with float64 features; ``init`` (a float32 state dict) makes both
    precisions start alike."""
    kb, km = ref.kbl_base, ref.kbl_module
    m = ref.KBL(device="cpu", verbose=0, **kw)
    rec = dict(pairs=[], stage1=[], log=[], within=[])

    def init_rec(**k):
        old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float32)
        try:
            net = kb.KBLBase(data_src=m.source_data, data_tar=m.target_data, device=m.device, k_cross=m.k_cross,
                             k_within=m.k_within, bridge_batch_size=1000, dim_hidden=64, num_layer=2,
                             num_epoch=num_epoch, lr=0.001, weight_decay=5e-3, source_clf=True, norm_mode='None',
                             norm_scale=1., **k)
        finally:
            torch.set_default_dtype(old)
        net.load_state_dict(on_grid(net.state_dict()) if init is None else
                            {k2: torch.as_tensor(v) for k2, v in init.items()})
        rec["init"] = {k2: v.detach().numpy().copy() for k2, v in net.state_dict().items()}
        net = net.to(dtype)
        torch.manual_seed(seeds[3])
        return net

    m.init_model = init_rec

    def sampling_rec(fn):
        def wrapped(self, *a, **k):
            i1, i2 = fn(self, *a, **k)
            n1 = int(round(np.sqrt(i1.numel())))
            assert n1 * n1 == i1.numel()
            l1, l2 = i1[:n1], i2[::n1]
            assert bool((i1 == l1.repeat(n1)).all()) and bool((i2 == l2.repeat_interleave(n1)).all())
            rec["pairs"].append((l1.numpy().copy(), l2.numpy().copy()))
            return i1, i2
        return wrapped

    def stage1_rec(fn):
        def wrapped(self, *a, **k):
            out = fn(self, *a, **k)
            rec["stage1"].append([float(v) for v in out])
            return out
        return wrapped

    def gen_rec(fn):
        def wrapped(self, *a, **k):
            rec["running"] = {k2: v.detach().double().numpy().copy() for k2, v in self.model.state_dict().items()
                              if "running_" in k2 or "num_batches" in k2}
            return fn(self, *a, **k)
        return wrapped

    def cross_rec(fn):
        def wrapped(self, k=3):
            out = fn(self, k=k)
            n_tar = self.data_tar.x.shape[0]
            more = fn(self, k=k + 1)[1].double()
            cos = torch.log(more) - torch.log1p(-more)
            rec["cross"] = (out[2].numpy().copy() // n_tar, out[2].numpy().copy() % n_tar,
                            out[1].double().numpy().copy(), float(cos[k - 1] - cos[k]))
            return out
        return wrapped

    def within_rec(fn):
        def wrapped(self, data_src, k=3, domain='source'):
            out = fn(self, data_src, k=k, domain=domain)
            rec["within"].append((out[0].numpy().copy(), out[1].double().numpy().copy(), out[2].numpy().copy()))
            return out
        return wrapped

    def log(**k):
        rec["log"].append((float(k["loss"]), float(k["source_train_acc"])))

    B, P = kb.BridgedGraph, kb.PairEnumerator
    old = (km.logger, P.sampling, B.train_adv_few_shot, B.gen_bridged_graph, B.add_topk_sim_cross_domain_edges_full,
           B.add_topk_sim_within_domain_edges_full, torch.get_default_dtype(), F.dropout)
    km.logger = log
    P.sampling, B.train_adv_few_shot, B.gen_bridged_graph = sampling_rec(old[1]), stage1_rec(old[2]), gen_rec(old[3])
    B.add_topk_sim_cross_domain_edges_full = cross_rec(old[4])
    B.add_topk_sim_within_domain_edges_full = within_rec(old[5])
    if not live_dropout:
        F.dropout = lambda x, p=0.5, training=True, inplace=False: old[7](x, 0.0, training, inplace)
    to_float = torch.Tensor.float
    if dtype == torch.float64:
        # the pair targets are (y_i == y_j).float(): in the float64 run .float() is the default dtype
        torch.Tensor.float = lambda self, *a, **k: self.to(torch.get_default_dtype())
        s = Data(x=s.x.double(), edge_index=s.edge_index, y=s.y, train_mask=s.train_mask, val_mask=s.val_mask,
                 test_mask=s.test_mask)
        t = Data(x=t.x.double(), edge_index=t.edge_index, y=t.y)
    try:
        torch.set_default_dtype(dtype)
        torch.manual_seed(seeds[0])
        random.seed(seeds[1])
        np.random.seed(seeds[2])
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            m.fit(s, t)
            logits, _ = m.predict(t)
    finally:
        (km.logger, P.sampling, B.train_adv_few_shot, B.gen_bridged_graph, B.add_topk_sim_cross_domain_edges_full,
         B.add_topk_sim_within_domain_edges_full) = old[:6]
        F.dropout = old[7]
        torch.Tensor.float = to_float
        torch.set_default_dtype(old[6])
    assert len(rec["stage1"]) == num_epoch and len(rec["pairs"]) == num_epoch
    return dict(init=rec["init"], running=rec["running"],
                ia=np.stack([a for a, _ in rec["pairs"]]), ib=np.stack([b for _, b in rec["pairs"]]),
                stage1=np.array(rec["stage1"], dtype=np.float64),
                cross_row=rec["cross"][0], cross_col=rec["cross"][1], cross_val=rec["cross"][2], gap=rec["cross"][3],
                within=rec["within"], merged_ei=m.stored_data.edge_index.numpy().copy(),
                losses=np.array([l for l, _ in rec["log"]], dtype=np.float64),
                accs=np.array([a for _, a in rec["log"]], dtype=np.float64),
                logits=logits.detach().double().numpy().copy())
