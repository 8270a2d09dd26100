"""GTrans fixture support: the driver that runs the reference's own ``pygda/models/gtrans.py`` on
``pygda/utils/perturb.py`` and ``pygda/nn/gnn_base.py`` (build container only, via ``make_golden_gtrans``).

TWO SHIMS beside ``_pyg_stub``:

* ``torch_sparse.coalesce(index, value, m, n, op)``: entries sorted by ``(row, col)``, duplicates reduced by ``op``
  ('add' / 'sum' or 'mean') in input order, differentiable in ``value`` (torch_sparse scatters the values with the
  requested reduction after sorting the keys).
* ``torch_geometric.utils.dropout_adj(edge_index, edge_attr, p)``: with ``p == 0`` its input, nothing drawn; else the
  mask ``torch.rand(E) >= p`` per directed edge (``force_undirected=False``), no rescaling, the filtered pair.  The
  draw is float32 whatever the default dtype, so that the float64 run of a fixture sees the masks of the float32 run.
  Every mask drawn is noted in ``MASKS``.

and a ``Data`` that answers ``edge_weight`` (None), which ``fit`` reads.

WHAT THE REFERENCE DOES WITH THE FLIP WEIGHTS.  ``fit`` hands ``optimizer_adj`` the tensor it creates and then works on
``perturbed_edge_weight.detach()`` and on what ``project`` returns: tensors the optimiser does not hold.
``update_edge_weights`` sets ``.grad`` on those, so ``optimizer_adj.step()`` finds no gradient and moves nothing: the
flip weights stay at 1e-7 for the whole fit, the raw weights wobble by 1e-7 under the repeated fold, and ``topk`` in
``sample_final_edges`` runs over ties.  The fixtures record exactly that, ties as torch's CPU ``topk`` breaks them.

What is recorded is observed from OUTSIDE the instance: ``test_time_loss`` is wrapped on the instance and ``inner`` /
``inner_margin`` / ``get_modified_adj`` in the module's namespace (return values and arguments are noted, nothing is
altered), ``np.random.permutation`` is wrapped for the duration of the fit, the module's ``logger`` is replaced by a
recorder, and ``init_model`` is wrapped so that the float32 and the float64 run start from one float32 state."""
import contextlib
import io
import random
import sys

import numpy as np
import torch

from . import _pyg_stub

MASKS = []


class Data(_pyg_stub.Data):
    edge_weight = None


def coalesce(index, value, m, n, op='add'):
    key = index[0] * n + index[1]
    uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
    out_index = torch.stack([uniq // n, uniq % n])
    if value is None:
        return out_index, None
    out = torch.zeros(uniq.numel(), dtype=value.dtype).index_add(0, inv, value)
    if op == 'mean':
        out = out / torch.zeros(uniq.numel(), dtype=value.dtype).index_add(0, inv, torch.ones_like(value))
    else:
        assert op in ('add', 'sum'), op
    return out_index, out


def dropout_adj(edge_index, edge_attr=None, p=0.5, force_undirected=False, num_nodes=None, training=True):
    assert not force_undirected and training
    if p == 0.0:
        return edge_index, edge_attr
    mask = torch.rand(edge_index.size(1), dtype=torch.float32) >= p
    MASKS.append(mask.numpy().copy())
    return edge_index[:, mask], (None if edge_attr is None else edge_attr[mask])


def load_gtrans(ref):
    from . import _ref_loader
    sys.modules["torch_sparse"].coalesce = coalesce
    sys.modules["torch_geometric.utils"].dropout_adj = dropout_adj
    sys.modules["torch_geometric.data"].Data = Data
    pert = _ref_loader._load("pygda.utils.perturb", "pygda/utils/perturb.py")
    gm = _ref_loader._load("pygda.models.gtrans", "pygda/models/gtrans.py")
    ref.GTrans, ref.gtrans_module, ref.perturb = gm.GTrans, gm, pert
    return ref


def gtrans_pair(seed, c):
    """``_soga_semantics.soga_pair``'s graphs (300 source / 260 target nodes; the target has a duplicate edge, a
    directed-only edge, an explicit self loop and an isolated node) as ``Data`` with ``edge_weight``."""
    from ._soga_semantics import soga_pair
    s, t = soga_pair(seed, c)
    return Data(x=s.x, edge_index=s.edge_index, y=s.y), Data(x=t.x, edge_index=t.edge_index, y=t.y)


def run_fit(ref, s, t, kw, epochs, seeds, dtype=torch.float32, init=None):
    """The reference's ``GTrans.fit`` and ``predict`` under the three ``seeds`` (torch, ``random``, ``np.random``).
    ``dtype`` float64 runs the same lines under ``torch.set_default_dtype(torch.float64)`` with float64 features;
    ``init`` (a float32 state dict) is loaded into the fresh network, so both precisions start alike."""
    gm = ref.gtrans_module
    m = ref.GTrans(device="cpu", epoch=epochs, verbose=0, **kw)
    rec, src_log, steps, perms, adj_calls = {}, [], [], [], []
    parts = []
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
    ttl = m.test_time_loss

    def ttl_rec(*a, **k):
        out = ttl(*a, **k)
        steps.append(float(out.detach()))
        return out

    m.test_time_loss = ttl_rec

    def noting(fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            parts.append(float(out.detach()))
            return out
        return wrapped

    def adj_rec(fn):
        def wrapped(mei, pw, *a, **k):
            ei, w = fn(mei, pw, *a, **k)
            adj_calls.append((pw.detach().numpy().copy(), ei.numpy().copy(), w.detach().double().numpy().copy()))
            return ei, w
        return wrapped

    def log(**k):
        src_log.append((float(k["loss"]), float(k["source_train_acc"])))

    draw = np.random.permutation

    def perm_rec(n):
        out = draw(n)
        perms.append(np.asarray(out).copy())
        return out

    old = (gm.logger, gm.inner, gm.inner_margin, gm.get_modified_adj, torch.get_default_dtype())
    gm.logger, gm.inner, gm.inner_margin = log, noting(gm.inner), noting(gm.inner_margin)
    gm.get_modified_adj = adj_rec(gm.get_modified_adj)
    np.random.permutation = perm_rec
    del MASKS[:]
    if dtype == torch.float64:
        s = Data(x=s.x.double(), edge_index=s.edge_index, y=s.y)
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
        gm.logger, gm.inner, gm.inner_margin, gm.get_modified_adj = old[:4]
        np.random.permutation = draw
        torch.set_default_dtype(old[4])
    return dict(init=rec["init"], masks=[k.copy() for k in MASKS], perms=perms, adj_calls=adj_calls,
                src_losses=np.array([l for l, _ in src_log], dtype=np.float64),
                accs=np.array([a for _, a in src_log], dtype=np.float64),
                steps=np.array(steps, dtype=np.float64), parts=np.array(parts, dtype=np.float64).reshape(-1, 2),
                new_feat=m.new_feat.detach().double().numpy().copy(), edge_index=m.edge_index.numpy().copy(),
                edge_weight=m.edge_weight.detach().double().numpy().copy(), logits=logits.detach().double().numpy().copy())


def crafted(ref):
    """``project`` and ``get_modified_adj`` of the reference on crafted inputs, float64 and float32: sums below and above
    the budget; pre-fold values below, above and exactly at 1."""
    P = ref.perturb
    out = {}
    g = torch.Generator().manual_seed(77)
    for name, m, scale, budget in (("below", 50, 0.05, 10), ("above", 50, 0.9, 10), ("one", 1, 0.9, 0),
                                   ("mid", 1000, 0.5, 100), ("mid_below", 1000, 0.05, 200), ("big", 40000, 0.3, 2000)):
        v = torch.rand(m, generator=g, dtype=torch.float64) * scale
        v[::7] = v[::7] + 0.6                                   # some entries beyond 1 after an Adam step
        v = v.float().double()                                  # float32 values: both precisions start alike
        out[f"project/{name}/in"] = v.float().numpy().copy()
        out[f"project/{name}/budget"] = np.int64(budget)
        out[f"project/{name}/out64"] = P.project(budget, v.clone(), 1e-7).numpy().copy()
        out[f"project/{name}/out32"] = P.project(budget, v.float(), 1e-7).numpy().copy()
    n = 7
    ei = torch.tensor([[0, 1, 1, 2, 2, 3, 3, 0, 4, 5], [1, 0, 2, 1, 2, 4, 4, 3, 5, 4]])   # a loop, a duplicate, one-way
    mei = torch.tensor([[0, 1, 3, 3, 0, 4], [1, 2, 4, 4, 3, 5]])
    pw = torch.tensor([0.25, 0.5, 0.125, 0.375, 0.75, 0.0], dtype=torch.float64)
    w = torch.tensor([1.0, 0.5, 0.5, 1.0, 0.7, 1.0, 1.0, 0.25, 1.0, 0.9], dtype=torch.float64)
    for und in (False, True):
        e1, w1 = P.get_modified_adj(mei, pw, n, "cpu", ei, w, und)
        e2, w2 = P.get_modified_adj(mei, pw, n, "cpu", e1, w1, und)
        tag = f"adj/{'und' if und else 'dir'}"
        out.update({f"{tag}/e1": e1.numpy().copy(), f"{tag}/w1": w1.numpy().copy(), f"{tag}/e2": e2.numpy().copy(),
                    f"{tag}/w2": w2.numpy().copy()})
    out.update({"adj/n": np.int64(n), "adj/ei": ei.numpy(), "adj/mei": mei.numpy(), "adj/p": pw.numpy(), "adj/w": w.numpy()})
    return out
