"""PyG ``FAConv`` as SAGDA's ``SAGNN`` layer uses it (pygda/nn/sagda_base.py:50,87): the published semantics of
torch_geometric >= 2.4 the build assumes, numbered in the style of tests/golden/_pyg_conv_semantics.py so a reviewer
can check each against PyG's source.  PyG cannot run here (not vendored, not installable), so
``make_golden_sagda.py`` runs the reference on the stand-in :class:`FAConv` below, and :func:`faconv_loop` restates
the same operator independently -- per-node Python loops in float64 over incoming-edge lists, no tensor gather or
scatter, no code shared with the stand-in -- so that the committed ``faconv.npz`` is pinned by two readings of the
assumptions.  "Parity unpinned at the PyG boundary" still holds for this operator.

 F1  ``FAConv(channels, eps=0.1, dropout=0.0, cached=False, add_self_loops=True, normalize=True)``: the defaults
     ``SAGNN`` keeps.  Dropout on the attention coefficients is 0.
 F2  ``att_l`` and ``att_r`` are ``Linear(channels, 1, bias=False)`` with PyG's default initialiser
     (``kaiming_uniform(fan=in, a=sqrt(5))`` = U(-1/sqrt(in), 1/sqrt(in)), _pyg_stub.py 13a), weight ``[1, channels]``.
 F3  ``FAConv.__init__`` builds both Linears (each draws in its own ``__init__``) and then calls
     ``reset_parameters()``, which resets att_l and att_r again: the init RNG stream is consumed
     att_l, att_r, att_l, att_r.  No other parameter, no buffer.
 F4  ``normalize=True``: ``gcn_norm(edge_index, None, N, improved=False, add_self_loops=True)`` on EVERY call
     (``cached=False``): ``add_remaining_self_loops`` with fill 1 (existing self loops dropped, one loop per node
     appended LAST in node order, _pyg_stub.py 2), degree summed over the DESTINATION (``col``, flow
     source_to_target), ``w_ij = deg_j^-1/2 deg_i^-1/2`` (0 where a degree is 0).
 F5  ``forward(x, x_0, edge_index)``: ``alpha_l = att_l(x)``, ``alpha_r = att_r(x)``; per edge j -> i the message is
     ``x_j * (tanh(alpha_l[j] + alpha_r[i]) * w_ij)`` -- the coefficient is the product ``tanh * w``, rounded once,
     then multiplied into ``x_j``; messages are summed per destination in edge order (aggr='add').
 F6  Then ``out = out + eps * x_0`` (eps != 0).  ``SAGNN`` passes ``x_0 = x``.
 F7  Multiset semantics: a duplicate edge is its own message; an isolated node receives only its self loop.
"""
import math

import torch
import torch.nn.functional as F


def _incoming(edge_index, n):
    inc = [[] for _ in range(n)]
    for j, i in zip(edge_index[0].tolist(), edge_index[1].tolist()):
        if j != i:                                                   # F4: existing loops dropped
            inc[i].append(j)
    for i in range(n):
        inc[i].append(i)                                             # F4: one loop per node, last
    return inc


def faconv_loop(x, edge_index, att_l, att_r, eps=0.1):
    """F4-F7 in float64, one node at a time; differentiable in ``x``, ``att_l`` and ``att_r`` (float64 leaves)."""
    n = x.size(0)
    inc = _incoming(edge_index, n)
    deg = [0.0] * n
    for i, nb in enumerate(inc):
        deg[i] = float(len(nb))                                      # every entry weighs 1 before normalisation
    dis = [1.0 / math.sqrt(v) if v > 0 else 0.0 for v in deg]
    al = [torch.dot(att_l.view(-1), x[j]) for j in range(n)]
    ar = [torch.dot(att_r.view(-1), x[i]) for i in range(n)]
    rows = []
    for i, nb in enumerate(inc):
        acc = torch.zeros(x.size(1), dtype=torch.float64)
        for j in nb:
            w = dis[j] * dis[i]
            acc = acc + x[j] * (torch.tanh(al[j] + ar[i]) * w)
        rows.append(acc + eps * x[i])
    return torch.stack(rows)


class FAConv(torch.nn.Module):
    """Stand-in for ``torch_geometric.nn.FAConv`` (F1-F7) installed by make_golden_sagda.py; vectorised, on the
    stub's ``Linear`` and ``gcn_norm``.  The stub's ``propagate`` does not lift ``alpha_i`` / ``alpha_j``, so the
    gathers are written out here."""

    def __init__(self, channels, eps=0.1, dropout=0.0, cached=False, add_self_loops=True, normalize=True, **kwargs):
        super().__init__()
        from . import _pyg_stub
        assert dropout == 0.0 and not cached and add_self_loops and normalize
        self.channels, self.eps, self.dropout = channels, eps, dropout
        self.att_l = _pyg_stub.Linear(channels, 1, bias=False)
        self.att_r = _pyg_stub.Linear(channels, 1, bias=False)
        self.reset_parameters()

    def reset_parameters(self):
        self.att_l.reset_parameters()
        self.att_r.reset_parameters()

    def forward(self, x, x_0, edge_index, edge_weight=None):
        from . import _pyg_stub
        assert edge_weight is None
        ei, w = _pyg_stub._gcn_norm(edge_index, None, x.size(0), False, True)
        alpha_l, alpha_r = self.att_l(x), self.att_r(x)
        j, i = ei[0], ei[1]
        alpha = (alpha_l.index_select(0, j) + alpha_r.index_select(0, i)).tanh().squeeze(-1)
        alpha = F.dropout(alpha, p=self.dropout, training=self.training)
        msg = x.index_select(0, j) * (alpha * w).view(-1, 1)
        out = torch.zeros_like(x).index_add_(0, i, msg)
        if self.eps != 0.0:
            out = out + self.eps * x_0
        return out
