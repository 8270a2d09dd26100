"""``PageRank`` of pygda/models/sepa.py: ``k`` steps of ``x <- (1 - alpha) A x + alpha x_0`` with ``A`` the
gcn-normalised graph (self loops added, destination degrees), i.e. the graph a ``GCNConv`` on the same ``edge_index``
already holds.  Device tensors: the cached :class:`~pygda_amd.graph.CSRGraph` and ``ops.ppr`` (one SpMM launch per
step, the restart in its epilogue, the transposed CSR going backwards).  Host tensors: the same steps in torch."""
import torch
from torch import nn


def host_gcn_graph(edge_index, n, dtype, edge_weight=None):
    """``gcn_norm`` on the host: existing self loops keep their weight, every other node gets a unit loop, weights
    ``deg^-1/2[row] w deg^-1/2[col]`` with destination (``col``) degrees.  Returns ``(row, col, norm)``."""
    row, col = edge_index[0].long(), edge_index[1].long()
    w = torch.ones(row.numel(), dtype=dtype) if edge_weight is None else edge_weight.to(dtype)
    keep = row != col
    loop_w = torch.ones(n, dtype=dtype)
    loop_w[row[~keep]] = w[~keep]
    loop = torch.arange(n)
    row, col, w = torch.cat([row[keep], loop]), torch.cat([col[keep], loop]), torch.cat([w[keep], loop_w])
    deg = torch.zeros(n, dtype=dtype).index_add_(0, col, w)
    dis = deg.pow(-0.5)
    dis = dis.masked_fill(dis == float("inf"), 0)
    return row, col, dis[row] * w * dis[col]


class PageRank(nn.Module):
    def __init__(self, k=5, alpha=0.9, **kwargs):
        super().__init__()
        self.k, self.alpha = k, alpha

    def forward(self, x, edge_index, edge_weight=None):
        if x.is_cuda:
            from ..graph import as_graph
            from ..ops import ppr
            return ppr(x, as_graph(edge_index, x.size(0), edge_weight, False, True, True, "col"), self.k, self.alpha)
        row, col, norm = host_gcn_graph(edge_index, x.size(0), x.dtype, edge_weight)
        hidden = x
        for _ in range(self.k):
            x = torch.zeros_like(hidden).index_add_(0, col, norm[:, None] * x[row])
            x = (1 - self.alpha) * x + self.alpha * hidden
        return x
