"""Host restatements of the layers that the device path runs on kernels: the four convolutions of ``GNNBase`` and its
bottleneck in torch (PyG's semantics, any dtype; ``GCNConv`` alone takes edge weights, and its parameters are cast to
the features' dtype), and the product that takes either kind of tensor."""
import torch
import torch.nn.functional as F

from .pagerank import host_gcn_graph


def _mm(a, b):
    """``a @ b``: the project's GEMM on device tensors, torch on host tensors."""
    if a.is_cuda:
        from .linear import tall_matmul
        return tall_matmul(a, b)
    return a @ b


def _scatter(src, index, n):
    return torch.zeros(n, src.size(1), dtype=src.dtype).index_add_(0, index, src)


def _host_conv(conv, x, edge_index, edge_weight=None):
    n = x.size(0)
    name = type(conv).__name__
    if name == "GCNConv":
        row, col, norm = host_gcn_graph(edge_index, n, x.dtype, edge_weight)
        return _scatter(norm[:, None] * F.linear(x, conv.lin.weight.to(x.dtype))[row], col, n) + conv.bias.to(x.dtype)
    if edge_weight is not None:
        raise NotImplementedError(f"{name} takes no edge weights")
    row, col = edge_index[0].long(), edge_index[1].long()
    if name == "SAGEConv":
        deg = torch.zeros(n, dtype=x.dtype).index_add_(0, col, torch.ones(col.numel(), dtype=x.dtype))
        mean = _scatter(x[row], col, n) / deg.clamp(min=1)[:, None]
        return F.linear(mean, conv.lin_l.weight, conv.lin_l.bias) + F.linear(x, conv.lin_r.weight)
    if name == "GINConv":
        return conv.nn(_scatter(x[row], col, n) + (1 + conv.eps) * x)
    keep = row != col                                        # GATConv: existing loops removed, one added per node
    loop = torch.arange(n)
    row, col = torch.cat([row[keep], loop]), torch.cat([col[keep], loop])
    h = F.linear(x, conv.lin.weight)
    a = F.leaky_relu((h * conv.att_src.view(1, -1)).sum(-1)[row] + (h * conv.att_dst.view(1, -1)).sum(-1)[col],
                     conv.negative_slope)
    amax = torch.full((n,), float("-inf"), dtype=x.dtype).scatter_reduce(0, col, a.detach(), reduce="amax")
    ex = (a - amax[col]).exp()
    alpha = ex / (torch.zeros(n, dtype=x.dtype).index_add_(0, col, ex) + 1e-16)[col]
    return _scatter(alpha[:, None] * h[row], col, n) + conv.bias


def _host_bottleneck(net, x, edge_index, edge_weight=None):
    last = len(net.convs) - 1
    for i, conv in enumerate(net.convs):
        x = _host_conv(conv, x, edge_index, edge_weight)
        if i < last:
            x = F.dropout(net.act(x), p=net.dropout, training=net.training)
    return x
