"""``SOGABase`` (pygda/nn/soga_base.py): ``num_layers`` gcn / sage / gat / gin layers with the activation and dropout
between them only (the last conv has neither) and a dense ``cls`` head; returns the raw logits.  The parameter names
are the reference's (``convs.<i>...``, ``cls.weight``, ``cls.bias``).  ``cce`` is its label-smoothed cross-entropy;
the sample tables of ``init_target`` are built by :func:`pygda_amd.utils.sampler.soga_samples`."""
import torch
import torch.nn.functional as F
from torch import nn

from .gnn_base import _make
from .linear import DenseLinear


class CustomizedCrossEntropy(nn.Module):
    """``mean_i -(t_i * log_softmax(outputs_i)).sum()``, ``t = (1 - epsilon) onehot + epsilon / num_classes``."""

    def __init__(self, num_classes, device=None, epsilon=0.1, reduction=True):
        super().__init__()
        self.num_classes, self.epsilon, self.reduction, self.device = num_classes, epsilon, reduction, device

    def forward(self, outputs, targets):
        if self.reduction:
            from ..ops import soga_smooth_ce
            return soga_smooth_ce(outputs, targets, self.epsilon)
        t = torch.zeros_like(outputs).scatter_(1, targets.long().unsqueeze(1), 1.0)
        t = (1 - self.epsilon) * t + self.epsilon / self.num_classes
        return (-t * torch.log_softmax(outputs, dim=1)).sum(dim=1)


class SOGABase(nn.Module):
    def __init__(self, in_dim, hid_dim, num_classes, num_layers=1, dropout=0.1, act=F.relu, gnn='gcn',
                 num_negative_samples=5, num_positive_samples=2, device='cuda:0', **kwargs):
        super().__init__()
        assert gnn in ('gcn', 'sage', 'gat', 'gin'), 'Invalid gnn backbone'
        self.in_dim, self.hid_dim, self.num_classes = in_dim, hid_dim, num_classes
        self.num_layers, self.dropout, self.gnn, self.act = num_layers, dropout, gnn, act
        self.num_negative_samples, self.num_positive_samples, self.device = num_negative_samples, num_positive_samples, device
        self.cce = CustomizedCrossEntropy(num_classes, device)
        dims = [in_dim] + [hid_dim] * num_layers
        self.convs = nn.ModuleList(_make(gnn, dims[i], dims[i + 1]) for i in range(num_layers))
        self.cls = DenseLinear(hid_dim, num_classes)

    def forward(self, x, edge_index, edge_weight=None):
        return self.feat_classifier(self.feat_bottleneck(x, edge_index, edge_weight))

    def feat_bottleneck(self, x, edge_index, edge_weight=None):
        last = len(self.convs) - 1
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index, edge_weight)
            if i < last:
                x = F.dropout(self.act(x), p=self.dropout, training=self.training)
        return x

    def feat_classifier(self, x):
        return self.cls(x)

    def init_target(self, graph_struct, graph_neigh=None):
        """The two views' ``center`` / ``positive`` / ``negative`` tables as int64 tensors on the module's attributes,
        named as in the reference.  Both views are sampled on ``graph_struct``'s edges, as the reference's are when it
        is handed a graph and its clone."""
        from ..utils.sampler import soga_samples
        views = soga_samples(graph_struct.edge_index, graph_struct.x.size(0), self.num_negative_samples)
        for name, (cen, pos, neg) in zip(("struct", "neigh"), views):
            setattr(self, "center_nodes_" + name, torch.from_numpy(cen))
            setattr(self, "positive_samples_" + name, torch.from_numpy(pos))
            setattr(self, "negative_samples_" + name, torch.from_numpy(neg))
        return views
