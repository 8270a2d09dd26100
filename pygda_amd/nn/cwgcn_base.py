"""``CWGCNBase`` (pygda/nn/cwgcn_base.py:11-219): two convs of the chosen backbone (gcn | sage | gat | gin, built as
``GNNBase`` builds them) and a classifier -- a conv of the same type in node mode, a linear layer in graph mode.
``forward`` returns the RAW logits and ``x_list``: ``dropout(act(conv0))`` and conv1's output (each mean-pooled per
graph in graph mode, :130-165).  ``c_loss`` is the correntropy-induced loss with its per-row sample weights on
csrc/gda_cwgcn.hip."""
import torch
import torch.nn.functional as F
from torch import nn

from ..ops import correntropy_loss
from .a2gnn_base import global_mean_pool
from .gnn_base import _make
from .linear import DenseLinear


class CWGCNBase(nn.Module):
    def __init__(self, in_dim, hid_dim, num_classes, num_layers=2, dropout=0.1, act=F.relu, gnn='gcn', mode='node',
                 **kwargs):
        super().__init__()
        assert gnn in ('gcn', 'sage', 'gat', 'gin'), 'Invalid gnn backbone'           # :53-54
        assert num_layers == 2, 'unsupport number of layers'
        self.in_dim, self.hid_dim, self.num_classes = in_dim, hid_dim, num_classes
        self.num_layers, self.dropout, self.gnn, self.act, self.mode = num_layers, dropout, gnn, act, mode
        # construction order = the reference's init RNG stream: conv0, conv1, then the classifier (:66-99)
        self.convs = nn.ModuleList([_make(gnn, in_dim, hid_dim), _make(gnn, hid_dim, hid_dim)])
        self.cls = _make(gnn, hid_dim, num_classes) if mode == 'node' else DenseLinear(hid_dim, num_classes)

    def forward(self, x, edge_index, edge_weight=None, batch=None):
        x, x_list = self.feat_bottleneck(x, edge_index, edge_weight, batch)
        return self.feat_classifier(x, edge_index, edge_weight), x_list

    def feat_bottleneck(self, x, edge_index, edge_weight=None, batch=None):
        x_list = []
        fused = self.act is F.relu and x.is_cuda and x.dtype == torch.float32
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index, edge_weight)
            if i < len(self.convs) - 1:
                if fused:                # activation + dropout as one kernel each way (no mask tensor)
                    from ..ops import relu_dropout
                    x = relu_dropout(x, self.dropout, self.training)
                else:
                    x = F.dropout(self.act(x), p=self.dropout, training=self.training)
            x_list.append(x if self.mode == 'node' else global_mean_pool(x, batch))
        if self.mode == 'graph':
            x = global_mean_pool(x, batch)
        return x, x_list

    def feat_classifier(self, x, edge_index, edge_weight=None):
        return self.cls(x) if self.mode == 'graph' else self.cls(x, edge_index, edge_weight)

    def c_loss(self, preds, labels):
        """(:193-219) ``d_i = sum_c (preds_ic - onehot(labels)_ic)^2``; ``(mean(1 - exp(-d / 100)), exp(-d / 10))``.  The
        weights are kept on ``self.weight`` as the reference keeps them."""
        loss, self.weight = correntropy_loss(preds, labels)
        return loss, self.weight
