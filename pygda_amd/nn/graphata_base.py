"""``GraphATABase`` (pygda/nn/graphata_base.py): a stack of :class:`NodeCentricConv` layers over the source models'
layer weights (activation and dropout between them) and a :class:`NodeCentricMLP` head over their classifiers; returns
``log_softmax``.  The parameters are the layers' ``att`` / ``weight`` and the head's ``att`` (``convs.<i>.att``,
``convs.<i>.weight``, ``cls.att``): the source models are held in plain lists, as in the reference.  On the device the
activation and the dropout between the layers are ``ops.relu_dropout`` (the project's keep-bit stream), which covers
``act=F.relu`` only."""
import torch.nn.functional as F
from torch import nn

from .a2gnn_base import global_mean_pool
from .node_centric_conv import NodeCentricConv, NodeCentricMLP


class GraphATABase(nn.Module):
    def __init__(self, in_dim, hid_dim, num_classes, model_weights, model_list, num_layers=1, dropout=0.1, act=F.relu,
                 gnn='gcn', mode='node', **kwargs):
        super().__init__()
        self.in_dim, self.hid_dim, self.num_classes = in_dim, hid_dim, num_classes
        self.num_layers, self.dropout, self.act, self.mode = num_layers, dropout, act, mode
        self.convs = nn.ModuleList()
        self.convs.append(NodeCentricConv(self.in_dim, self.hid_dim, model_weights[0]))
        for i in range(self.num_layers - 1):
            self.convs.append(NodeCentricConv(self.hid_dim, self.hid_dim, model_weights[i + 1]))
        self.cls = NodeCentricMLP(self.num_classes, model_list)

    def forward(self, x, edge_index, edge_weight=None, batch=None):
        x = self.feat_bottleneck(x, edge_index, edge_weight, batch)
        x = self.feat_classifier(x, edge_index, edge_weight)
        return F.log_softmax(x, dim=1)

    def feat_bottleneck(self, x, edge_index, edge_weight=None, batch=None):
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index, edge_weight)
            if i < len(self.convs) - 1:
                if x.is_cuda:
                    if self.act is not F.relu:
                        raise NotImplementedError("GraphATABase: act other than F.relu is not supported on the device")
                    from ..ops import relu_dropout
                    x = relu_dropout(x, self.dropout, self.training)
                else:
                    x = F.dropout(self.act(x), p=self.dropout, training=self.training)
        if self.mode == 'graph':
            x = global_mean_pool(x, batch)
        return x

    def feat_classifier(self, x, edge_index, edge_weight=None, batch=None):
        return self.cls(x, edge_index, edge_weight)
