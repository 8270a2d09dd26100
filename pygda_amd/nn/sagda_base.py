"""``SAGDABase`` (pygda/nn/sagda_base.py:257-330): UDAGCN's dual-view target encoder (``TgtGNN`` = UDAGCN's ``GNN``,
the GCN and PPMI stacks on shared weights, view attention) beside a source encoder of ``SAGNN`` layers that share the
same weights and biases; linear classifier; MLP domain discriminator.

``SAGNN`` (:14-90) is PyG ``FAConv(in_features)`` called as ``conv(x, x, edge_index)``, then ``torch.mm(., W) + b``.
FAConv is linear in x and both attention logits are rank-1 projections of x (tests/golden/_faconv_semantics.py), so
the layer runs reassociated: ONE projection ``[h | s | r] = x [W | att_l^T | att_r^T]`` -- over the sparse bag-of-words
features at layer 0 (sparse_features), on the hand-written GEMMs above it -- then the fused aggregation
``out = A_att h + eps h + b`` (csrc/gda_faconv.hip) gathers ``hid``-wide rows instead of input-wide ones.  The
gradients ``d[W | att_l^T | att_r^T] = x^T [gh | gs | gr]`` and ``dx = [gh | gs | gr] [W | att_l^T | att_r^T]^T`` are
that projection's own backward.

``SrcGNN.forward`` (:147-170) chains the layers with no activation and no dropout; its ``dropout_layers``, ``act``,
``alpha`` and ``beta`` are stored and never used, as in the reference."""
import weakref

import torch
import torch.nn.functional as F
from torch import nn

from .. import sparse_features
from ..graph import build_csr
from ..ops import faconv_aggregate_packed
from .attention import Attention
from .linear import DenseLinear, Linear, glorot, tall_matmul, tall_matmul_ok, zeros
from .udagcn_base import GNN as TgtGNN

_graphs = {}      # FAConv graphs (gcn_norm: remaining self loops, destination degree; edge map), keyed by identity


def faconv_graph(edge_index, num_nodes):
    """The graph FAConv normalises on every call (gcn_norm with ``add_remaining_self_loops`` fill 1 and the degree over
    the destination), built once per edge tensor with the by-source edge map the backward walks."""
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), int(num_nodes))
    hit = _graphs.get(key)
    if hit is not None and hit[0]() is edge_index:
        return hit[1]
    g = build_csr(edge_index, num_nodes, None, False, True, True, "col", with_edge_map=True)
    _graphs[key] = (weakref.ref(edge_index), g)
    if len(_graphs) > 32:
        for k in [k for k, v in _graphs.items() if v[0]() is None]:
            del _graphs[k]
    return g


class FAConvAttention(nn.Module):
    """The parameters of PyG ``FAConv(channels)`` -- ``att_l`` and ``att_r``, ``Linear(channels, 1, bias=False)`` with
    PyG's default initialiser -- under FAConv's names, so state dicts load by name.  ``FAConv.__init__`` ends in
    ``reset_parameters()``, so each vector is drawn twice: att_l, att_r, att_l, att_r.  Not a standalone FAConv: the
    aggregation runs inside :class:`SAGNN`, reassociated with the layer's weight."""

    def __init__(self, channels, eps=0.1):
        super().__init__()
        self.channels, self.eps = channels, eps
        self.att_l = Linear(channels, 1, bias=False, weight_initializer=None)
        self.att_r = Linear(channels, 1, bias=False, weight_initializer=None)
        self.reset_parameters()

    def reset_parameters(self):
        self.att_l.reset_parameters()
        self.att_r.reset_parameters()

    def __repr__(self):
        return f"FAConv({self.channels}, eps={self.eps})"


class SAGNN(nn.Module):
    def __init__(self, in_features, out_features, alpha, beta, weight=None, bias=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.alpha, self.beta = alpha, beta
        self.conv = FAConvAttention(in_features)                       # :50, drawn before the weight
        if weight is None:
            self.weight = nn.Parameter(torch.empty(in_features, out_features, dtype=torch.float32))
            glorot(self.weight)
        else:
            self.weight = weight          # shared with the target encoder's conv layer
        if bias is None:
            self.bias = nn.Parameter(torch.empty(out_features, dtype=torch.float32))
            zeros(self.bias)
        else:
            self.bias = bias

    def forward(self, x, edge_index):
        if not x.is_cuda:
            raise RuntimeError("SAGNN runs on the GPU kernels (csrc/gda_faconv.hip); move the data to the device")
        # [W | att_l^T | att_r^T]  [in, out + 2]
        wc = torch.cat([self.weight, self.conv.att_l.weight.t(), self.conv.att_r.weight.t()], dim=1)
        sf = sparse_features.lookup(x) if x.dim() == 2 and x.size(1) >= sparse_features.MIN_WIDTH else None
        if sf is not None:
            p = sparse_features.sparse_matmul(sf, wc)
        elif tall_matmul_ok(x, wc):
            p = tall_matmul(x, wc)
        else:
            raise RuntimeError(f"SAGNN: no kernel for a {x.dtype} input of shape {tuple(x.shape)}")
        return faconv_aggregate_packed(p, self.out_features, faconv_graph(edge_index, x.size(0)), self.conv.eps,
                                       self.bias)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_features}, {self.out_features})"


class SrcGNN(nn.Module):
    def __init__(self, in_dim, hid_dim, alpha=0.5, beta=0.5, num_layers=3, act=F.relu, base_model=None):
        super().__init__()
        self.dropout_layers = [nn.Dropout(0.1) for _ in range(num_layers)]      # stored, never applied (:147-170)
        self.act, self.alpha, self.beta = act, alpha, beta
        shared = None if base_model is None else list(base_model.conv_layers)
        dims = [in_dim] + [hid_dim] * num_layers
        self.conv_layers = nn.ModuleList(
            SAGNN(dims[i], dims[i + 1], alpha=alpha, beta=beta, weight=None if shared is None else shared[i].weight,
                  bias=None if shared is None else shared[i].bias) for i in range(num_layers))

    def forward(self, x, edge_index):
        for conv in self.conv_layers:
            x = conv(x, edge_index)
        return x


class SAGDABase(nn.Module):
    def __init__(self, in_dim, hid_dim, num_classes, num_layers=3, dropout=0.1, act=F.relu, beta=0.5, alpha=0.5,
                 ppmi=True, adv_dim=40, **kwargs):
        super().__init__()
        if not ppmi:
            # the reference lists self.ppmi_encoder in self.models unconditionally (sagda_base.py:322): without the
            # PPMI view its constructor fails with AttributeError
            raise ValueError("SAGDABase needs ppmi=True: the reference builds no model without the PPMI view "
                             "(pygda/nn/sagda_base.py:322 lists ppmi_encoder unconditionally)")
        self.ppmi = ppmi
        self.encoder = TgtGNN(in_dim=in_dim, hid_dim=hid_dim, gnn_type='gcn', act=act, num_layers=num_layers)
        self.ppmi_encoder = TgtGNN(in_dim=in_dim, hid_dim=hid_dim, gnn_type='ppmi', base_model=self.encoder,
                                   path_len=10, num_layers=num_layers)
        self.src_encoder = SrcGNN(in_dim=in_dim, hid_dim=hid_dim, num_layers=num_layers, alpha=alpha, beta=beta,
                                  base_model=self.encoder)
        self.cls_model = nn.Sequential(DenseLinear(hid_dim, num_classes))
        self.domain_model = nn.Sequential(DenseLinear(hid_dim, adv_dim), nn.ReLU(), nn.Dropout(0.1),
                                          DenseLinear(adv_dim, 2))
        self.att_model = Attention(hid_dim)
        self.models = [self.encoder, self.cls_model, self.domain_model, self.ppmi_encoder, self.att_model,
                       self.src_encoder]
        self.loss_func = nn.CrossEntropyLoss()

    def src_encode(self, x, edge_index, mask=None):
        out = self.src_encoder(x, edge_index)
        return out if mask is None else out[mask]

    def gcn_encode(self, data, cache_name, mask=None):
        out = self.encoder(data.x, data.edge_index, cache_name)
        return out if mask is None else out[mask]

    def ppmi_encode(self, data, cache_name, mask=None):
        out = self.ppmi_encoder(data.x, data.edge_index, cache_name)
        return out if mask is None else out[mask]

    def encode(self, data, cache_name, mask=None):
        return self.att_model([self.gcn_encode(data, cache_name, mask), self.ppmi_encode(data, cache_name, mask)])
