"""``ASNBase`` (pygda/nn/asn_base.py): eight ``GNNVAE`` encoders' worth of modules -- private local / global per domain,
shared local / global -- the two inner-product decoders, the classifier, the domain discriminator behind a gradient
reversal and three view attentions.  Same module names, state dict keys and init RNG stream as the reference: every
``GCNConv`` and ``nn.Linear`` draws its init when built, in the reference's construction order.

What the port keeps on purpose:
- ``GNNVAE.dropout_layers`` is a plain Python list, so ``model.eval()`` never reaches those ``Dropout(0.1)``: the hidden
  dropout is always on, in ``predict`` too;
- ``reparameterize`` uses ``exp(logvar)``, not ``exp(0.5 logvar)``.

``forward`` of the modules here is the reference's host computation (``GCNConv`` restated from PyG's ``gcn_norm``: the
``edge_index`` branch with ``add_remaining_self_loops``, and a dense normalised matrix for the global encoders); the
trainer's device path (pygda_amd/models/asn.py) runs the same parameters on the HIP kernels."""
import torch
import torch.nn.functional as F
from torch import nn

from ..ops import asn_diff_loss, asn_kld, asn_recon_loss, asn_reparam
from .attention import Attention
from .gcn_conv import GCNConv
from .linear import DenseLinear


def host_gcn(conv, x, adj):
    """PyG ``GCNConv(x, adj)`` on the host: ``adj`` an ``edge_index`` ([2, E], source row 0; gcn_norm with
    add_remaining_self_loops, destination degrees) or the dense normalised matrix of a sparse adjacency
    (ops.asn_gcn_norm_sparse)."""
    h = F.linear(x, conv.lin.weight)
    if adj.is_floating_point():
        return adj @ h + conv.bias
    n = x.size(0)
    row, col = adj[0], adj[1]
    keep = row != col
    loop = torch.arange(n, device=x.device)
    row, col = torch.cat([row[keep], loop]), torch.cat([col[keep], loop])
    w = torch.ones(row.numel(), dtype=x.dtype, device=x.device)
    deg = torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(0, col, w)
    dis = deg.pow(-0.5)
    dis.masked_fill_(dis == float("inf"), 0)
    norm = dis[row] * w * dis[col]
    out = torch.zeros(n, h.size(1), dtype=x.dtype, device=x.device).index_add_(0, col, norm[:, None] * h[row])
    return out + conv.bias


class InnerProductDecoder(nn.Module):
    def __init__(self, dropout, act=torch.sigmoid):
        super().__init__()
        self.dropout = dropout
        self.act = act

    def forward(self, z):
        z = F.dropout(z, self.dropout, training=self.training)
        return self.act(torch.mm(z, z.t()))


class DiffLoss(nn.Module):
    def forward(self, input1, input2):
        return asn_diff_loss(input1, input2)


class GNNVAE(nn.Module):
    def __init__(self, in_dim, hid_dim, num_classes, gnn_type='gcn', num_layers=3, base_model=None, act=F.relu,
                 **kwargs):
        super().__init__()
        if num_layers != 3:
            raise ValueError("GNNVAE: num_layers must be 3 (the reference asserts it)")
        self.dropout_layers = [nn.Dropout(0.1) for _ in range(num_layers)]     # a list: eval() never reaches them
        self.gnn_type, self.act, self.num_layers = gnn_type, act, num_layers
        self.conv_layers = nn.ModuleList()
        self.conv_layers.append(GCNConv(in_dim, hid_dim))
        self.conv_layers.append(GCNConv(hid_dim, num_classes))
        self.conv_layers.append(GCNConv(hid_dim, num_classes))

    def forward(self, x, edge_index, eps=None):
        """``(z, mu, logvar)`` as the reference computes them; ``eps`` replaces the ``randn_like`` draw.  Host tensors
        take an ``edge_index`` or the dense normalised matrix of ``ASN.process_graph``; device tensors an
        ``edge_index`` or its :class:`CSRGraph` (the convs' SpMM, the fused ReLU + dropout, the Philox noise)."""
        if x.is_cuda:
            from ..ops import relu_dropout
            h = self.conv_layers[0](x, edge_index)
            p = self.dropout_layers[0].p
            x = relu_dropout(h, p, True) if self.act is F.relu else F.dropout(self.act(h), p)
            mu, logvar = self.conv_layers[-2](x, edge_index), self.conv_layers[-1](x, edge_index)
            return (asn_reparam(mu, logvar, eps) if self.training else mu), mu, logvar
        x = self.dropout_layers[0](self.act(host_gcn(self.conv_layers[0], x, edge_index)))
        mu = host_gcn(self.conv_layers[-2], x, edge_index)
        logvar = host_gcn(self.conv_layers[-1], x, edge_index)
        z = asn_reparam(mu, logvar, eps) if self.training else mu
        return z, mu, logvar


class ASNBase(nn.Module):
    def __init__(self, in_dim, hid_dim, hid_dim_vae, num_classes, num_layers=3, act=F.relu, dropout=0.1, adv_dim=40,
                 **kwargs):
        super().__init__()
        enc = dict(in_dim=in_dim, hid_dim=hid_dim, num_classes=hid_dim_vae, act=act, num_layers=num_layers)
        self.private_encoder_s_l = GNNVAE(**enc)
        self.private_encoder_t_l = GNNVAE(**enc)
        self.private_encoder_s_g = GNNVAE(**enc)
        self.private_encoder_t_g = GNNVAE(**enc)
        self.decoder_s = InnerProductDecoder(dropout=dropout, act=lambda x: x)
        self.decoder_t = InnerProductDecoder(dropout=dropout, act=lambda x: x)
        self.shared_encoder_l = GNNVAE(**enc)
        self.shared_encoder_g = GNNVAE(**enc)
        self.cls_model = nn.Sequential(DenseLinear(hid_dim_vae, num_classes))
        self.domain_model = nn.Sequential(DenseLinear(hid_dim_vae, adv_dim), nn.ReLU(), nn.Dropout(0.1),
                                          DenseLinear(adv_dim, 2))
        self.att_model = Attention(hid_dim_vae)
        self.att_model_self_s = Attention(hid_dim_vae)
        self.att_model_self_t = Attention(hid_dim_vae)
        self.models = [self.private_encoder_s_l, self.private_encoder_s_g, self.private_encoder_t_l,
                       self.private_encoder_t_g, self.shared_encoder_g, self.shared_encoder_l, self.cls_model,
                       self.domain_model, self.decoder_s, self.decoder_t, self.att_model, self.att_model_self_s,
                       self.att_model_self_t]
        self.cls_loss = nn.CrossEntropyLoss()
        self.loss_diff = DiffLoss()

    def recon_loss(self, preds, labels, mu, logvar, n_nodes, norm, pos_weight):
        """The reference's entry point: ``preds`` the decoder's dense N x N logits, ``labels`` the dense ``A + I``.
        Kept for scripts written against the reference; the trainer uses :meth:`recon_loss_fused`."""
        cost = norm * F.binary_cross_entropy_with_logits(preds, labels, pos_weight=pos_weight)
        return cost + asn_kld(mu, logvar, n_nodes)

    def recon_loss_fused(self, z, labels, mu, logvar, n_nodes):
        """``recon_loss(decoder(z), ...)`` with the decoder input ``z`` (after its dropout) and the domain's
        :class:`~pygda_amd.ops.AsnLabels`: on the device the N x N logits are never formed (ops.asn_recon_loss)."""
        return asn_recon_loss(z, labels) + asn_kld(mu, logvar, n_nodes)

    def adj_label_for_reconstruction(self, data):
        """The reference's ``(adj_label, pos_weight, norm)``: dense ``to_dense_adj(edge_index) + I`` and the two
        scalars as fp32 tensors."""
        from ..ops import AsnLabels
        lab = AsnLabels(data.edge_index, int(data.edge_index.max()) + 1)
        dev = data.x.device
        return (lab.dense().to(dev), torch.tensor([[lab.pos_weight]], device=dev),
                torch.tensor(lab.norm, device=dev))
