"""``DGDABase`` (pygda/nn/dgda_base.py): the VGAE encoder with three latent spaces (domain ``d``, semantic ``y``,
random ``m``), the graph decoder, the class classifier and the one-logit domain classifier behind a gradient reversal.
Same module names, state dict keys and init RNG stream as the reference: the four frozen ``nn.Embedding`` tables draw
their (overwritten) init when built, every ``BatchGraphConvolution`` fills its bias before its Xavier weight.

Only ``backbone='gcn'`` is supported.  ``GraphDiscriminator`` and ``NoiseDecoder`` exist for the state dict; as in the
reference no loss term reaches them, so they never receive a gradient.

``forward`` here is the reference's host computation on a dense adjacency, which -- as in the reference -- is MUTATED IN
PLACE (``adj += I`` in ``vectorized_sym_norm``); the trainer's device path (pygda_amd/models/dgda.py) runs the same
parameters on the HIP kernels."""
import torch
import torch.nn.init as init
from torch import nn
from torch.nn.parameter import Parameter

from .linear import DenseLinear
from .reverse_layer import GradReverse


class BatchGraphConvolution(nn.Module):
    """``adj @ (x @ weight) + bias`` with ``weight [in, out]``."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = Parameter(torch.Tensor(in_features, out_features))
        if bias:
            self.bias = Parameter(torch.Tensor(out_features))
            init.constant_(self.bias, 0)
        else:
            self.register_parameter("bias", None)
        init.xavier_uniform_(self.weight)

    def forward(self, x, adj):
        out = torch.mm(adj, torch.mm(x, self.weight))
        return out if self.bias is None else out + self.bias

    def __repr__(self):
        return f"{type(self).__name__} ({self.in_features} -> {self.out_features})"


def sym_norm_(adj):
    """``vectorized_sym_norm``: ``adj += I`` IN PLACE, then ``D^-1/2 adj D^-1/2`` with the row sums on both sides."""
    adj += torch.eye(adj.shape[1], device=adj.device, dtype=adj.dtype)
    inv = 1.0 / adj.sum(dim=-1, keepdim=True).sqrt()
    inv[torch.isinf(inv)] = 0.0
    return (inv * adj) * inv.transpose(0, 1)


class GNN_VGAE_Encoder(nn.Module):
    def __init__(self, in_dim, hs, dim_d, dim_y, dim_m, droprate, backbone="gcn"):
        super().__init__()
        if backbone != "gcn":
            raise NotImplementedError(f"DGDA: only backbone='gcn' is supported, got {backbone!r}")
        self.backbone = backbone
        self.dims = (dim_d, dim_y, dim_m)
        self.gnn0 = BatchGraphConvolution(in_dim, hs)
        self.gnn1 = BatchGraphConvolution(hs, hs)
        self.d_gnn2 = BatchGraphConvolution(hs, 2 * dim_d)
        self.y_gnn2 = BatchGraphConvolution(hs, 2 * dim_y)
        self.m_gnn2 = BatchGraphConvolution(hs, 2 * dim_m)
        self.act = nn.ReLU()
        self.dropout = nn.Dropout(droprate)

    def repara(self, mu, lv, eps=None):
        """``mu + eps * exp(lv)`` in training (``exp(lv)``, not ``exp(lv / 2)``, as written), ``mu`` otherwise."""
        if not self.training:
            return mu
        if eps is None:
            eps = torch.randn_like(lv)
        return mu + eps * torch.exp(lv)

    def forward(self, x, adj, eps=(None, None, None)):
        adj = sym_norm_(adj)
        res = dict()
        h = self.dropout(self.act(self.gnn0(x, adj)))
        h = self.dropout(self.act(self.gnn1(h, adj)))
        for name, conv in zip("dym", (self.d_gnn2, self.y_gnn2, self.m_gnn2)):
            res[name + "mu"], res[name + "lv"] = conv(h, adj).chunk(chunks=2, dim=-1)
        for name, e in zip("dym", eps):
            res[name] = self.repara(res[name + "mu"], res[name + "lv"], e)
        return res, h


class GraphDiscriminator(nn.Module):
    def __init__(self, in_dim, hs, droprate):
        super().__init__()
        self.lin_0 = nn.Linear(in_dim, hs)
        self.lin_1 = nn.Linear(hs, 1)
        self.act = nn.ReLU()
        self.dropout = nn.Dropout(droprate)

    def forward(self, x):
        h = self.act(self.dropout(self.lin_0(x)))
        return self.lin_1(torch.mean(h, dim=1))


class GraphDecoder(nn.Module):
    def __init__(self, dec_hs, dim_d, dim_y, dim_m, droprate):
        super().__init__()
        self.d_lin0 = DenseLinear(dim_d, dim_d)
        self.y_lin0 = DenseLinear(dim_y, dim_y)
        self.m_lin0 = DenseLinear(dim_m, dim_m)
        self.dym_lin1 = DenseLinear(dim_d + dim_y + dim_m, dec_hs)
        self.dropout = nn.Dropout(droprate)
        self.act = nn.ReLU()

    def embed(self, d, y, m):
        """The decoder's input ``dym`` ([N, dec_hs]); the reconstruction is ``dym dym^T``."""
        d = self.dropout(self.act(self.d_lin0(d)))
        y = self.dropout(self.act(self.y_lin0(y)))
        m = self.dropout(self.act(self.m_lin0(m)))
        return self.dym_lin1(torch.cat([d, y, m], dim=-1))

    def forward(self, d, y, m):
        dym = self.embed(d, y, m)
        return torch.mm(dym, dym.permute(1, 0))


class NoiseDecoder(nn.Module):
    def __init__(self, dim_m, droprate):
        super().__init__()
        self.m_lin0 = nn.Linear(dim_m, dim_m)
        self.m_lin1 = nn.Linear(dim_m, dim_m)
        self.dropout = nn.Dropout(droprate)
        self.act = nn.ReLU()

    def forward(self, x):
        h = self.m_lin1(self.dropout(self.act(self.m_lin0(x))))
        return torch.mm(h, h.permute(1, 0))


class ClassClassifier(nn.Module):
    def __init__(self, hs, n_class, droprate):
        super().__init__()
        self.lin0 = DenseLinear(hs, hs)
        self.lin1 = DenseLinear(hs, n_class)
        self.dropout = nn.Dropout(droprate)
        self.act = nn.ReLU()

    def forward(self, x):
        return self.lin1(self.dropout(self.act(self.lin0(x))))


class DomainClassifier(nn.Module):
    def __init__(self, dim_d):
        super().__init__()
        self.lin = DenseLinear(dim_d, 1)

    def forward(self, x):
        return self.lin(x)


class DGDABase(nn.Module):
    def __init__(self, in_dim, num_class, enc_hs, dec_hs, dim_d, dim_y, dim_m, droprate, backbone,
                 source_pretrained_emb, source_vertex_feats, target_pretrained_emb, target_vertex_feats):
        super().__init__()
        self.feat_dim = int(in_dim)
        for name, table in (("semb", source_pretrained_emb), ("temb", target_pretrained_emb)):
            emb = nn.Embedding(table.size(0), table.size(1))
            emb.weight = Parameter(table, requires_grad=False)
            setattr(self, name, emb)
        in_dim += int(source_pretrained_emb.size(1))
        for name, table in (("svf", source_vertex_feats), ("tvf", target_vertex_feats)):
            emb = nn.Embedding(table.size(0), table.size(1))
            emb.weight = Parameter(table, requires_grad=False)
            setattr(self, name, emb)
        in_dim += int(source_vertex_feats.size(1))
        self.encoder = GNN_VGAE_Encoder(in_dim, enc_hs, dim_d, dim_y, dim_m, droprate, backbone)
        self.graphDiscriminator = GraphDiscriminator(enc_hs, enc_hs // 2, droprate)
        self.graph_decoder = GraphDecoder(dec_hs, dim_d, dim_y, dim_m, droprate)
        self.noise_decoder = NoiseDecoder(dim_m, droprate)
        self.classClassifier = ClassClassifier(dim_y, num_class, droprate)
        self.domainClassifier = DomainClassifier(dim_d)

    def forward(self, x, vts, adj, domain, recon=True, alpha=1.0, eps=(None, None, None)):
        """The reference's forward on the host.  ``adj`` is a dense matrix and is mutated in place (``+= I``)."""
        emb, vf = (self.semb, self.svf) if domain == 0 else (self.temb, self.tvf)
        x = torch.cat((x, emb(vts)), dim=-1)
        x = torch.cat((x, vf(vts)), dim=-1)
        res, h = self.encoder(x, adj, eps)
        if recon:
            res["a_recons"] = self.graph_decoder(res["d"], res["y"], res["m"])
            res["m_recons"] = self.noise_decoder(res["m"])
        res["dom_output"] = self.domainClassifier(GradReverse.apply(res["d"], alpha))
        res["cls_output"] = self.classClassifier(res["y"])
        return res
