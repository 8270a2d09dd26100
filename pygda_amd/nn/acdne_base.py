"""``ACDNEBase`` (pygda/nn/acdne_base.py): the network embedding (two two-layer encoders, FE1 on a node's own features
and FE2 on its PPMI-weighted neighbour features, joined by ``emb``), the node classifier and the 128 -> 128 -> 2 domain
discriminator behind a gradient reversal.  Same module names, state dict keys and init RNG stream as the reference:
each ``nn.Linear`` draws its default init when built, then ``trunc_normal_`` / ``constant_`` overwrite it, module by
module.  The linear layers are :class:`DenseLinear` (``nn.Linear`` on the hand-written GEMMs for GPU tensors).

Dropout follows the reference's ``F.dropout(x, self.drop)``: always on, in ``predict`` as well.  The trainer runs the
heads (classifier, discriminator, their losses) and the proximity loss as fused kernels on ``pre_embedding``'s output
(pygda_amd/ops.py: acdne_heads, acdne_prox); ``forward`` is the reference's module forward for host tensors and tests."""
import torch
import torch.nn.functional as F
from torch import nn

from ..ops import relu_dropout
from .linear import DenseLinear
from .reverse_layer import GradReverse


def _trunc(lin, std, bias=0.1):
    nn.init.trunc_normal_(lin.weight, std=std, a=-2 * std, b=2 * std)
    nn.init.constant_(lin.bias, bias)


def _drop_relu(x, p):
    """``F.dropout(F.relu(x), p)`` with training always on (the reference's call)."""
    if x.is_cuda and x.dtype == torch.float32:
        return relu_dropout(x, p, True)
    return F.dropout(F.relu(x), p)


class FE1(nn.Module):
    def __init__(self, n_input, n_hidden, drop):
        super().__init__()
        self.drop = drop
        self.h1_self = DenseLinear(n_input, n_hidden[0])
        self.h2_self = DenseLinear(n_hidden[0], n_hidden[1])
        _trunc(self.h1_self, 1 / (n_input / 2) ** 0.5)
        _trunc(self.h2_self, 1 / (n_hidden[0] / 2) ** 0.5)

    def forward(self, x):
        return torch.relu(self.h2_self(_drop_relu(self.h1_self(x), self.drop)))


class FE2(nn.Module):
    def __init__(self, n_input, n_hidden, drop):
        super().__init__()
        self.drop = drop
        self.h1_nei = DenseLinear(n_input, n_hidden[0])
        self.h2_nei = DenseLinear(n_hidden[0], n_hidden[1])
        _trunc(self.h1_nei, 1 / (n_input / 2) ** 0.5)
        _trunc(self.h2_nei, 1 / (n_hidden[0] / 2) ** 0.5)

    def forward(self, x_nei):
        return torch.relu(self.h2_nei(_drop_relu(self.h1_nei(x_nei), self.drop)))


class NetworkEmbedding(nn.Module):
    def __init__(self, n_input, n_hidden, n_emb, drop, batch_size):
        super().__init__()
        self.drop, self.batch_size = drop, batch_size
        self.fe1 = FE1(n_input, n_hidden, drop)
        self.fe2 = FE2(n_input, n_hidden, drop)
        self.emb = DenseLinear(n_hidden[-1] * 2, n_emb)
        _trunc(self.emb, 1 / (n_hidden[-1] * 2) ** 0.5)

    def pre_embedding(self, x, x_nei):
        """``emb``'s input to its final ReLU: the trainer's fused heads apply the ReLU themselves."""
        return self.emb(torch.cat((self.fe1(x), self.fe2(x_nei)), 1))

    def forward(self, x, x_nei):
        return F.relu(self.pre_embedding(x, x_nei))

    def pairwise_constraint(self, emb):
        return emb[:int(self.batch_size / 2), :], emb[int(self.batch_size / 2):, :]

    @staticmethod
    def net_pro_loss(emb, a):
        r = torch.sum(emb * emb, 1)
        r = torch.reshape(r, (-1, 1))
        dis = r - 2 * torch.matmul(emb, emb.T) + r.T
        return torch.mean(torch.sum(a.clone().detach().__mul__(dis), 1))


class NodeClassifier(nn.Module):
    def __init__(self, n_emb, num_class):
        super().__init__()
        self.layer = DenseLinear(n_emb, num_class)
        _trunc(self.layer, 1 / (n_emb / 2) ** 0.5)

    def forward(self, emb):
        return self.layer(emb)


class DomainDiscriminator(nn.Module):
    def __init__(self, n_emb):
        super().__init__()
        self.h_dann_1 = DenseLinear(n_emb, 128)
        self.h_dann_2 = DenseLinear(128, 128)
        self.output_layer = DenseLinear(128, 2)
        _trunc(self.h_dann_1, 1 / (n_emb / 2) ** 0.5)
        _trunc(self.h_dann_2, 0.125)
        _trunc(self.output_layer, 0.125)

    def forward(self, h_grl):
        h_grl = F.relu(self.h_dann_1(h_grl))
        h_grl = F.relu(self.h_dann_2(h_grl))
        return self.output_layer(h_grl)


class ACDNEBase(nn.Module):
    def __init__(self, n_input, n_hidden, n_emb, num_class, batch_size, drop):
        super().__init__()
        self.network_embedding = NetworkEmbedding(n_input, n_hidden, n_emb, drop, batch_size)
        self.node_classifier = NodeClassifier(n_emb, num_class)
        self.domain_discriminator = DomainDiscriminator(n_emb)

    def head_parameters(self):
        """(Wc, bc, W1, b1, W2, b2, W3, b3): the order of ops.acdne_heads."""
        c, d = self.node_classifier.layer, self.domain_discriminator
        return [c.weight, c.bias, d.h_dann_1.weight, d.h_dann_1.bias, d.h_dann_2.weight, d.h_dann_2.bias,
                d.output_layer.weight, d.output_layer.bias]

    def forward(self, x, x_nei, alpha):
        emb = self.network_embedding(x, x_nei)
        pred_logit = self.node_classifier(emb)
        d_logit = self.domain_discriminator(GradReverse.apply(emb, alpha))
        return emb, pred_logit, d_logit
