"""The modules of KBL / Bridged-GNN (pygda/nn/kbl_base.py) under the reference's class and state-dict names, on the
project's layers: ``SAGEConv`` and ``GNNBase`` on the SpMM, ``Linear`` on the fp32 GEMM kernels, the fused
ReLU-dropout of ``ops.relu_dropout``.  Host tensors take the torch restatements of ``nn.host``.

``BridgedGraph`` keeps the two domains, the ``AdversarialLearner`` and the numbers the reference hard-codes; its
epochs and the bridge generation are driven by ``pygda_amd.models.KBL``.  ``PairEnumerator.sampling`` calls
``np.random`` in the reference's order and returns the two index LISTS whose Cartesian product the reference
enumerates (``ops.kbl_pair_bce`` takes the lists); ``enumerate_pairs`` restates the enumeration itself.

``BatchNorm1d`` is ``torch.nn.BatchNorm1d`` in parameters, buffers and state dict (running mean, unbiased running
variance, momentum 0.1); on device tensors its forward is spelled out in torch's reductions, so that it is captured
like any other launch and the eval-mode bridge generation reads the statistics the training epochs left."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .gnn_base import GNNBase
from .host import _host_conv
from .linear import Linear
from .sage_gin_conv import SAGEConv


def _relu_dropout(x, p, training):
    if x.is_cuda:
        from ..ops import relu_dropout
        return relu_dropout(x, p, training)
    return F.dropout(F.relu(x), p=p, training=training)


class BatchNorm1d(nn.BatchNorm1d):
    def forward(self, x):
        if not x.is_cuda:
            return super().forward(x)
        if self.training:
            n = x.size(0)
            mean, var = x.mean(dim=0), x.var(dim=0, unbiased=False)
            with torch.no_grad():
                m = self.momentum
                self.running_mean.mul_(1 - m).add_(mean, alpha=m)
                self.running_var.mul_(1 - m).add_(var * (n / max(n - 1, 1)), alpha=m)
                self.num_batches_tracked.add_(1)
        else:
            mean, var = self.running_mean, self.running_var
        return (x - mean) * torch.rsqrt(var + self.eps) * self.weight + self.bias


class PairNorm(nn.Module):
    def __init__(self, mode='PN', scale=10):
        assert mode in ['None', 'PN', 'PN-SI', 'PN-SCS']
        super().__init__()
        self.mode, self.scale = mode, scale

    def forward(self, x):
        if self.mode == 'None':
            return x
        col_mean = x.mean(dim=0)
        if self.mode == 'PN':
            x = x - col_mean
            x = self.scale * x / (1e-6 + x.pow(2).sum(dim=1).mean()).sqrt()
        if self.mode == 'PN-SI':
            x = x - col_mean
            x = self.scale * x / (1e-6 + x.pow(2).sum(dim=1, keepdim=True)).sqrt()
        if self.mode == 'PN-SCS':
            x = self.scale * x / (1e-6 + x.pow(2).sum(dim=1, keepdim=True)).sqrt() - col_mean
        return x


class GraphEncoder(nn.Module):
    def __init__(self, dim_in, dim_out, dim_hidden=64, layer_num=2, root_weight=True, norm_mode='PN-SCS', norm_scale=1,
                 log_softmax=False, dropout=0.5):
        super().__init__()
        dims = [dim_in] + [dim_hidden] * (layer_num - 1) + [dim_out]
        self.convs = nn.ModuleList(SAGEConv(dims[i], dims[i + 1], root_weight=root_weight) for i in range(layer_num))
        self.norm = PairNorm(mode=norm_mode, scale=norm_scale)
        self.log_softmax, self.dropout = log_softmax, dropout

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, x, edge_index):
        last = len(self.convs) - 1
        for ind, conv in enumerate(self.convs):
            x = conv(x, edge_index) if x.is_cuda else _host_conv(conv, x, edge_index)
            if ind != last:
                x = _relu_dropout(self.norm(x), self.dropout, self.training)
        return F.log_softmax(x, dim=1) if self.log_softmax else x


_ACTS = {'relu': nn.ReLU, 'leakyrelu': lambda: nn.LeakyReLU(0.2, inplace=False), 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}


def _act(name):
    if name not in _ACTS:
        raise NotImplementedError('Not Implemented Activation Function:{}'.format(name))
    return _ACTS[name]()


def _mlp_layers(dim_in, dim_hidden, dim_out, num_layer):
    dims = [dim_in] + [dim_hidden] * (num_layer - 1) + [dim_out]
    return nn.ModuleList(Linear(dims[i], dims[i + 1], bias=True, weight_initializer=None) for i in range(num_layer))


class Decoder(nn.Module):
    def __init__(self, dim_in, dim_hidden, dim_out, num_layer=2, use_norm=False, dropout=0.5, act_fn='relu',
                 norm_mode='PN', norm_scale=1.):
        super().__init__()
        self.use_norm, self.dropout, self.num_layer = use_norm, dropout, num_layer
        self.layers = _mlp_layers(dim_in, dim_hidden, dim_out, num_layer)
        if use_norm:
            self.pair_norm = PairNorm(norm_mode, norm_scale)
        self.act_fn = _act(act_fn)
        self.reset_parameters()

    def reset_parameters(self):
        for l in self.layers:
            l.reset_parameters()

    def forward(self, z):
        x = z
        for idx in range(self.num_layer - 1):
            x = self.layers[idx](x)
            if self.use_norm:
                x = self.pair_norm(x)
            x = self.act_fn(x)
        return self.layers[-1](x)


class Discriminator(nn.Module):
    def __init__(self, dim_in, dim_hidden, num_layer=2, use_bn=False, use_pair_norm=False, dropout=0.5,
                 act_fn='leakyrelu', sigmoid_output=True, norm_mode='PN', norm_scale=1.):
        super().__init__()
        self.use_bn, self.dropout, self.num_layer, self.sigmoid_output = use_bn, dropout, num_layer, sigmoid_output
        self.layers = _mlp_layers(dim_in, dim_hidden, 1, num_layer)
        self.use_pair_norm = use_pair_norm
        if use_pair_norm:
            self.pair_norm = PairNorm(mode=norm_mode, scale=norm_scale)
        if use_bn:
            self.bns = nn.ModuleList(BatchNorm1d(dim_hidden) for _ in range(num_layer - 1))
        self.act_fn = _act(act_fn)
        self.reset_parameters()

    def reset_parameters(self):
        for l in self.layers:
            l.reset_parameters()
        if self.use_bn:
            for bn in self.bns:
                bn.reset_parameters()

    def forward(self, z):
        x = z
        for idx in range(self.num_layer - 1):
            x = self.layers[idx](x)
            if self.use_bn:
                x = self.bns[idx](x)
            elif self.use_pair_norm:
                x = self.pair_norm(x)
            x = self.act_fn(x)
        logits = self.layers[-1](x)
        return torch.sigmoid(logits) if self.sigmoid_output else logits


class Similar(nn.Module):
    """``embed(h)`` is what every similarity of the reference compares: ``z + biasatt(z)`` with ``z = lin_self(h)``,
    once per node (the reference applies ``biasatt`` once per pair; per row it is the same function)."""

    def __init__(self, in_channels, num_clf_classes, dropout=0.6, use_clf=True):
        super().__init__()
        # (the reference's kaiming loop over biasatt looks for nn.Linear and finds PyG's Linear: glorot stays)
        self.biasatt = nn.Sequential(Linear(128, 64, bias=True, weight_initializer='glorot'), nn.Tanh(),
                                     Linear(64, 128, bias=True, weight_initializer='glorot'))
        self.use_clf = use_clf
        if use_clf:
            self.lin_clf = Linear(in_channels, num_clf_classes, bias=True, weight_initializer='glorot')
        self.lin_self = nn.Sequential(BatchNorm1d(in_channels),
                                      Linear(in_channels, 64, bias=False, weight_initializer='glorot'),
                                      BatchNorm1d(64), nn.Tanh(),
                                      Linear(64, 128, bias=False, weight_initializer='glorot'))
        self.dropout = dropout
        self.reset_parameters()

    def reset_parameters(self):
        """As the reference: the classifier is drawn again, ``lin_self`` and ``biasatt`` keep their constructors' draws
        (its loops look for ``nn.Linear`` and find PyG's).  PyG draws the bias of a glorot ``Linear`` from
        U(+-1/sqrt(in)); the project's ``Linear`` zeroes it for the GCN layers it was written for."""
        if self.use_clf:
            self.lin_clf.reset_parameters()
        for lin in [self.biasatt[0], self.biasatt[2]] + ([self.lin_clf] if self.use_clf else []):
            with torch.no_grad():
                lin.bias.uniform_(-lin.in_channels ** -0.5, lin.in_channels ** -0.5)

    def embed(self, x):
        z = self.lin_self(x)
        return z + self.biasatt(z)

    def classify(self, x):
        """``log_softmax(lin_clf(dropout(relu(x))))``, or None without the classifier."""
        if not self.use_clf:
            return None
        return F.log_softmax(self.lin_clf(_relu_dropout(x, self.dropout, self.training)), dim=-1)

    def similarity(self, x, idx1, idx2):
        """The reference's line for index tensors of any shape (its bridge generation passes ``[N, 1]`` ones, which
        makes ``CosineSimilarity(dim=1)`` reduce a dimension of size one: see ``pygda_amd.models.kbl``)."""
        u = self.embed(x)
        return torch.sigmoid(F.cosine_similarity(u[idx1], u[idx2], dim=1))

    def forward(self, x, idx1, idx2):
        return self.similarity(x, idx1, idx2).unsqueeze(-1), self.classify(x)


def _num_classes(data):
    return int(data.y.max()) + 1


class SourceLearner(nn.Module):
    def __init__(self, data, dim_hidden=64, norm_mode='None', norm_scale=1, use_clf=True, encoder_dropout=0.5,
                 clf_dropout=0.6):
        super().__init__()
        self.dim_in, self.num_classes, self.dim_hidden = data.x.shape[1], _num_classes(data), dim_hidden
        self.backbone = GraphEncoder(self.dim_in, dim_hidden, dim_hidden=dim_hidden, layer_num=2, root_weight=True,
                                     norm_mode=norm_mode, norm_scale=norm_scale, log_softmax=False,
                                     dropout=encoder_dropout)
        self.sim_net = Similar(dim_hidden, num_clf_classes=self.num_classes, dropout=clf_dropout, use_clf=use_clf)

    def reset_parameters(self):
        self.backbone.reset_parameters()
        self.sim_net.reset_parameters()

    def forward(self, data, idx1, idx2, return_representation=False):
        h = self.backbone(data.x, data.edge_index)
        probs_pair, logits_clf = self.sim_net(h, idx1, idx2)
        return (probs_pair, logits_clf, h) if return_representation else (probs_pair, logits_clf)


class TargetLearnerAE(nn.Module):
    def __init__(self, data, dim_eq_trans=128, dim_hidden=64, norm_mode='None', norm_scale=1, encoder_dropout=0.5):
        super().__init__()
        self.dim_in, self.dim_eq_trans = data.x.shape[1], dim_eq_trans
        self.num_classes, self.dim_hidden = _num_classes(data), dim_hidden
        self.equavilent_trans_layer = nn.Sequential(Linear(self.dim_in, dim_eq_trans, bias=True, weight_initializer=None),
                                                    PairNorm(mode=norm_mode, scale=norm_scale), nn.Tanh())
        self.encoder = GraphEncoder(dim_eq_trans, dim_hidden, dim_hidden=dim_hidden, layer_num=2, root_weight=True,
                                    norm_mode=norm_mode, norm_scale=norm_scale, log_softmax=False,
                                    dropout=encoder_dropout)
        self.decoder = Decoder(dim_hidden, dim_hidden, dim_eq_trans, num_layer=2, use_norm=True, dropout=0.5,
                               act_fn='relu', norm_mode=norm_mode, norm_scale=norm_scale)

    def reset_parameters(self):
        self.encoder.reset_parameters()
        self.decoder.reset_parameters()

    def encode(self, data):
        h0 = self.equavilent_trans_layer(data.x)
        return self.encoder(h0, data.edge_index), h0

    def decode(self, z):
        return torch.tanh(self.decoder(z))

    def forward(self, data):
        z, h0 = self.encode(data)
        return h0, z, self.decode(z)


class AdversarialLearner(nn.Module):
    def __init__(self, data_src, data_tar, dim_hidden=64, num_layer=2, source_clf=True, norm_mode='PN', norm_scale=1.,
                 encoder_dropout=0.5, clf_dropout=0.6):
        super().__init__()
        self.num_layer, self.source_clf = num_layer, source_clf
        self.source_learner = SourceLearner(data_src, dim_hidden=dim_hidden, norm_mode=norm_mode, norm_scale=norm_scale,
                                            use_clf=source_clf, encoder_dropout=encoder_dropout, clf_dropout=clf_dropout)
        self.target_learner = TargetLearnerAE(data_tar, dim_eq_trans=128, dim_hidden=dim_hidden, norm_mode=norm_mode,
                                              norm_scale=norm_scale, encoder_dropout=encoder_dropout)
        self.discriminator = Discriminator(dim_hidden, dim_hidden, num_layer=2, use_pair_norm=False, dropout=0.5,
                                           act_fn='relu', sigmoid_output=True, norm_mode=norm_mode, norm_scale=norm_scale)

    def embeddings(self, data_src, data_tar):
        """``(u_src, u_tar)``: what the bridge generation compares, both through the SOURCE learner's ``sim_net``."""
        sim = self.source_learner.sim_net
        z_tar, _ = self.target_learner.encode(data_tar)
        return sim.embed(self.source_learner.backbone(data_src.x, data_src.edge_index)), sim.embed(z_tar)


def enumerate_pairs(idx1, idx2):
    """The reference's ``pair_enumeration`` of two index lists: the pair ``(p, q)`` at position ``q len(idx1) + p``."""
    return idx1.repeat(idx2.numel()), idx2.repeat_interleave(idx1.numel())


class PairEnumerator:
    def __init__(self, data, mode='train'):
        self.num_classes = _num_classes(data)
        self.mode = mode
        y = data.y.cpu()
        mask = {'train': lambda: data.train_mask, 'val': lambda: data.val_mask, 'test': lambda: data.test_mask,
                'all': lambda: data.train_mask + data.val_mask + data.test_mask}
        if mode not in mask:
            raise NotImplementedError('Not Implemented Mode:{}'.format(mode))
        keep = mask[mode]().cpu().bool()
        self.class_bucket = {lbl: torch.nonzero((y == lbl) & keep).squeeze(1) for lbl in range(self.num_classes)}

    def sampling_lists(self, max_class_num=2, sample_size=40000):
        """The two index lists of one ``sampling`` call, drawn as the reference draws them: the classes without
        replacement when there are more than ``max_class_num``, then per class two draws with replacement."""
        if self.num_classes > max_class_num:
            selected = np.random.choice(torch.arange(self.num_classes), replace=False, size=max_class_num)
        else:
            selected = np.arange(self.num_classes).astype(np.int8)
        per_class = int(np.sqrt(sample_size) / max_class_num)
        idx1, idx2 = [], []
        for lbl in selected:
            idx1.append(torch.from_numpy(np.random.choice(self.class_bucket[int(lbl)], size=per_class)).long())
            idx2.append(torch.from_numpy(np.random.choice(self.class_bucket[int(lbl)], size=per_class)).long())
        return torch.cat(idx1), torch.cat(idx2)

    def sampling(self, max_class_num=2, sample_size=40000, shuffle=False):
        if shuffle:
            raise NotImplementedError("PairEnumerator.sampling: shuffle=True is not used by KBL")
        return enumerate_pairs(*self.sampling_lists(max_class_num, sample_size))


class BridgedGraph(nn.Module):
    def __init__(self, data_src, data_tar, k_cross=20, k_within=6, epsilon=0.5, dim_hidden=64, batch_size=1000,
                 num_layer=2, num_epoch=200, lr=0.001, weight_decay=5e-3, source_clf=True, norm_mode='PN', norm_scale=1.,
                 device=None, encoder_dropout=0.5, clf_dropout=0.6):
        super().__init__()
        self.data_src, self.data_tar = data_src, data_tar
        self.k_cross, self.k_within, self.epsilon = k_cross, k_within, epsilon
        self.dim_hidden, self.num_layer, self.num_epoch = dim_hidden, num_layer, num_epoch
        self.lr, self.weight_decay = lr, weight_decay
        self.source_clf, self.norm_mode, self.norm_scale, self.device = source_clf, norm_mode, norm_scale, device
        self.model = AdversarialLearner(data_src, data_tar, dim_hidden=dim_hidden, num_layer=num_layer,
                                        source_clf=source_clf, norm_mode=norm_mode, norm_scale=norm_scale,
                                        encoder_dropout=encoder_dropout, clf_dropout=clf_dropout)

    def param_groups(self):
        """The reference's ``optimizer_src_tar`` (two groups) and ``optimizer_d`` as three groups of one Adam: a step
        moves the parameters that hold a gradient.  The reference writes 1e-3 and 5e-3 into some groups and passes ``lr``
        and ``weight_decay`` (the same numbers) to the others; here every group takes the two arguments."""
        m = self.model
        kw = dict(lr=self.lr, weight_decay=self.weight_decay)
        return [dict(params=list(m.source_learner.parameters()), betas=(0.9, 0.999), **kw),
                dict(params=list(m.target_learner.parameters()), betas=(0.5, 0.999), **kw),
                dict(params=list(m.discriminator.parameters()), betas=(0.5, 0.999), **kw)]


class KBLBase(nn.Module):
    def __init__(self, data_src, data_tar, device, k_cross=20, k_within=6, epsilon=0.5, bridge_batch_size=1000,
                 dim_hidden=64, num_layer=2, num_epoch=200, lr=0.001, weight_decay=5e-3, source_clf=True, norm_mode='PN',
                 norm_scale=1., encoder_dropout=0.5, clf_dropout=0.6, gnn_dropout=0.1):
        super().__init__()
        self.bridged_graph = BridgedGraph(data_src, data_tar, k_cross=k_cross, k_within=k_within,
                                          batch_size=bridge_batch_size, dim_hidden=dim_hidden, num_layer=num_layer,
                                          num_epoch=num_epoch, lr=lr, weight_decay=weight_decay, source_clf=source_clf,
                                          norm_mode=norm_mode, norm_scale=norm_scale, device=device,
                                          encoder_dropout=encoder_dropout, clf_dropout=clf_dropout)
        self.bridge_batch_size = bridge_batch_size
        self.gnn = GNNBase(in_dim=data_src.x.shape[1], hid_dim=dim_hidden, num_classes=_num_classes(data_src),
                           num_layers=num_layer, dropout=gnn_dropout, act=F.relu, gnn='gcn')

    def forward(self, data):
        return self.gnn(data.x, data.edge_index)
