"""``SAGDA`` trainer (pygda/models/sagda.py:21-390): source CE on the structure-aware source encoder (``SrcGNN`` of
FAConv layers) + gradient-reversed domain CE per domain (MLP discriminator) + annealed target entropy on UDAGCN's
dual-view target encoder.  The loss is UDAGCN's with the source side encoded by ``src_encode``.

The optimiser runs over ``itertools.chain`` of the six models (:229), so the shared conv weights and biases are listed
three times -- encoder, ppmi_encoder, src_encoder -- and the reference's CPU Adam updates them three times per step,
one listing after the other; ``optim.Adam`` does the same in three rounds of duplicates.

Scope: node mode with full batches, which every benchmark sheet uses.  The reference's step sits outside its loader
loop (:264-270), so with mini-batches it trains on the last batch pair only; ``mode='graph'`` and ``batch_size > 0``
raise ``NotImplementedError``, as does ``ppmi=False``, which the reference cannot build (sagda_base.py:322)."""
import itertools

import torch
import torch.nn.functional as F

from ..nn import SAGDABase
from .base import BaseGDA
from .udagcn import UDAGCN


class SAGDA(BaseGDA):
    def __init__(self, in_dim, hid_dim, num_classes, mode='node', beta=1.0, alpha=1.0, num_layers=2, dropout=0.0,
                 act=F.relu, ppmi=True, adv_dim=40, weight_decay=3e-3, lr=4e-3, epoch=200, device='cuda:0',
                 batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        assert beta == 1.0 and alpha == 1.0, 'unsupport for alpha and beta values'            # :108
        if mode == 'graph':
            raise NotImplementedError("SAGDA: mode='graph' is not supported (pygda/models/sagda.py:218-226, 273-277 "
                                      "pool the source encoder's nodes per graph); node mode only")
        if mode != 'node':
            raise ValueError(f"SAGDA: invalid train mode {mode!r}")
        if batch_size != 0:
            raise NotImplementedError("SAGDA: batch_size > 0 is not supported -- the reference steps once per epoch on "
                                      "the last batch pair only (pygda/models/sagda.py:264-270); use batch_size=0")
        if not ppmi:
            raise NotImplementedError("SAGDA: ppmi=False is not supported -- the reference lists ppmi_encoder in "
                                      "SAGDABase.models unconditionally (pygda/nn/sagda_base.py:322)")
        self.ppmi, self.adv_dim, self.alpha, self.beta, self.mode = ppmi, adv_dim, alpha, beta, mode

    def init_model(self, **kwargs):
        return SAGDABase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes,
                         num_layers=self.num_layers, dropout=self.dropout, act=self.act, beta=self.beta,
                         alpha=self.alpha, ppmi=self.ppmi, adv_dim=self.adv_dim, **kwargs).to(self.device)

    _domain_loss = UDAGCN._domain_loss          # GRL + discriminator CE per domain, the fused row kernels on the GPU

    def forward_model(self, source_data, target_data, alpha, epoch):
        net = self.sagda
        encoded_source = net.src_encode(source_data.x, source_data.edge_index)                 # :275
        encoded_target = net.encode(target_data, 'target')                                     # :278
        source_logits = net.cls_model(encoded_source)
        gm = self._gmean
        ns, nt = encoded_source.size(0), encoded_target.size(0)
        from ..ops import softmax_entropy, source_ce
        loss = gm(source_ce(source_logits, source_data.y), ns)                                 # :284
        loss = loss + self._domain_loss(net, encoded_source, encoded_target, alpha, ns, nt)    # :286-299
        target_logits = net.cls_model(encoded_target)                                          # :302-308
        loss_entropy = gm(softmax_entropy(target_logits, 1e-9), nt)
        return loss + loss_entropy * (epoch / self.epoch * 0.01), source_logits, target_logits

    def _prepare(self, source_data, target_data):
        self._loaders(source_data, target_data)                                                # :201-226
        self.sagda = self.init_model(**self.kwargs)
        params = itertools.chain(*[m.parameters() for m in self.sagda.models])                 # :229-235
        if torch.device(self.device).type == "cuda":
            # the shared conv Parameters appear three times; one capturable multi-tensor launch per round of
            # duplicates, each listing updated after the previous one (pygda_amd/optim.py)
            from ..optim import Adam
            optimizer = Adam(list(params), lr=self.lr, weight_decay=self.weight_decay)
            self._graph_safe_step, self._graph_uses_scalars = True, True
        else:
            optimizer = torch.optim.Adam(params, lr=self.lr, weight_decay=self.weight_decay, foreach=False)

        def step(src, tgt, alpha, epoch):
            loss, source_logits, _ = self.forward_model(src, tgt, alpha, epoch)
            return loss, source_logits

        def before_step():
            for m in self.sagda.models:
                m.train()

        return self.sagda, optimizer, step, lambda e: min((e + 1) / self.epoch, 0.05), before_step      # :246

    def fit(self, source_data, target_data):
        self._train_epochs(*self._prepare(source_data, target_data))

    def process_graph(self, data):
        pass

    def predict(self, data, source=False):
        for m in self.sagda.models:
            m.eval()
        if source:                                                                             # :363-375
            loader = self.source_loader
            forward = lambda b: self.sagda.cls_model(self.sagda.src_encode(b.x, b.edge_index))      # noqa: E731
        else:                                                                                  # :376-388
            loader = self.target_loader
            forward = lambda b: self.sagda.cls_model(self.sagda.encode(b, 'target'))                 # noqa: E731
        return self._predict_loader(loader, forward)
