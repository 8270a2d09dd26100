"""``CWGCN`` trainer (pygda/models/cwgcn.py:17-458): correntropy-induced Wasserstein GCN, in two stages.

Stage 1 (:258-292): ``2 * epoch`` epochs over the source loader only; the correntropy-induced loss ``c_loss``
(pygda/nn/cwgcn_base.py:193-219) under Adam with weight decay; the log line is the sum of the batch losses and the
source accuracy.  Between the stages (:295-304) the parameters named exactly ``cls.bias`` / ``cls.lin.weight`` are
frozen (which ones exist depends on the backbone) and a FRESH Adam is built over all parameters.  Stage 2 (:306-350):
``epoch`` epochs over the target loader only, loss ``sum (mean_s - mean_t)^2 + sum (std_s - std_t)^2`` of conv1's
output, ``std_t, mean_t = torch.std_mean(., dim=0)`` over the target batch, ``(mean_s, std_s)`` =
``get_src_mean_std(x_list[1], weight)`` (:423-458) of the LAST stage-1 batch (its forward, before its optimiser step),
detached.  The layer-0 terms of :311 and :324-325 are overwritten before use and are not computed.  The classifier is
outside the stage-2 loss: it receives no gradient and leaves stage 2 bit-identical.  The stage-2 log line is the LAST
batch's loss and the target accuracy (``target=``).

Every stage-1 step writes the weighted source moments of its own batch into a persistent pair of device buffers
(csrc/gda_cwgcn.hip), so after the last step -- eager, or replayed from a hipGraph several steps at a time -- they hold
what the reference computes from the batch it last saw; stage 2 reads them.

Full batches in node mode: both stages replay as hipGraphs (BaseGDA._train_epochs; a second capture for the second
optimiser; a stage hands its one loader's batch in both slots of the step).  Mini-batches and graph mode run eagerly.

Label range: ``c_loss`` one-hot encodes with width ``max(y) + 1`` and the reference raises where that is not the
logits' width; ``fit`` checks the source labels once and raises ``ValueError``.  A mini-batch that happens to lack the
top class trains here (its rows simply match no missing column) where the reference would raise on that batch.
Out of scope, raised before any device work: data-parallel runs and ``edge_weight``."""
import time

import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn import CWGCNBase
from ..ops import std_mean_match, weighted_moments
from .base import BaseGDA


class CWGCN(BaseGDA):
    def __init__(self, in_dim, hid_dim, num_classes, mode='node', num_layers=2, dropout=0., gnn='gcn', act=F.relu,
                 weight_decay=0.0001, lr=0.001, epoch=200, device='cuda:0', batch_size=0, num_neigh=-1, verbose=2,
                 **kwargs):
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        assert gnn in ('gcn', 'sage', 'gat', 'gin'), 'Invalid gnn backbone'                  # :94-95
        assert num_layers == 2, 'unsupport number of layers'
        assert mode in ('graph', 'node'), 'Invalid train mode'
        self.arc, self.mode = gnn, mode
        self.stage = 0                 # 1 / 2 while the stages run (an epoch_hook may read it)

    def init_model(self, **kwargs):
        return CWGCNBase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes,
                         num_layers=self.num_layers, dropout=self.dropout, act=self.act, gnn=self.arc, mode=self.mode,
                         **kwargs).to(self.device)

    def _forward(self, data):
        return self.gnn(data.x, data.edge_index, batch=data.batch if self.mode == 'graph' else None)

    def forward_model(self, source_data):
        """(:144-176) ``(loss, source_logits, weight, x_list)`` of one source batch."""
        source_logits, x_list = self._forward(source_data)
        loss, weight = self.gnn.c_loss(source_logits, source_data.y)
        return loss, source_logits, weight, x_list

    def _check_scope(self, source_data, target_data):
        from ..distributed import active
        if active():
            raise NotImplementedError("CWGCN: data-parallel training is not supported")
        graphs = (list(source_data) + list(target_data)) if self.mode == 'graph' else [source_data, target_data]
        if any(getattr(g, "edge_weight", None) is not None for g in graphs):
            raise NotImplementedError("CWGCN: edge_weight is not supported (the reference never passes it, "
                                      "pygda/models/cwgcn.py:170,318)")
        y = torch.cat([g.y.reshape(-1) for g in source_data]) if self.mode == 'graph' else source_data.y
        top = int(y.max()) + 1
        if top != self.num_classes:
            raise ValueError(f"CWGCN: the source labels span {top} classes but num_classes is {self.num_classes}: "
                             "c_loss's one_hot would not match the logits (pygda/nn/cwgcn_base.py:213-215)")

    def _optimizer(self):
        if torch.device(self.device).type == "cuda":
            from ..optim import Adam
            return Adam(list(self.gnn.parameters()), lr=self.lr, weight_decay=self.weight_decay)
        return torch.optim.Adam(self.gnn.parameters(), lr=self.lr, weight_decay=self.weight_decay, foreach=False)

    def fit(self, source_data, target_data):
        self._check_scope(source_data, target_data)
        self._loaders(source_data, target_data)                                                # :230-256
        self.gnn = self.init_model(**self.kwargs)
        cuda = torch.device(self.device).type == "cuda"
        self._graph_safe_step = self._graph_unroll_ok = cuda
        self._graphed = None
        self.src_stats = tuple(torch.zeros(self.hid_dim, dtype=torch.float32, device=self.device) for _ in range(2))
        start = time.time()

        def step1(batch):
            loss, logits, weight, x_list = self.forward_model(batch)
            weighted_moments(x_list[1], weight, out=self.src_stats)                            # :423-458, detached
            return loss, logits

        def step2(batch):
            logits, tgt_list = self._forward(batch)
            return std_mean_match(tgt_list[1], *self.src_stats), logits                        # :327-328

        print('Step 1, train source data...')
        self.stage = 1
        self._stage(self.source_loader, self._optimizer(), step1, range(self.epoch * 2), "source_train_acc", True, start)
        for k, v in self.gnn.named_parameters():                                               # :295-298
            if k == 'cls.bias' or k == 'cls.lin.weight':
                v.requires_grad = False
        print('Step 2, train target data...')
        self.stage = 2
        self._stage(self.target_loader, self._optimizer(), step2, range(self.epoch), "target", False, start)
        self.stage = 0

    def _stage(self, loader, optimizer, step, epochs, acc_key, sum_losses, start):
        self._log_acc_key = acc_key
        try:
            self._stage_epochs(loader, optimizer, step, epochs, sum_losses, start)
        finally:
            del self._log_acc_key

    def _stage_epochs(self, loader, optimizer, step, epochs, sum_losses, start):
        if self.mode == 'node' and self.batch_size == 0:
            # one full batch: the shared loop, captured when it can be; the stage's loader fills both slots
            saved = self.source_loader, self.target_loader
            self.source_loader = self.target_loader = loader
            self._graphed = None
            try:
                self._train_epochs(self.gnn, optimizer, lambda s, t, a, e: step(s), lambda e: 0.0, epochs=epochs)
            finally:
                self.source_loader, self.target_loader = saved
                self._graphed = None
            return
        cuda = torch.device(self.device).type == "cuda"
        for epoch in epochs:
            epoch_loss, logits, labels = 0.0, [], []
            for batch in loader:
                self.gnn.train()
                batch = batch.to(self.device)
                if cuda:
                    from ..ops import dropout_state
                    dropout_state.next_step(batch.x.device)
                loss, batch_logits = step(batch)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
                epoch_loss = epoch_loss + loss.item() if sum_losses else loss.item()            # :270 / :336
                logits.append(batch_logits.detach())
                labels.append(batch.y)
            acc = eval_micro_f1(torch.cat(labels), torch.cat(logits).argmax(dim=1))
            self._report(epoch, epoch_loss, acc, start)

    def process_graph(self, data):
        pass

    def predict(self, data, source=False, reference_compat=None):
        """(:368-421) raw logits and labels over the loader ``fit`` stored (``data`` is ignored), in eval mode."""
        self.gnn.eval()
        loader = self.source_loader if source else self.target_loader
        return self._predict_loader(loader, lambda b: self._forward(b)[0], reference_compat)

    def get_src_mean_std(self, embedding, weight):
        """(:423-458) the weighted source mean and bias-corrected std, detached."""
        return weighted_moments(embedding, weight)
