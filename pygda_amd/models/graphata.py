"""``GraphATA`` trainer (pygda/models/graphata.py): Aggregate to Adapt -- node-centric aggregation for multi-source-free
graph domain adaptation (node level).

``fit(source_data_list, target_data)`` keeps the reference's behaviour:

* one :class:`~pygda_amd.nn.GNNBase` and one FRESH Adam per source graph, ``epoch`` pretraining epochs of the
  cross-entropy each, the log's accuracy the micro-F1 of the training pass's arg-max;
* then a :class:`~pygda_amd.nn.GraphATABase` over the source models' layer weights and classifiers and a NEW Adam over
  all source parameters plus GraphATABase's; ``epoch`` adaptation epochs on the target alone.  Per epoch: a train-mode
  forward; information maximisation (``ent + div``) plus the cross-entropy against pseudo labels -- the first arg-max of
  the mean class memory over the ``K`` nearest rows of the feature memory (cosine; rank 1 of the ``K + 1`` is dropped,
  whichever row it is); the step; an eval-mode forward whose bottleneck output and sharpened softmax move the two
  memory banks by ``momentum``.  The reference then calls ``predict`` for the log's target micro-F1: that is the same
  computation as the eval-mode forward before it (same weights, eval mode), so it runs once here and the log's
  accuracy is taken from it;
* parameters that receive no gradient during adaptation stay untouched -- no weight decay reaches them: the source
  convolutions' biases, and the classifier entry of the collected ``lin.weight`` lists, which no layer uses;
* the feature memory is ``torch.rand(N, hid_dim)`` drawn from the CPU generator after the models are built, then moved;
  the class memory starts at exactly ``1 / C``, so every pseudo label of the first epoch is class 0.

``predict(data)`` returns the eval-mode log-probabilities of GraphATABase and ``data.y``.

On the GPU a layer is restated through two identities that hold in exact arithmetic (pygda_amd/nn/node_centric_conv.py:
one aggregation instead of two, folded score vectors instead of ``S`` score projections), layer 0's aggregates are
computed once per fit, the blend is ``ops.ata_mix``, the head and the whole loss with its gradient ``ops.ata_head_loss``
over ONE width-``S C`` aggregation, the neighbours ``ops.cta_knn`` on normalised rows (no ``[N, N]`` array), the vote
``ops.ata_vote``, the memory ``ops.ata_memory_update``; dropout is the keep-bit stream of csrc/gda_dropout.h.  Both
phases go through ``epoch_graph.run_epochs`` and neither epoch has a host decision in it: ``epochs_per_graph`` epochs
per hipGraph replay, the same bits as eager epochs.  An adaptation epoch moves the two memory banks in place, so the
capture rolls them back with the parameters, the optimiser's state and the dropout counter.  (The layers read the source
models' parameters themselves: a transposed view made once, when the layer is built, as the reference does, is an
autograd node of the stream the layer was built on, and a backward pass recorded on another stream does not get past
it -- pygda_amd/nn/node_centric_conv.py.)  ``device='cpu'`` restates the reference's lines in torch (any dtype): a seeded host fit follows the reference, dropout
included.

Supported: ``mode='node'``, ``batch_size=0``, ``gnn='gcn'``, any ``S >= 1`` source graphs; anything else raises
NotImplementedError naming the argument.  Data-parallel runs are refused.  Private keywords: ``record=True`` keeps every
adaptation epoch's ``[loss, ent, div, ce]`` in ``parts_log``, its pseudo labels in ``pred_log``, its sorted neighbour
sets in ``near_log`` and the layers' sparsemax support sizes in ``supp_log``; ``init_hook(stage, obj)`` runs after
``init_model`` (``"sources"``, the list of models) and after GraphATABase is built (``"graphata"``, the module) -- tests
load a recorded state there."""
import time

import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn import GNNBase, GraphATABase
from ..nn.host import _host_bottleneck, _host_conv
from .own_epoch import SourceFreeGDA, refuse_data_parallel


class GraphATA(SourceFreeGDA):
    _target_accuracy = True       # the reference logs the target's micro-F1 in every adaptation epoch

    def __init__(self, in_dim, hid_dim, num_classes, num_src_domains, K=10, momentum=0.9, num_layers=3, dropout=0.,
                 act=F.relu, weight_decay=0., lr=1e-4, epoch=200, gnn='gcn', mode='node', device='cuda:0', batch_size=0,
                 num_neigh=-1, verbose=2, **kwargs):
        self.record = bool(kwargs.pop("record", False))
        self.init_hook = kwargs.pop("init_hook", None)
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        if mode != 'node':
            raise NotImplementedError("GraphATA: mode != 'node' is not supported (only node-level tasks)")
        if batch_size != 0:
            raise NotImplementedError("GraphATA: batch_size != 0 is not supported (only full-batch training, "
                                      "batch_size=0)")
        if gnn != 'gcn':
            raise NotImplementedError("GraphATA: gnn != 'gcn' is not supported (the node-centric layers read the source "
                                      "models' GCN weights)")
        if num_src_domains < 1 or K < 1:
            raise ValueError("GraphATA: num_src_domains and K must be at least 1")
        self.gnn, self.mode, self.num_src_domains, self.K, self.momentum = gnn, mode, int(num_src_domains), int(K), momentum
        self._reset_logs()

    def _reset_logs(self):
        self.source_log = [[] for _ in range(self.num_src_domains)]
        self.target_log, self.parts_log, self.pred_log, self.near_log, self.supp_log = [], [], [], [], []
        self._phase, self._src = "source", 0

    def init_model(self, **kwargs):
        self.source_model_list = [GNNBase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes,
                                          num_layers=self.num_layers, dropout=self.dropout, gnn=self.gnn, mode=self.mode,
                                          **kwargs).to(self.device) for _ in range(self.num_src_domains)]
        return self.source_model_list

    def _report(self, epoch, loss, acc, start):
        (self.source_log[self._src] if self._phase == "source" else self.target_log).append((loss, acc))
        super()._report(epoch, loss, acc, start)

    def _check(self, source_data_list, target_data):
        from ..ops import ATA_MAX_CLASSES, ATA_MAX_SOURCES, CTA_MAX_K1, WGCN_MAX_WIDTH
        refuse_data_parallel(self)
        if not isinstance(source_data_list, (list, tuple)) or len(source_data_list) != self.num_src_domains:
            raise ValueError(f"GraphATA: fit takes a list of num_src_domains = {self.num_src_domains} source graphs, got "
                             f"{len(source_data_list) if isinstance(source_data_list, (list, tuple)) else type(source_data_list).__name__}")
        self._check_edges(*source_data_list, target_data)
        for s in source_data_list:
            self._check_labels(s.y)
        n = target_data.x.shape[0]
        if n < self.K + 1:
            raise ValueError(f"GraphATA: K + 1 = {self.K + 1} neighbours need as many target nodes, got {n}")
        if torch.device(self.device).type == "cuda" and (
                self.num_classes > ATA_MAX_CLASSES or self.num_src_domains > ATA_MAX_SOURCES
                or self.hid_dim > WGCN_MAX_WIDTH or self.K + 1 > CTA_MAX_K1):
            raise ValueError(f"GraphATA: the kernels cover up to {ATA_MAX_SOURCES} sources, {ATA_MAX_CLASSES} classes, "
                             f"hidden widths up to {WGCN_MAX_WIDTH} and K up to {CTA_MAX_K1 - 1}, got "
                             f"{self.num_src_domains}, {self.num_classes}, {self.hid_dim}, {self.K}")

    # -- fit -----------------------------------------------------------------------------------------------------------
    def fit(self, source_data_list, target_data):
        self._check(source_data_list, target_data)
        dev = torch.device(self.device)
        on_gpu = dev.type == "cuda"
        sources, t = [self._dom(s, dev) for s in source_data_list], self._dom(target_data, dev)
        self._reset_logs()
        models = self.init_model(**self.kwargs)
        if not on_gpu:
            for m in models:
                m.to(t.x.dtype)
        if self.init_hook is not None:
            self.init_hook("sources", models)
        if on_gpu:
            from ..optim import Adam
        else:
            Adam = torch.optim.Adam
        start = time.time()
        for self._src, (model, s) in enumerate(zip(models, sources)):
            self.optimizer = Adam(model.parameters(), lr=self.lr, weight_decay=self.weight_decay)
            (self._device_pretrain if on_gpu else self._host_pretrain)(model, s, start)
        self._phase = "target"
        param_group = [p for model in models for p in model.parameters()]
        weight_list = [[p for name, p in model.named_parameters() if name[-10:] == 'lin.weight'] for model in models]
        self.graphata = GraphATABase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes,
                                     model_weights=list(zip(*weight_list)), model_list=models,
                                     num_layers=self.num_layers, dropout=self.dropout, act=self.act, gnn=self.gnn,
                                     mode=self.mode, **self.kwargs).to(dev)
        if not on_gpu:
            self.graphata.to(t.x.dtype)
        if self.init_hook is not None:
            self.init_hook("graphata", self.graphata)
        param_group += list(self.graphata.parameters())
        self.optimizer = Adam(param_group, lr=self.lr, weight_decay=self.weight_decay)
        # the reference draws the feature memory on the host, after the models are built
        self.mem_fea = torch.rand(t.n, self.hid_dim).to(dev, t.x.dtype)
        self.mem_cls = (torch.ones(t.n, self.num_classes) / self.num_classes).to(dev, t.x.dtype)
        self._log_acc_key = "target"
        try:
            (self._device_adapt if on_gpu else self._host_adapt)(t, start)
        finally:
            del self._log_acc_key

    # -- what both devices share ---------------------------------------------------------------------------------------
    def _pseudo_labels(self, feat):
        """``(pred [N], idx_near [N, K + 1])`` from the bottleneck's output and the two memory banks; no gradient."""
        from ..ops import ata_vote, cta_knn
        with torch.no_grad():
            feat_norm, mem_fea_norm = F.normalize(feat.detach(), dim=1), F.normalize(self.mem_fea, dim=1)
            if feat.is_cuda:
                idx_near, _ = cta_knn(feat_norm, mem_fea_norm, self.K + 1)
            else:             # the reference's line: a zero row (dropout) ties with every row, and topk breaks the tie
                _, idx_near = torch.topk(feat_norm @ mem_fea_norm.T, dim=-1, largest=True, k=self.K + 1)
            return ata_vote(idx_near, self.mem_cls), idx_near

    def _eval_pass(self, t):
        """The eval-mode forward behind the step: the memory update, and the logits the log's accuracy is taken from."""
        from ..ops import ata_head_loss, ata_memory_update
        net = self.graphata
        net.eval()
        with torch.no_grad():
            feat = net.feat_bottleneck(t.x, t.edge_index)
            logits = ata_head_loss(net.cls.outputs(feat, t.edge_index), net.cls.att.to(feat.dtype))
            ata_memory_update(logits, feat, self.mem_cls, self.mem_fea, self.momentum)
        return logits

    def _supports(self):
        return torch.stack([(conv.last_w != 0).sum(dim=1) for conv in self.graphata.convs])

    # -- the host fit: the reference's lines ---------------------------------------------------------------------------
    def _host_pretrain(self, model, s, start):
        def source_epoch(epoch):
            model.train()
            logits = _host_conv(model.cls, _host_bottleneck(model, s.x, s.edge_index), s.edge_index)
            return (F.nll_loss(F.log_softmax(logits, dim=1), s.y),
                    lambda: eval_micro_f1(s.y, logits.detach().argmax(dim=1)))

        self._host_epochs(self.optimizer, source_epoch, start)

    def _host_adapt(self, t, start):
        from ..ops import ata_head_loss
        net = self.graphata

        def target_epoch(epoch):
            net.train()
            feat = net.feat_bottleneck(t.x, t.edge_index)
            Z = net.cls.outputs(feat, t.edge_index)
            pred, idx_near = self._pseudo_labels(feat)
            loss, parts, _ = ata_head_loss(Z, net.cls.att.to(feat.dtype), pred)
            if self.record:
                self.parts_log.append(parts.tolist())
                self.pred_log.append(pred.clone())
                self.near_log.append(torch.sort(idx_near[:, 1:], dim=1).values)
                self.supp_log.append(self._supports())

            def accuracy():
                self.mem_fea, self.mem_cls = self.mem_fea.clone(), self.mem_cls.clone()
                return eval_micro_f1(t.y, self._eval_pass(t).argmax(dim=1))

            return loss, accuracy

        self._host_epochs(self.optimizer, target_epoch, start)

    # -- the device fit ------------------------------------------------------------------------------------------------
    @staticmethod
    def _device_logits(model, x, edge_index):
        """``GNNBase``'s layers with the activation and the dropout between them in one kernel, the keep bits from the
        project's stream (``GNNBase`` itself calls torch's dropout, whose generator a capture's warm-up advances)."""
        from ..ops import relu_dropout
        last = len(model.convs) - 1
        for i, conv in enumerate(model.convs):
            x = conv(x, edge_index)
            if i < last:
                x = relu_dropout(x, model.dropout, model.training)
        return model.cls(x, edge_index)

    def _device_pretrain(self, model, s, start):
        from ..epoch_graph import run_epochs
        from ..ops import dropout_state
        run_epochs(self, lambda u: self._source_epoch(model, s, u), s.n, self._slots(), self._want_hip_graph(),
                   also=[dropout_state.counter(s.x.device)])

    def _source_epoch(self, model, s, u):
        from ..ops import ce_stats_for, dropout_state, source_ce
        dropout_state.next_step(s.x.device)
        model.train()
        logits = self._device_logits(model, s.x, s.edge_index)
        loss = source_ce(logits, s.y)
        stats = ce_stats_for(logits, s.y)
        self._step(u, loss, hit=stats[1] if stats is not None else (logits.detach().argmax(dim=1) == s.y).sum())

    def _device_adapt(self, t, start):
        from ..epoch_graph import run_epochs
        from ..ops import dropout_state
        U = self._slots(parts=(4,))
        if self.record:
            self._slots(dtype=torch.int64, pred=(t.n,), near=(t.n, self.K), supp=(len(self.graphata.convs), t.n))

        def record(k):
            if self.record:
                self.parts_log.extend(self._parts_buf[:k].tolist())
                self.pred_log.extend(self._pred_buf[:k].clone().cpu().unbind(0))
                self.near_log.extend(self._near_buf[:k].clone().cpu().unbind(0))
                self.supp_log.extend(self._supp_buf[:k].clone().cpu().unbind(0))

        # an epoch moves the two memory banks in place and draws from the dropout stream: what the capture's warm-up and
        # its recording did to them is rolled back with the parameters
        run_epochs(self, lambda u: self._target_epoch(t, u), t.n, U, self._want_hip_graph(), after_group=record,
                   also=[self.mem_cls, self.mem_fea, dropout_state.counter(t.x.device)])

    def _target_epoch(self, t, u):
        """One adaptation epoch into slot ``u``.  No host decision."""
        from ..ops import ata_head_loss, dropout_state, first_argmax
        dropout_state.next_step(t.x.device)
        net = self.graphata
        net.train()
        feat = net.feat_bottleneck(t.x, t.edge_index)
        Z = net.cls.outputs(feat, t.edge_index)
        pred, idx_near = self._pseudo_labels(feat)
        loss, parts, _ = ata_head_loss(Z, net.cls.att, pred)
        if self.record:
            self._pred_buf[u].copy_(pred)
            self._near_buf[u].copy_(torch.sort(idx_near[:, 1:], dim=1).values)
            self._supp_buf[u].copy_(self._supports())
        self._step(u, loss, parts=parts)
        logits = self._eval_pass(t)
        self._hit_buf[u].copy_((first_argmax(logits) == t.y).sum())

    # -- predict -------------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(log-probabilities of GraphATABase in eval mode, data.y)``."""
        self.graphata.eval()
        d = self._dom(data, torch.device(self.device))
        with torch.no_grad():
            logits = self.graphata(d.x, d.edge_index)
        return logits, data.y
