"""``SOGA`` trainer (pygda/models/soga.py): Source Free Graph Unsupervised Domain Adaptation (source-free, node level).

``fit`` pretrains a :class:`~pygda_amd.nn.SOGABase` on the source graph alone -- ``epoch`` epochs of the
label-smoothed cross-entropy, the log's accuracy the micro-F1 of the training pass's arg-max -- and then adapts it on
the target graph alone with the SAME Adam instance (its moments carry over): ``epoch`` epochs of
``IM + struct_lambda NCE_struct + neigh_lambda NCE_neigh`` over the two views' fixed tables, which
``SOGABase.init_target`` draws once between the phases (Python's ``random`` and ``np.random``, in the reference's
order).  The adaptation log carries the loss only.  ``parts_log`` keeps each adaptation epoch's ``[loss, IM, NCE_struct,
NCE_neigh]`` when ``record=True``.  ``predict`` returns the eval-mode logits and the labels.

On the GPU both losses are single ops of csrc/gda_soga.hip (``ops.soga_smooth_ce``, ``ops.soga_adapt`` on an
``ops.soga_plan`` built once per fit), neither epoch has a host decision in it, and both phases go through
``epoch_graph.run_epochs``: ``epochs_per_graph`` (default 4, ``PYGDA_AMD_GRAPH_UNROLL``) epochs per hipGraph replay, the
log read back once per replay; the second phase's capture keeps the optimiser's state instead of starting it fresh.
Eager and captured fits are bit-identical.  ``device='cpu'`` restates the reference's lines in torch (any dtype).

Only full batch (``batch_size=0``) and ``num_positive_samples=2`` are supported; anything else raises
NotImplementedError naming the argument: the reference's mini-batch path concatenates loader batches that include
non-seed rows, and a walk length other than 2 builds a ragged list."""
import time

import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn import SOGABase
from ..nn.host import _host_bottleneck
from .own_epoch import SourceFreeGDA, refuse_data_parallel


class SOGA(SourceFreeGDA):
    def __init__(self, in_dim, hid_dim, num_classes, num_layers=3, dropout=0., act=F.relu, num_negative_samples=5,
                 num_positive_samples=2, struct_lambda=1.0, neigh_lambda=1.0, weight_decay=0., lr=4e-3, epoch=200,
                 gnn='gcn', device='cuda:0', batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        self.record = bool(kwargs.pop("record", False))
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        if batch_size != 0:
            raise NotImplementedError("SOGA: batch_size != 0 is not supported (only full-batch training, batch_size=0)")
        if num_positive_samples != 2:
            raise NotImplementedError("SOGA: num_positive_samples != 2 is not supported (the walks are centre and one "
                                      "positive)")
        self.gnn = gnn
        self.num_negative_samples, self.num_positive_samples = num_negative_samples, num_positive_samples
        self.struct_lambda, self.neigh_lambda = struct_lambda, neigh_lambda
        self.parts_log, self._phase = [], "source"

    def init_model(self, **kwargs):
        return SOGABase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes,
                        num_layers=self.num_layers, dropout=self.dropout, act=self.act, gnn=self.gnn,
                        num_negative_samples=self.num_negative_samples,
                        num_positive_samples=self.num_positive_samples, device=self.device, **kwargs).to(self.device)

    def _check(self, source_data, target_data):
        from ..ops import SOGA_MAX_CLASSES
        refuse_data_parallel(self)
        if torch.device(self.device).type == "cuda" and self.num_classes > SOGA_MAX_CLASSES:
            raise ValueError(f"SOGA: the loss kernels cover up to {SOGA_MAX_CLASSES} classes, got {self.num_classes}")
        self._check_edges(source_data, target_data)
        self._check_labels(source_data.y)

    # -- the network and the two losses on either device ---------------------------------------------------------------
    def _logits(self, x, ei):
        if x.is_cuda:
            return self.soga(x, ei)
        return F.linear(_host_bottleneck(self.soga, x, ei), self.soga.cls.weight, self.soga.cls.bias)

    def ent(self, softmax_output):
        return torch.mean(torch.sum(-softmax_output * torch.log(softmax_output + 1e-5), dim=1))

    def div(self, softmax_output):
        mean = softmax_output.mean(dim=0)
        return torch.sum(-mean * torch.log(mean + 1e-8))

    def NCE_loss(self, outputs, center_nodes, positive_samples, negative_samples):
        """InfoNCE of one view's tables on the probabilities ``outputs [N, C]`` (host composition, any device)."""
        c = outputs[center_nodes.reshape(-1)]
        p = outputs[positive_samples.reshape(-1)]
        n = outputs[negative_samples]
        pos = torch.exp((c * p).sum(-1))
        neg = torch.exp((c.unsqueeze(1) * n).sum(-1)).sum(dim=1)
        return (-torch.log(pos / neg)).mean()

    # -- fit -----------------------------------------------------------------------------------------------------------
    def _plan(self, target_data, dev):
        from ..ops import soga_plan
        views = self.soga.init_target(target_data)
        return soga_plan(views, target_data.x.shape[0], dev)

    def _dom(self, data, dev):
        d = super()._dom(data, dev)
        d.data = data                                      # init_target draws the views' tables from the caller's graph
        return d

    def _init_fit(self, s, t):
        self.soga = self.init_model(**self.kwargs)
        self.parts_log, self._phase = [], "source"
        return self.soga.parameters()

    def _host_fit(self, s, t, optimizer):
        from ..ops import soga_adapt, soga_smooth_ce
        start = time.time()

        def source_epoch(epoch):
            self.soga.train()
            logits = self._logits(s.x, s.edge_index)
            return (soga_smooth_ce(logits, s.y, self.soga.cce.epsilon),
                    lambda: eval_micro_f1(s.y, logits.detach().argmax(dim=1)))

        def target_epoch(epoch):
            self.soga.train()
            loss, parts = soga_adapt(self._logits(t.x, t.edge_index), plan, self.struct_lambda, self.neigh_lambda)
            if self.record:
                self.parts_log.append(parts.tolist())
            return loss, lambda: None

        self._host_epochs(optimizer, source_epoch, start)
        self._phase = "target"
        plan = self._plan(t.data, torch.device(self.device))
        self._host_epochs(optimizer, target_epoch, start)

    def _device_fit(self, s, t):
        """Both phases through epoch_graph.run_epochs.  A pretraining epoch leaves its loss and the loss kernel's count
        of correct arg-maxes in slot ``u``; an adaptation epoch its loss and, beside it, the four loss parts.  The
        second phase hands the optimiser's state to the capture as tensors to keep: it is not a fresh optimiser."""
        from ..epoch_graph import run_epochs
        U, use_graph = self._slots(), self._want_hip_graph()
        run_epochs(self, lambda u: self._source_epoch(s, u), s.n, U, use_graph)
        self._phase = "target"
        plan = self._plan(t.data, torch.device(self.device))
        self._slots(parts=(4,))
        state = [v for st in self.optimizer.state.values() for v in st.values() if torch.is_tensor(v)]

        def record(k):
            if self.record:
                self.parts_log.extend(self._parts_buf[:k].tolist())

        run_epochs(self, lambda u: self._target_epoch(t, plan, u), 1, U, use_graph, after_group=record, also=state)

    def _source_epoch(self, s, u):
        from ..ops import ce_stats_for, soga_smooth_ce
        self.soga.train()
        logits = self.soga(s.x, s.edge_index)
        loss = soga_smooth_ce(logits, s.y, self.soga.cce.epsilon)
        self._step(u, loss, hit=ce_stats_for(logits, s.y)[1])

    def _target_epoch(self, t, plan, u):
        from ..ops import soga_adapt
        self.soga.train()
        loss, parts = soga_adapt(self.soga(t.x, t.edge_index), plan, self.struct_lambda, self.neigh_lambda)
        self._step(u, loss, parts=parts)

    # -- predict -------------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(logits of the network in eval mode, data.y)``."""
        self.soga.eval()
        d = super()._dom(data, torch.device(self.device))
        with torch.no_grad():
            logits = self._logits(d.x, d.edge_index)
        return logits, data.y
