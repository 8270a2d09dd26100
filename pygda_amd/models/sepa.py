"""``SEPA`` trainer (pygda/models/sepa.py): Structure Enhanced Prototypical Alignment (source-needed, node level).

Full batch only: every epoch is one pass of a :class:`~pygda_amd.nn.GNNBase` over both domains and one Adam step on
``lamda_im loss_im + lamda_pp loss_pp + lamda_sep loss_sep + nll``: the information-maximisation term of the target's
softmax, the InfoNCE alignment of the source class prototypes with the target's structure-enhanced ones (biased
centres by arg-max, re-weighted against the class confusion matrix, a personalised PageRank of the correction, the
node's entropy as its step), the separation of the source prototypes, and the source's NLL.  The log's loss is the
epoch's loss before the step; its source micro-F1 comes from ``predict`` in eval mode after it.  ``parts_log`` and
``pred_log`` keep each epoch's four loss parts and the target's arg-max beside the log when ``record=True``.

On the GPU ``fit`` goes through ``ops.sepa_term`` (csrc/gda_sepa.hip: one row pass for softmax / arg-max / entropy,
ordered class-grouped reductions, the C x C stages in single workgroups, the PageRank on the target GCN's cached CSR)
instead of the five loss methods; arg-max, empty classes and the log stay on the device, so ``epochs_per_graph``
(default 4, ``PYGDA_AMD_GRAPH_UNROLL``) epochs are captured into one hipGraph and replayed, the log read back once per
replay.  Eager and captured fits are bit-identical.  With ``dropout == 0`` the source's two encoder passes of the
reference have the same values and are run once (the gradient is their sum).

The five loss methods stay callable on their own on either device; on device tensors their products run on the
project's GEMM / SpMM and the SEPA kernels.  As in the reference, ``self.gnn`` is the backbone's name until ``fit``
replaces it with the network.  ``device='cpu'`` restates the reference's lines in torch (any dtype).
Raised as ValueError before any device work: ``batch_size != 0``, a source class without a labelled node (the
reference divides by its zero count and trains on NaN), and on the GPU ``num_classes`` / ``hid_dim`` beyond
ops.SEPA_MAX_CLASSES / ops.SEPA_MAX_WIDTH."""
import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn import GNNBase
from ..nn.host import _host_bottleneck, _host_conv, _mm
from ..nn.pagerank import PageRank
from ..ops import SEPA_MAX_CLASSES, SEPA_MAX_WIDTH
from .own_epoch import OwnEpochGDA, refuse_data_parallel


class SEPA(OwnEpochGDA):
    _unroll_env = "PYGDA_AMD_GRAPH_UNROLL"

    def __init__(self, in_dim, hid_dim, num_classes, num_layers=2, dropout=0., gnn='gcn', lamda_im=0.2, lamda_pp=0.1,
                 lamda_sep=1.0, tau=1.5, act=F.relu, weight_decay=0.01, lr=0.001, epoch=200, device='cuda:0',
                 batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        self.record = bool(kwargs.pop("record", False))
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        if batch_size != 0:
            raise ValueError("SEPA: only full-batch training (batch_size=0) is supported")
        if torch.device(device).type == "cuda" and (num_classes > SEPA_MAX_CLASSES or hid_dim > SEPA_MAX_WIDTH):
            raise ValueError(f"SEPA: the prototype kernels cover up to {SEPA_MAX_CLASSES} classes and hidden widths up "
                             f"to {SEPA_MAX_WIDTH}, got num_classes={num_classes}, hid_dim={hid_dim}")
        self.gnn = gnn
        self.lamda_im, self.lamda_pp, self.lamda_sep, self.tau = lamda_im, lamda_pp, lamda_sep, tau
        self.pagerank = PageRank()
        self.parts_log, self.pred_log = [], []

    def init_model(self, **kwargs):
        return GNNBase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes,
                       num_layers=self.num_layers, dropout=self.dropout, gnn=self.gnn, **kwargs).to(self.device)

    def process_graph(self, data):
        pass

    def _check(self, source_data, target_data):
        refuse_data_parallel(self)
        counts = torch.bincount(source_data.y.reshape(-1).cpu().long(), minlength=self.num_classes)
        if counts.numel() > self.num_classes:
            raise ValueError(f"SEPA: a source label is outside [0, {self.num_classes})")
        empty = (counts == 0).nonzero().flatten().tolist()
        if empty:
            raise ValueError(f"SEPA: source class {empty[0]} has no labelled node (its prototype would divide by a "
                             "zero count)")
        self._check_edges(source_data, target_data)

    # -- the network on either device ----------------------------------------------------------------------------------
    def _bottleneck(self, x, ei):
        return self.gnn.feat_bottleneck(x, ei) if x.is_cuda else _host_bottleneck(self.gnn, x, ei)

    def _classifier(self, feat, ei):
        return self.gnn.feat_classifier(feat, ei) if feat.is_cuda else _host_conv(self.gnn.cls, feat, ei)

    # -- the five loss methods -----------------------------------------------------------------------------------------
    def cls_im(self, prob):
        """``(loss_im, div_loss, ent_loss, per-node entropies)``; ``div_loss`` is ``sum m log(m + 1e-12)`` of the mean
        probabilities (the negative diversity), the entropies use the same offset."""
        mean_prob = prob.mean(dim=0)
        div_loss = torch.sum(mean_prob * torch.log(mean_prob + 1e-12))
        ent = -torch.sum(prob * torch.log(prob + 1e-12), dim=1)
        ent_loss = torch.mean(ent)
        return div_loss + ent_loss, div_loss, ent_loss, ent

    def obtain_source_prototype(self, feat, label):
        """Class means of the source features ``[num_classes, d]`` (no offset in the count)."""
        from ..ops import sepa_class_mean
        return sepa_class_mean(feat, label, self.num_classes, 0.0)

    def obtain_target_prototype(self, prob, feat, edge_index, ent):
        """The structure-enhanced target prototypes ``[num_classes, d]``; the arg-max carries no gradient, the
        entropies ``ent`` do."""
        from ..ops import sepa_class_mean
        C = self.num_classes
        pred = torch.max(prob, dim=1)[1]
        biased = sepa_class_mean(feat, pred, C, 1e-12)
        onehot = torch.eye(C, dtype=prob.dtype, device=prob.device)[pred]
        count = onehot.sum(dim=0)
        # a class's mean probabilities over the nodes predicted as it; a zero row where nobody is
        if prob.is_cuda:
            matrix = sepa_class_mean(prob, pred, C, 1e-30)           # 0 / 1e-30 = 0 for an empty class
        else:
            matrix = (onehot.t() @ prob) / count.clamp(min=1)[:, None]
        matrix = F.normalize(matrix * (1 - torch.eye(C, dtype=prob.dtype, device=prob.device)), dim=1)
        every = F.normalize(prob * matrix[pred], dim=1)
        own = biased[pred]
        unbiased = _mm(every, biased) / torch.sum(every + 1e-12, dim=1, keepdim=True)
        unbiased = F.normalize(self.pagerank(unbiased - own, edge_index), dim=1)
        per_node = own + ent.unsqueeze(-1) * unbiased
        if per_node.is_cuda:
            return sepa_class_mean(per_node, pred, C, 1e-12)
        return (_mm(per_node.t(), onehot) / (count + 1e-12)).t()

    def seperate_center(self, center, feat=None, label=None):
        """InfoNCE separation of the prototypes among themselves; ``feat`` and ``label`` are ignored, as in the
        reference."""
        if center.is_cuda:
            from ..ops import sepa_separate
            return sepa_separate(center, self.tau)
        C = self.num_classes
        unit = F.normalize(center, dim=1)
        sim = torch.exp(unit @ unit.t() / self.tau)
        away = (sim.sum(dim=1) - sim.diagonal()) / (C - 1)
        return torch.mean(torch.log(away + 1e-8))

    def proto_alignment(self, target_proto, source_proto):
        """InfoNCE of matching target / source prototypes against every other pair inside and across the domains."""
        if target_proto.is_cuda:
            from ..ops import sepa_proto_alignment
            return sepa_proto_alignment(target_proto, source_proto, self.tau)
        t = F.normalize(target_proto + 1e-6, dim=1)
        s = F.normalize(source_proto + 1e-6, dim=1)
        ts, tt, ss = (torch.exp(a @ b.t() / self.tau) for a, b in ((t, s), (t, t), (s, s)))
        pos = ts.diagonal()
        den = ts.sum(dim=1) - pos + tt.sum(dim=1) - tt.diagonal() + ss.sum(dim=1) - ss.diagonal()
        logit = pos / den.clamp(min=1e-6)
        return -torch.log(logit.clamp(min=1e-6)).mean()

    # -- one epoch's loss ----------------------------------------------------------------------------------------------
    def forward_model(self, source_data, target_data):
        """``(loss, source_logits, target_logits)``: the source's log-probabilities and the target's raw classifier
        output.  Host tensors take the reference's lines through the five methods; device tensors the fused term."""
        sx, sei, sy = source_data.x, source_data.edge_index, source_data.y
        tx, tei = target_data.x, target_data.edge_index
        source_feat = self._bottleneck(sx, sei)
        target_feat = self._bottleneck(tx, tei)
        target_cls = self._classifier(target_feat, tei)
        if tx.is_cuda:
            from ..graph import as_graph
            from ..ops import sepa_term, source_ce
            y32 = getattr(source_data, "y32", None)
            if y32 is None:
                y32 = sy.to(torch.int32)
            graph = as_graph(tei, tx.size(0), None, False, True, True, "col")
            term, parts, pred = sepa_term(target_cls, target_feat, source_feat, y32, graph, self.lamda_im,
                                          self.lamda_pp, self.lamda_sep, self.tau, self.pagerank.k, self.pagerank.alpha)
            source_cls = self._classifier(source_feat if self.dropout == 0 else self._bottleneck(sx, sei), sei)
            nll = source_ce(source_cls, sy)
            self._parts = torch.cat([parts, nll.detach().reshape(1)])
            self._pred = pred
            return term + nll, source_cls, target_cls
        target_prob = F.softmax(target_cls, dim=1)
        loss_im, _, _, ent = self.cls_im(target_prob)
        source_proto = self.obtain_source_prototype(source_feat, sy)
        target_proto = self.obtain_target_prototype(target_prob, target_feat, tei, ent)
        loss_pp = self.proto_alignment(target_proto, source_proto)
        loss_sep = self.seperate_center(source_proto, source_feat, sy)
        output = F.log_softmax(self._classifier(self._bottleneck(sx, sei), sei), dim=1)
        nll = F.nll_loss(output, sy)
        self._parts = torch.stack([loss_im, loss_pp, loss_sep, nll]).detach()
        self._pred = torch.max(target_prob, dim=1)[1]
        return self.lamda_im * loss_im + self.lamda_pp * loss_pp + self.lamda_sep * loss_sep + nll, output, target_cls

    # -- fit -----------------------------------------------------------------------------------------------------------
    def _dom(self, data, dev):
        d = super()._dom(data, dev)
        d.y32 = d.y.to(torch.int32)
        return d

    def _init_fit(self, s, t):
        self.gnn = self.init_model(**self.kwargs)          # replaces the backbone's name, as in the reference
        self.parts_log, self.pred_log = [], []
        return self.gnn.parameters()

    def _host_epoch(self, s, t, epoch):
        self.gnn.train()
        loss, _, _ = self.forward_model(s, t)
        if self.record:
            self.parts_log.append(self._parts.tolist())
            self.pred_log.append(self._pred.clone())
        return loss, lambda: eval_micro_f1(s.y, self.predict(s)[0].argmax(dim=1))

    def _device_fit(self, s, t):
        """Epochs on the device (epoch_graph.run_epochs).  Epoch ``u`` of a replay writes its loss, its four parts, its
        count of correct source predictions (``predict`` after the step) and, when recording, the target's arg-max
        into slot ``u`` of small buffers that are read once per replay."""
        from ..epoch_graph import run_epochs
        U = self._slots(parts=(4,))
        self._slots(torch.int32, pred=(t.n if self.record else 0,))

        def record(k):
            if self.record:
                self.parts_log.extend(self._parts_buf[:k].tolist())
                self.pred_log.extend(self._pred_buf[:k].long().cpu().unbind(0))

        run_epochs(self, lambda u: self._device_epoch(s, t, u), s.n, U, self._want_hip_graph(),
                   after_group=record)

    def _device_epoch(self, s, t, u):
        self.gnn.train()
        loss, _, _ = self.forward_model(s, t)
        self._step(u, loss, parts=self._parts, **(dict(pred=self._pred) if self.record else {}))
        self.gnn.eval()
        with torch.no_grad():
            logits = self.gnn(s.x, s.edge_index)
            self._hit_buf[u].copy_((logits.argmax(dim=1) == s.y).sum())

    # -- predict -------------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(log-probabilities of the network in eval mode, data.y)``."""
        self.gnn.eval()
        d = super()._dom(data, torch.device(self.device))
        x, ei = d.x, d.edge_index
        with torch.no_grad():
            if x.is_cuda:
                logits = self.gnn(x, ei)
            else:
                logits = F.log_softmax(_host_conv(self.gnn.cls, _host_bottleneck(self.gnn, x, ei), ei), dim=1)
        return logits, data.y
