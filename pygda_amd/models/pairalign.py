"""``PairAlign`` trainer (pygda/models/pa.py, "Pairwise Alignment Improves Graph Domain Adaptation", ICML-24): a
``ReweightGNN`` trained on the source with a class-weighted cross-entropy, whose source edges are re-weighted every
``ew_freq`` epochs by a least-squares fit over the ``C^2`` ordered class pairs and whose loss is re-weighted every
``lw_freq`` epochs by a least-squares fit over the ``C`` classes.

Full batch (``batch_size=0``), node mode, backbones ``GS`` / ``GCN``, pooling ``mean`` / ``add``; anything else raises
``NotImplementedError`` before any device work, and so do data-parallel runs and, on the GPU, more than
``ops.PA_MAX_CLASSES`` classes.

What the reference does with ``[E, C, C]``, ``[E, C^2]``, ``[E, N]`` and ``[N, N]`` host arrays is here
- two ``bincount``s at setup (``true_ew`` / ``true_lw`` / ``true_beta``, with the reference's ``inf -> 1``, ``nan -> 1`` and
  the orientation ``to_dense_adj(...).squeeze().T`` gives ``true_ew`` on a directed edge),
- ops.pa_edge_stats (the class-pair outer-product sums ``C_hat`` and ``muhat_tgt``) and ops.pa_softmax_sums (``cov_mat``
  and ``yhat_tgt``) at a re-weighting, one small device-to-host copy, :func:`pygda_amd.qp.solve_simplex_ls`,
  ``calc_ratio_weight`` in float64 numpy as written, one upload, ops.pa_refresh of the CSR values in place,
- ops.pa_ce for all four loss variants: ``coef = 1`` (``CE_loss``), ``1 / p_y`` (``CE_srcweight_loss``),
  ``lw / (p_y * class_num)`` (``CE_loss_weight`` with ``weight_src``) and the constant ``mean(lw[y]) / class_num``
  (``CE_loss_weight`` without it: the reference's ``nn.CrossEntropyLoss()`` there has the default mean reduction, so its
  "per-row" loss is a scalar and the result is ``mean(ce) * mean(lw[y]) / class_num`` -- kept as the reference's
  behaviour).  ``p_y`` is over the masked labels, ``class_num = len(label.unique())``.

SOLVER.  cvxpy / SCS stop at about 1e-4 relative accuracy; ``solve_simplex_ls`` returns the exact optimum of the same
strictly convex program, which is what SCS approximates.  This trainer therefore matches the reference up to the
reference's own solver tolerance, not beyond it.

SCHEDULE.  A reference epoch runs the network five times (two forwards before the step, two after it, one in
``predict``).  At dropout 0 the source forward after the step of epoch ``e`` -- with the weights ``update_ew`` may just
have written, which is what ``predict`` sees -- is the forward before the step of epoch ``e + 1``, and the target forward
is read only where a re-weighting fires and for ``y_hat``.  So an epoch here is one source forward, one backward and one
Adam step; the log's accuracy (over ALL source nodes, as ``predict`` gives it) is the ``stats`` of the next epoch's loss
kernel, and only a re-weighting epoch and the last one pay further forwards.  ``update_lw`` runs only where its result is
stored (``(epoch + 1) >= lw_start and (epoch + 1) % lw_freq == 0``): it has no other effect.  At dropout above 0 the
reference draws masks in ``predict`` as well (``F.dropout`` without ``training=``); that is kept, the masks come from the
project's stream (a forward outside an epoch opens a new step of it, so eager and captured fits draw the same masks),
and parity is in distribution only.

CAPTURE.  The epochs between two re-weightings replay as hipGraphs, ``epochs_per_graph`` at a time; a replay never spans
a re-weighting.  The loss kernel reads ``coef`` and the aggregation reads the CSR values from device buffers that a
re-weighting updates in place, so nothing is captured again.  Captured and eager fits are bit-identical.

``ew_type='truth'`` and the ratio mode hit a ``NameError`` in the reference (``src_graph`` in ``update_ew``); they are
implemented with ``src_data``, as plainly meant.

PERSISTENCE (unverified).  The weights ``update_ew`` and the ``lw`` assignment write persist from epoch to epoch here,
which is what the method intends and what the reference does on a loader that yields the very ``Data`` object in full
batch.  PyG's real ``NeighborLoader`` hands out a fresh batch object each epoch, on which those assignments may well be
lost; PyG was not available to check this against, so that is a supposition.

Set on ``source_data``: ``true_ew`` / ``ew`` (float64 ``[C, C]``), ``true_lw`` (float32 ``[C]``), ``lw`` (float32 ones,
float64 once fitted), ``true_beta`` (float64 ``[C^2]``), ``edge_weight`` (ones where it was ``None``, then
``ew[y_i, y_j]`` per edge, fp32); on ``target_data``: ``edge_weight`` and ``y_hat``.  A ``source_data`` without a
``train_mask`` is trained on all its rows."""
import time

import numpy as np
import torch
import torch.nn.functional as F

from ..nn.reweight_gnn import HostEdges, ReweightGNN
from ..qp import solve_simplex_ls
from .own_epoch import OwnEpochGDA, refuse_data_parallel


def ratio_weight(p_eij_src, kmm_weight, gamma_reg, num_classes):
    """``calc_ratio_weight`` (pa.py:895-908) as written: ``(gamma, p_ei_tgt_reg)``."""
    p_eij_tgt = p_eij_src * kmm_weight.reshape(-1)
    p_eij_src_reg = p_eij_src + gamma_reg
    p_eij_tgt_reg = p_eij_tgt + gamma_reg
    p_ei_src_reg = np.sum(p_eij_src_reg.reshape(num_classes, num_classes), axis=1)
    p_ei_tgt_reg = np.sum(p_eij_tgt_reg.reshape(num_classes, num_classes), axis=1)
    gamma = ((p_eij_tgt_reg.reshape(num_classes, num_classes).T / p_ei_tgt_reg).T) / \
            ((p_eij_src_reg.reshape(num_classes, num_classes).T / p_ei_src_reg).T)
    return gamma, p_ei_tgt_reg


class PairAlign(OwnEpochGDA):
    def __init__(self, in_dim, hid_dim, num_classes, num_layers=2, cls_dim=128, cls_layers=2, dropout=0.,
                 backbone='GS', pooling='mean', ew_type='pseudobeta', rw_lmda=1.0, ls_lambda=1.0, lw_lambda=0.005,
                 label_rw=False, edge_rw=False, ew_start=0, ew_freq=10, lw_start=0, lw_freq=10, gamma_reg=1e-4,
                 weight_CE_src=False, bn=False, act=F.relu, weight_decay=0.0001, lr=0.001, epoch=200, device='cuda:0',
                 batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        self.rw_lmda, self.cls_dim, self.cls_layers, self.backbone, self.pooling = rw_lmda, cls_dim, cls_layers, backbone, pooling
        self.bn, self.label_rw, self.weight_CE_src, self.gamma_reg, self.edge_rw = bn, label_rw, weight_CE_src, gamma_reg, edge_rw
        self.ew_start, self.ew_freq, self.ew_type, self.ls_lambda = ew_start, ew_freq, ew_type, ls_lambda
        self.lw_lambda, self.lw_freq, self.lw_start = lw_lambda, lw_freq, lw_start
        self.solves = []             # tests: (kind, cov, m, mu, lam, x) of every program solved, in order
        self._lw_every_epoch = False  # tests: solve the label program at every epoch, as the reference does

    def init_model(self, **kwargs):
        return ReweightGNN(input_dim=self.in_dim, gnn_dim=self.hid_dim, output_dim=self.num_classes,
                           cls_dim=self.cls_dim, gnn_layers=self.num_layers, cls_layers=self.cls_layers,
                           backbone=self.backbone, pooling=self.pooling, dropout=self.dropout, bn=self.bn,
                           rw_lmda=self.rw_lmda, **kwargs).to(self.device)

    def forward_model(self, source_data, target_data, epoch):
        pass

    def process_graph(self, data):
        pass

    # -- checks and setup --------------------------------------------------------------------------------------------
    def _check(self, source_data, target_data):
        refuse_data_parallel(self)
        if self.batch_size != 0:
            raise NotImplementedError("PairAlign: only full-batch training (batch_size=0): the reference's own "
                                      "src_edge_class is full-graph and would mis-index a sampled batch")
        if self.backbone not in ("GS", "GCN"):
            raise NotImplementedError(f"PairAlign: backbone {self.backbone!r} is not covered (GS, GCN)")
        if self.pooling not in ("mean", "add"):
            raise NotImplementedError(f"PairAlign: pooling {self.pooling!r} is not covered (mean, add)")
        if torch.device(self.device).type == "cuda":
            from ..ops import PA_MAX_CLASSES
            if self.num_classes > PA_MAX_CLASSES:
                raise NotImplementedError(f"PairAlign: the statistic kernels cover up to {PA_MAX_CLASSES} classes, "
                                          f"got {self.num_classes}")
        self._check_edges(source_data, target_data)
        self._check_labels(source_data.y)
        self._check_labels(target_data.y)

    def fit(self, source_data, target_data):
        self._src_data, self._tgt_data = source_data, target_data
        super().fit(source_data, target_data)

    def _dom(self, data, dev):
        d = super()._dom(data, dev)
        mask = getattr(data, "train_mask", None)
        d.sel = None if mask is None else torch.nonzero(mask.to(dev).bool()).view(-1).contiguous()
        w = getattr(data, "edge_weight", None)
        d.edge_weight = torch.ones(d.edge_index.size(1), device=dev) if w is None else w.to(dev)
        data.edge_weight = d.edge_weight
        return d

    def _graph(self, d):
        """(Re)build what ``ReweightGNN.forward_on`` aggregates ``d`` on, from ``d.edge_weight``."""
        flags = self.gnn.prop_input.graph_flags()
        if d.x.is_cuda:
            from ..ops import PaGraph
            d.pg = PaGraph(d.edge_index, d.n, d.edge_weight, self.rw_lmda, *flags)
            d.g = d.pg.graph
        else:
            d.g = HostEdges(d.edge_index, d.edge_weight.to(d.x.dtype), self.rw_lmda, d.n, *flags)

    def _init_fit(self, s, t):
        C, src = self.num_classes, self._src_data
        self.num_source_nodes, self.num_target_nodes = s.n, t.n
        self._s, self._t = s, t

        def pairs(d):
            return torch.bincount(d.y[d.edge_index[0]] * C + d.y[d.edge_index[1]], minlength=C * C).cpu().numpy()

        def nodes(d):
            return torch.bincount(d.y, minlength=C).cpu().numpy()

        cnt_s, cnt_t, n_s, n_t = pairs(s), pairs(t), nodes(s), nodes(t)
        self._E_s, self._E_t = int(s.edge_index.size(1)), int(t.edge_index.size(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            # cal_edge_prob_sep: (onehot.T adj.T onehot)[a, b] = #edges j -> i with j in b, i in a; rows by n_a * N
            prob_s = cnt_s.reshape(C, C).T.astype(np.float64) / (n_s.astype(np.float64) * s.n).reshape(C, 1)
            prob_t = cnt_t.reshape(C, C).T.astype(np.float64) / (n_t.astype(np.float64) * t.n).reshape(C, 1)
            src.true_ew = (prob_t + self.gamma_reg) / (prob_s + self.gamma_reg)
            src.ew = np.ones_like(src.true_ew)
            # calc_true_lw: integer counts / int -> float32 in torch
            src.true_lw = ((n_t.astype(np.float32) / np.float32(t.n)) / (n_s.astype(np.float32) / np.float32(s.n)))
            src.lw = np.ones_like(src.true_lw)
            self._p_eij_src = cnt_s.astype(np.float64) / self._E_s
            beta = (cnt_t.astype(np.float64) / self._E_t) / self._p_eij_src
            beta[beta == float('inf')] = 1
            src.true_beta = np.nan_to_num(beta, nan=1)
        # what the reference's float32 means of 0/1 columns give (exact sums, one rounding)
        self._mu_edge = (cnt_s.astype(np.float32) / np.float32(self._E_s)).astype(np.float64)
        self._mu_label = (n_s.astype(np.float32) / np.float32(s.n)).astype(np.float64)
        y_sel = s.y if s.sel is None else s.y[s.sel]
        self._n_sel = int(y_sel.numel())
        if self._n_sel == 0:
            raise ValueError("PairAlign: the source train_mask selects no row")
        self._mask_cnt = torch.bincount(y_sel, minlength=C).cpu().numpy()
        self._class_num = int((self._mask_cnt > 0).sum())
        self.gnn = self.init_model(**self.kwargs).to(s.x.dtype)
        self._coef = torch.ones(C, dtype=torch.float32, device=s.x.device)
        self._set_coef()
        self._graph(s)
        self._graph(t)
        if s.x.is_cuda:
            from ..ops import PaEdgePlan, PaSoftPlan
            self._edge_plan_s = PaEdgePlan(s.edge_index, s.n, s.y, C)
            self._edge_plan_t = PaEdgePlan(t.edge_index, t.n, None, 1)
            self._soft_plan = PaSoftPlan(s.n, s.y, C, t.n, None, 1, s.x.device)
            self._rw_dev = torch.ones(C, C, dtype=torch.float32, device=s.x.device)
        return list(self.gnn.parameters())

    # -- the loss ----------------------------------------------------------------------------------------------------
    def _set_coef(self):
        """The class coefficients of the loss (module docstring) from ``source_data.lw``, in float32 as the reference
        forms them, written into the device vector in place."""
        C, cnt = self.num_classes, self._mask_cnt.astype(np.float32)
        with np.errstate(divide="ignore"):
            cw = np.float32(1.0) / (cnt / np.float32(self._n_sel))
        lw = np.asarray(self._src_data.lw).astype(np.float32)
        if self.label_rw and self.weight_CE_src:
            coef = cw * lw / np.float32(self._class_num)
        elif self.label_rw:
            coef = np.full(C, np.float32((cnt * lw).sum() / np.float32(self._n_sel)) / np.float32(self._class_num))
        elif self.weight_CE_src:
            coef = cw
        else:
            coef = np.ones(C, dtype=np.float32)
        coef = np.where(cnt > 0, coef, np.float32(0)).astype(np.float32)      # a class no masked row has is never read
        self._coef.copy_(torch.from_numpy(coef))

    def _loss(self, logits, stats=None):
        from ..ops import pa_ce
        s = self._s
        return pa_ce(logits, s.y, self._coef.to(logits.dtype) if not logits.is_cuda else self._coef, s.sel, stats)

    def _forward(self, d):
        return self.gnn.forward_on(d.g, d.x)[1]

    def _fresh_masks(self):
        """Ahead of forwards that are not an epoch's own: a new step of the dropout stream, so that their masks are a
        function of the step counter alone and not of how many launches the host numbered before (a replayed epoch
        numbers none)."""
        if self.dropout > 0 and torch.device(self.device).type == "cuda":
            from ..ops import dropout_state
            dropout_state.next_step(torch.device(self.device))

    # -- the two re-weightings ---------------------------------------------------------------------------------------
    def _fires(self, epoch):
        """``(edge weights move, label weights are stored)`` after the step of ``epoch``."""
        return (bool(self.edge_rw) and (epoch + 1) >= self.ew_start and (epoch + 1) % self.ew_freq == 0,
                (epoch + 1) >= self.lw_start and (epoch + 1) % self.lw_freq == 0)

    def _solve(self, kind, cov, m, mu, lam):
        x = solve_simplex_ls(cov, m, mu, lam)
        self.solves.append((kind, cov, m, mu, float(lam), x))
        return x

    def _edge_stats(self, pred_src, pred_tgt):
        """``(C_hat [C^2, C^2], muhat_tgt [C^2])`` of calc_edge_rw_pseudo, float64 numpy."""
        C, s, t = self.num_classes, self._s, self._t
        if pred_src.is_cuda:
            from ..ops import pa_edge_stats
            S_s, S_t = pa_edge_stats(pred_src, self._edge_plan_s), pa_edge_stats(pred_tgt, self._edge_plan_t)
        else:
            from ..ops import _pa_edge_stats_host
            S_s = _pa_edge_stats_host(pred_src, s.edge_index, s.y, C)
            S_t = _pa_edge_stats_host(pred_tgt, t.edge_index, None, 1)
        both = torch.cat([S_s.permute(1, 3, 0, 2).reshape(-1), S_t.reshape(-1)]).cpu().numpy()     # one copy
        return both[:C ** 4].reshape(C * C, C * C) / self._E_s, both[C ** 4:] / self._E_t

    def update_ew(self, pred_src, pred_tgt):
        """``update_ew`` (pa.py:678-721): the class-pair table ``ew`` and the per-edge weights it gives."""
        C, src = self.num_classes, self._src_data
        if self.ew_type == "pseudobeta":
            C_hat, muhat = self._edge_stats(pred_src.detach(), pred_tgt.detach())
            w = self._solve("edge", C_hat, muhat, self._mu_edge, self.ls_lambda).reshape(C, C)
            with np.errstate(divide="ignore", invalid="ignore"):
                edge_rw, _ = ratio_weight(self._p_eij_src, w, self.gamma_reg, C)
            edge_rw[edge_rw == float('inf')] = 1
            edge_rw = np.nan_to_num(edge_rw, nan=1)
        elif self.ew_type == "truth":
            edge_rw = src.true_ew
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                edge_rw, _ = ratio_weight(self._p_eij_src, src.true_beta, self.gamma_reg, C)
        self._set_edge_weight(edge_rw)

    def _set_edge_weight(self, edge_rw):
        s, C, src = self._s, self.num_classes, self._src_data
        table = torch.from_numpy(np.ascontiguousarray(edge_rw, dtype=np.float64)).float()
        if s.x.is_cuda:
            from ..ops import pa_refresh
            self._rw_dev.copy_(table)
            pa_refresh(s.pg, s.y, self._rw_dev)
            table = self._rw_dev
        s.edge_weight = table.reshape(-1)[s.y[s.edge_index[0]] * C + s.y[s.edge_index[1]]]
        if not s.x.is_cuda:
            self._graph(s)
        src.edge_weight, src.ew = s.edge_weight, edge_rw

    def update_lw(self, pred_src, pred_tgt):
        """``update_lw`` (pa.py:910-945): the label weights, float64 ``[C]``."""
        C, s, t = self.num_classes, self._s, self._t
        if pred_src.is_cuda:
            from ..ops import pa_softmax_sums
            P_s, P_t = pa_softmax_sums(pred_src, pred_tgt, self._soft_plan)
        else:
            from ..ops import _pa_softmax_sums_host
            P_s = _pa_softmax_sums_host(pred_src, s.y, C)
            P_t = _pa_softmax_sums_host(pred_tgt, None, 1)
        both = torch.cat([P_s.t().reshape(-1), P_t.reshape(-1)]).cpu().numpy()                    # one copy
        return self._solve("label", both[:C * C].reshape(C, C) / s.n, both[C * C:] / t.n, self._mu_label, self.lw_lambda)

    def _reweight(self, epoch, pred_src, pred_tgt):
        """What follows the step of ``epoch`` in forward_model (pa.py:260-270), given the forwards after the step."""
        fire_ew, fire_lw = self._fires(epoch)
        self._tgt_data.y_hat = pred_tgt.detach().argmax(dim=1)
        if fire_ew:
            self.update_ew(pred_src, pred_tgt)
        if fire_lw or self._lw_every_epoch:
            lw = self.update_lw(pred_src.detach(), pred_tgt.detach())
            if fire_lw:
                self._src_data.lw = lw
                self._set_coef()
        return fire_ew

    def _after_step(self, epoch):
        """The forwards after the step of ``epoch`` and what reads them; returns the source logits ``predict`` would
        give (the log's accuracy) where they were computed anyway, else None."""
        self._fresh_masks()
        with torch.no_grad():
            pred_src, pred_tgt = self._forward(self._s), self._forward(self._t)
            moved = self._reweight(epoch, pred_src, pred_tgt)
        return None if moved else pred_src

    def _is_event(self, epoch):
        return any(self._fires(epoch)) or self._lw_every_epoch or epoch == self.epoch - 1

    def _final_accuracy(self, logits):
        s = self._s
        if logits is None:
            self._fresh_masks()
            with torch.no_grad():
                logits = self._forward(s)
        return float((logits.argmax(dim=1) == s.y).sum()) / s.n

    # -- host path ---------------------------------------------------------------------------------------------------
    def _host_fit(self, s, t, optimizer):
        start, pending, logits = time.time(), None, None
        for epoch in range(self.epoch):
            self.gnn.train()
            logits = self._forward(s)
            if pending is not None:
                self._report(epoch - 1, pending, float((logits.detach().argmax(dim=1) == s.y).sum()) / s.n, start)
            loss = self._loss(logits)
            pending = loss.item()
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            logits = self._after_step(epoch) if self._is_event(epoch) else None
        if pending is not None:
            self._report(self.epoch - 1, pending, self._final_accuracy(logits), start)

    # -- device path -------------------------------------------------------------------------------------------------
    def _device_epoch(self, u):
        from ..ops import dropout_state
        dropout_state.next_step(torch.device(self.device))
        self.gnn.train()
        loss = self._loss(self._forward(self._s), self._stats_buf[u])
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()

    def _device_fit(self, s, t):
        from ..epoch_graph import capture_rolled_back
        from ..ops import dropout_state
        dev = torch.device(self.device)
        U = self._slots(torch.float64, stats=(2,))
        use_graph, graph = self._want_hip_graph() and self.epoch >= U, None
        start, pending, logits, epoch = time.time(), None, None, 0
        while epoch < self.epoch:
            nxt = next(e for e in range(epoch, self.epoch) if self._is_event(e))
            while epoch <= nxt:
                k = U if use_graph and nxt - epoch + 1 >= U else 1
                if use_graph and k == U:
                    if graph is None:
                        params = [p for g in self.optimizer.param_groups for p in g["params"]]
                        graph = capture_rolled_back(self._device_epoch, U, params, [self.optimizer],
                                                    [dropout_state.counter(dev)])
                    graph.replay()
                else:
                    self._device_epoch(0)
                for u, (loss, hits) in enumerate(self._stats_buf[:k].tolist()):
                    if pending is not None:
                        self._report(epoch + u - 1, pending, hits / s.n, start)
                    pending = loss
                epoch += k
            logits = self._after_step(nxt)
        if pending is not None:
            self._report(self.epoch - 1, pending, self._final_accuracy(logits), start)

    # -- predict -----------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(logits, data.y)`` of the network on ``data`` with its ``edge_weight`` (pa.py:384-413).  The layers'
        dropout stays on, as in the reference (``F.dropout`` without ``training=``)."""
        self.gnn.eval()
        self._fresh_masks()
        with torch.no_grad():
            for mine, d in ((getattr(self, "_src_data", None), getattr(self, "_s", None)),
                            (getattr(self, "_tgt_data", None), getattr(self, "_t", None))):
                if data is mine and d is not None:
                    return self._forward(d), data.y
            d = self._dom(data, torch.device(self.device))
            d.x = d.x.to(next(self.gnn.parameters()).dtype)
            self._graph(d)
            return self._forward(d), data.y
