"""``GraphCTA`` trainer (pygda/models/graphcta.py): Collaborate to Adapt -- source-free graph domain adaptation via
bi-directional adaptation (node level).

The fit is :class:`~pygda_amd.models.graph_transform.GraphTransformGDA`'s -- pretraining, the feature perturbation and
the flip weights, why the flip weights do not move by default, ``loop_adj > 1`` and the final sampling (on ``data.x``,
not on the perturbed features) are explained there.  What is GraphCTA's own, per iteration:

* ``loop_model`` MODEL steps ahead of the others: a train-mode forward on the current features and edge weights, the
  prototypes of the feature memory per arg-max class of that forward, the pseudo label of every node from the unweighted
  in-neighbour mean of the class memory, ``ops.cta_model_loss`` (instance-prototype contrast and the similarity-weighted
  cross-entropy), an Adam step of the network (the pretraining optimiser, moments carried over; both perturbations are
  a further parameter group of it), then an eval-mode forward whose bottleneck output and sharpened softmax move the two
  memory banks by ``momentum``;
* ``test_time_loss`` through the frozen network in eval mode: the cross-entropy of the low-entropy share of every
  predicted class against its own prediction, minus the inner product with the ``K`` nearest memory rows, plus the inner
  product with the memory rows of the other classes (``ops.cta_knn``, ``ops.cta_test_time_loss``).

``predict`` ignores its argument's graph and returns the eval-mode log-probabilities on the stored ``new_feat``,
``edge_index``, ``edge_weight`` beside ``data.y``.

On the GPU the three losses are the kernels of csrc/gda_graphcta.hip, which store no ``[N, N]`` array.  The layer-0
projection of the features is taken once per iteration, after the model steps; a feature step adds ``delta_feat W0^T``.

As they are in the reference: ``mem_fea = torch.rand(N, hid)`` is drawn from torch's CPU generator after ``init_model``
and ``mem_cls = 1 / C``; the neighbour mean is structural and unweighted -- over the target's edge list as given, with
multiplicity, until the first structure step has coalesced it, and over the coalesced list (with the reverse pairs that
``make_undirected`` adds at weight 1e-7) from then on; the row that ``idx_near`` drops is rank 1, whichever it is.

Private keywords beside the shared ``record`` and ``step_structure``: recording also keeps every model step's ``[loss,
loss_local, cl]`` in ``model_log`` with its pseudo labels in ``pred_log``, and beside every ``test_time_loss`` call's
``[loss, ce, nb, ng]`` its ``[pred, selected, the K neighbours]`` in ``choice_log``."""
import time

import torch
import torch.nn.functional as F

from ..ops import first_argmax as _first_argmax
from .graph_transform import GraphTransformGDA


class GraphCTA(GraphTransformGDA):
    _net_name = "graphcta"

    def __init__(self, in_dim, hid_dim, num_classes, num_layers=3, dropout=0., act=F.relu, loop_model=3, loop_adj=1,
                 loop_feat=4, ratio=0.1, K=5, tau=0.2, lamb=0.2, momentum=0.9, make_undirected=True, weight_decay=0.,
                 lr=1e-4, epoch=500, gnn='gcn', device='cuda:0', batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, gnn=gnn, loop_adj=loop_adj,
                         loop_feat=loop_feat, ratio=ratio, make_undirected=make_undirected, **kwargs)
        if loop_model < 0:
            raise ValueError("GraphCTA: loop_model must not be negative")
        if K < 1:
            raise ValueError("GraphCTA: K must be at least 1")
        self.loop_model, self.tau, self.lamb, self.momentum, self.K = loop_model, tau, lamb, momentum, K

    def _reset_logs(self):
        super()._reset_logs()
        self.model_log, self.pred_log, self.choice_log = [], [], []

    def _check_limits(self, n, on_gpu):
        from ..ops import CTA_MAX_CLASSES, CTA_MAX_K1, WGCN_MAX_WIDTH
        if n < self.K + 1:
            raise ValueError(f"GraphCTA: K + 1 = {self.K + 1} neighbours need as many target nodes, got {n}")
        if on_gpu and (self.hid_dim > WGCN_MAX_WIDTH or self.num_classes > CTA_MAX_CLASSES or self.K + 1 > CTA_MAX_K1):
            raise ValueError(f"GraphCTA: the kernels cover hidden widths up to {WGCN_MAX_WIDTH}, {CTA_MAX_CLASSES} "
                             f"classes and K up to {CTA_MAX_K1 - 1}, got {self.hid_dim}, {self.num_classes}, {self.K}")

    def _fit_bytes(self, n, f, nnz, m):
        from ..ops import graphcta_bytes
        return graphcta_bytes(n, f, nnz, m, self.hid_dim, self.num_classes, self.K)

    def _init_fit(self, s, t):
        params = super()._init_fit(s, t)
        # the reference draws the feature memory on the host, after init_model and before anything else
        self._mem0 = torch.rand(t.n, self.hid_dim)
        return params

    # -- what both devices share ---------------------------------------------------------------------------------------
    @staticmethod
    def _neighprop(x, edge_index):
        """``SimpleConv(aggr='mean')``: per node the mean of ``x`` over its listed in-edges' sources (0 without one)."""
        src, dst = edge_index[0], edge_index[1]
        n = x.size(0)
        cnt = torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(0, dst, torch.ones(dst.numel(), dtype=x.dtype,
                                                                                         device=x.device))
        return torch.zeros_like(x).index_add_(0, dst, x[src]) / cnt.clamp(min=1)[:, None]

    def _prototypes(self, mem_fea, cls_output):
        from ..ops import cta_prototypes
        return cta_prototypes(mem_fea, _first_argmax(cls_output.detach()), self.num_classes)

    def _memory_update(self, mem_fea, mem_cls, feat_output, cls_output):
        from ..ops import colsum
        softmax_out = F.softmax(cls_output, dim=1)
        sq = softmax_out ** 2
        outputs_target = sq / (colsum(sq) if sq.is_cuda else sq.sum(dim=0))
        mem_cls.copy_((1.0 - self.momentum) * mem_cls + self.momentum * outputs_target)
        mem_fea.copy_((1.0 - self.momentum) * mem_fea + self.momentum * feat_output)

    def test_time_loss(self, feat, edge_index, edge_weight, mem_fea, mem_cls):
        """The reference's ``test_time_loss`` in eval mode: ``(loss, [loss, ce, nb, ng], [pred, selected, neighbours])``."""
        from ..ops import cta_knn, cta_test_time_loss
        self.graphcta.eval()
        feat_output, cls_output = self._forward(feat, edge_index, edge_weight)
        idx_near, _ = cta_knn(feat_output.detach(), mem_fea, self.K + 1)
        loss, parts, pred, sel = cta_test_time_loss(cls_output, feat_output, mem_fea, mem_cls, idx_near)
        return loss, parts, self._choices(pred, sel, idx_near)

    @staticmethod
    def _choices(pred, sel, idx_near):
        return torch.cat([pred[None].long(), sel[None].long(), idx_near[:, 1:].t().long()]).detach()

    def _logged_loss(self, feat, edge_index, edge_weight, mem_fea, mem_cls):
        loss, parts, choices = self.test_time_loss(feat, edge_index, edge_weight, mem_fea, mem_cls)
        if self.record:
            self.parts_log.append(parts.tolist())
            self.choice_log.append(choices.cpu())
        return loss

    def sample_final_edges(self, n_perturbations, perturbed_edge_weight, t, modified_edge_index, mem_fea, mem_cls):
        return self._sample_final_edges(
            n_perturbations, perturbed_edge_weight, t, modified_edge_index,
            lambda i, feat, edge_index, edge_weight: self._logged_loss(feat, edge_index, edge_weight, mem_fea, mem_cls))

    # -- the host fit: the reference's lines ---------------------------------------------------------------------------
    def _host_fit(self, s, t, optimizer):
        from ..ops import cta_model_loss
        start = time.time()
        net = self.graphcta
        st = self._host_state(t)
        mem_fea = self._mem0.to(t.x.dtype)
        mem_cls = torch.ones(t.n, self.num_classes, dtype=t.x.dtype) / self.num_classes
        self._host_pretrain(s, optimizer, start)
        loss_of = lambda feat: self._logged_loss(feat, st.edge_index, st.edge_weight, mem_fea, mem_cls)   # noqa: E731
        loss = None
        for it in range(st.iters):
            for _ in range(self.loop_model):
                self._freeze(False)
                net.train()
                st.feat, st.edge_weight = st.feat.detach(), st.edge_weight.detach()
                optimizer.zero_grad()
                feat_output, cls_output = self._forward(st.feat, st.edge_index, st.edge_weight)
                proto = self._prototypes(mem_fea, cls_output)
                pred = _first_argmax(self._neighprop(mem_cls, st.edge_index))
                loss, parts = cta_model_loss(feat_output, cls_output, proto, pred, self.tau, self.lamb)
                loss.backward()
                optimizer.step()
                if self.record:
                    self.model_log.append(parts.tolist())
                    self.pred_log.append(pred.clone())
                net.eval()
                with torch.no_grad():
                    feat_output, cls_output = self._forward(st.feat, st.edge_index, st.edge_weight)
                    mem_fea, mem_cls = mem_fea.clone(), mem_cls.clone()
                    self._memory_update(mem_fea, mem_cls, feat_output, cls_output)
            self._freeze()
            st.p = st.p.detach()
            for _ in range(self.loop_feat):
                st.optimizer_feat.zero_grad()
                loss = loss_of(t.x + st.delta_feat)
                loss.backward()
                st.optimizer_feat.step()
            self._host_structure(st, t, it, loss, loss_of, start)
        self.new_feat = (t.x + st.delta_feat).detach()
        self.p_final = st.p.detach().clone()
        self.mem_fea, self.mem_cls = mem_fea, mem_cls
        self.edge_index, self.edge_weight = self.sample_final_edges(st.budget, st.p, t, st.pairs, mem_fea, mem_cls)

    # -- the device fit ------------------------------------------------------------------------------------------------
    def _mean_values(self, plan, dev):
        """The neighbour mean on the plan's by-destination pattern as ``[(values, counts)]`` -- the sum over the listed
        in-edges with their multiplicity, divided by their number, the reference's order -- over the edges as given and
        over the coalesced list; a self-loop slot without a listed edge weighs 0, a node without an in-edge divides by 1."""
        ec, n = plan.ec, plan.n
        dst = plan.edge_index[1].cpu()
        mult = torch.bincount(plan.raw_to_edge, minlength=ec).double()
        listed = (plan.epos >= 0).cpu()
        pos = plan.epos.cpu().long().clamp(min=0)
        out = []
        for weight in (mult, torch.ones(ec, dtype=torch.float64)):
            indeg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, weight)
            out.append((torch.where(listed, weight[pos], torch.zeros((), dtype=torch.float64)).to(dev, torch.float32),
                        indeg.clamp(min=1).to(dev, torch.float32)[:, None]))
        return out

    def _adapt(self, t, U, use_graph):
        from ..epoch_graph import run_epochs
        from ..ops import dropout_state, wgcn_view
        dev, c = t.x.device, self.num_classes
        modified_edge_index, n_perturbations, iters = self._device_state(t, parts=4)
        st, steps = self._st, self.loop_feat + self.loop_adj
        (raw_mean, raw_cnt), coalesced_mean = self._mean_values(st["plan"], dev)
        mean_graph, mean_cnt = wgcn_view(st["plan"], raw_mean), raw_cnt.clone()
        st.update(mean_graph=mean_graph, mean_cnt=mean_cnt, coalesced_mean=coalesced_mean, feat=t.x.clone(),
                  mem_fea=self._mem0.to(dev), mem_cls=torch.ones(t.n, c, dtype=torch.float32, device=dev) / c)
        self._slots(mparts=(max(self.loop_model, 1), 3))
        if self.record:
            self._slots(dtype=torch.int64, mpred=(max(self.loop_model, 1), t.n), choice=(steps, 2 + self.K, t.n))

        def record(k):
            if self.record:
                self.model_log.extend(row for it in self._mparts_buf[:k, :self.loop_model].tolist() for row in it)
                self.pred_log.extend(r for it in self._mpred_buf[:k, :self.loop_model].clone().cpu().unbind(0)
                                     for r in it.unbind(0))
                self.parts_log.extend(row for it in self._parts_buf[:k].tolist() for row in it)
                self.choice_log.extend(r for it in self._choice_buf[:k].clone().cpu().unbind(0) for r in it.unbind(0))
                self._record_weights(k)

        epochs = self.epoch
        self.optimizer.add_param_group(dict(params=[st["delta"], st["p"]], weight_decay=0.0))   # optimizer_feat, _adj
        self.epoch = iters
        try:
            # the capture's roll-back zeroes every optimiser state: the network's moments come from the pretraining
            moments = [v for state in self.optimizer.state.values() for v in state.values() if torch.is_tensor(v)]
            run_epochs(self, lambda u: self._iteration(t, u), 1, U, use_graph, after_group=record,
                       also=[st["w"], st["feat"], st["mem_fea"], st["mem_cls"], mean_graph.val, mean_cnt,
                             dropout_state.counter(dev)] + moments)
        finally:
            self.epoch = epochs
            self.optimizer.param_groups.pop()
        self._freeze()
        self.new_feat = (t.x + st["delta"]).detach()
        self.p_final = st["p"].detach().clone()
        self.mem_fea, self.mem_cls = st["mem_fea"], st["mem_cls"]
        self.edge_index, self.edge_weight = self.sample_final_edges(n_perturbations, st["p"], t, modified_edge_index,
                                                                    st["mem_fea"], st["mem_cls"])
        self._st = None

    def _tt_step(self, h0, val, view, u, j):
        from ..ops import cta_knn, cta_test_time_loss
        st = self._st
        feat_output, cls_output = self._device_layers(h0, val, view, head=True)
        idx_near, _ = cta_knn(feat_output.detach(), st["mem_fea"], self.K + 1)
        loss, parts, pred, sel = cta_test_time_loss(cls_output, feat_output, st["mem_fea"], st["mem_cls"], idx_near)
        self._parts_buf[u, j].copy_(parts)
        if self.record:
            self._choice_buf[u, j].copy_(self._choices(pred, sel, idx_near))
        return loss

    def _structure_loss(self, h0, u, j, p):
        from ..ops import wgcn_norm
        val0, w_new = wgcn_norm(self._st["plan"], self._st["w"], p, view=0)
        return self._tt_step(h0, val0, 0, u, j), w_new

    def _iteration(self, t, u):
        """One adaptation iteration into slot ``u``: ``loop_model`` steps of the network with the memory updates,
        ``loop_feat`` steps on ``delta_feat``, ``loop_adj`` on the flip weights, the carried raw weights folded once
        more.  No host decision."""
        from ..ops import GEMM_NT, cta_model_loss, gemm, linear_nt, spmm_kstep, wgcn_norm
        st, net, opt = self._st, self.graphcta, self.optimizer
        plan, delta = st["plan"], st["delta"]
        w0 = net.convs[0].lin.weight
        with torch.no_grad():
            val, _ = wgcn_norm(plan, st["w"], None, view=1)              # the weights as they stand, for this iteration
        loss = None
        for j in range(self.loop_model):
            self._freeze(False)
            net.train()
            feat_output, cls_output = self._device_layers(linear_nt(st["feat"], w0), val, 1, head=True)
            with torch.no_grad():
                proto = self._prototypes(st["mem_fea"], cls_output)
                pred = _first_argmax(spmm_kstep(st["mean_graph"], st["mem_cls"], 1, None) / st["mean_cnt"])
            loss, parts = cta_model_loss(feat_output, cls_output, proto, pred, self.tau, self.lamb)
            self._mparts_buf[u, j].copy_(parts)
            if self.record:
                self._mpred_buf[u, j].copy_(pred)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            net.eval()
            with torch.no_grad():
                feat_output, cls_output = self._device_layers(gemm(GEMM_NT, st["feat"], w0.detach()), val, 1, head=True)
                self._memory_update(st["mem_fea"], st["mem_cls"], feat_output, cls_output)
        self._freeze()
        net.eval()
        w0 = w0.detach()
        with torch.no_grad():
            xw0 = gemm(GEMM_NT, t.x, w0)                                 # the layer-0 projection, once per iteration
        for j in range(self.loop_feat):
            loss = self._tt_step(xw0 + linear_nt(delta, w0), val, 1, u, j)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        with torch.no_grad():
            h0 = xw0 + gemm(GEMM_NT, delta.detach(), w0)
        for j in range(self.loop_feat, self.loop_feat + self.loop_adj):
            loss = self._structure_step(lambda p: self._structure_loss(h0, u, j, p))
        self._fold_weights()
        with torch.no_grad():
            if self.loop_adj != 0:
                st["mean_graph"].val.copy_(st["coalesced_mean"][0])
                st["mean_cnt"].copy_(st["coalesced_mean"][1])
            if self.loop_feat != 0:
                st["feat"].copy_(t.x + delta)
        self._close_iteration(u, loss)
