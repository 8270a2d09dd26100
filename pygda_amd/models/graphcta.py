"""``GraphCTA`` trainer (pygda/models/graphcta.py): Collaborate to Adapt -- source-free graph domain adaptation via
bi-directional adaptation (node level).

``fit`` pretrains a :class:`~pygda_amd.nn.GNNBase` on the source graph -- ``epoch`` epochs of the cross-entropy -- and
then runs ``epoch // (loop_feat + loop_adj)`` iterations on the target alone, each of

* ``loop_model`` MODEL steps: a train-mode forward on the current features and edge weights, the prototypes of the
  feature memory per arg-max class of that forward, the pseudo label of every node from the unweighted in-neighbour mean
  of the class memory, ``ops.cta_model_loss`` (instance-prototype contrast and the similarity-weighted cross-entropy),
  an Adam step of the network (the pretraining optimiser, moments carried over), then an eval-mode forward whose
  bottleneck output and sharpened softmax move the two memory banks by ``momentum``;
* ``loop_feat`` steps on a dense feature perturbation ``delta_feat [N, F]`` and ``loop_adj`` steps on one flip weight
  per target edge with ``row < col`` (the clamp to ``>= 1e-7`` and ``perturb.project`` onto the budget ``int(ratio * E
  // 2)`` behind each), both on ``test_time_loss`` through the frozen network in eval mode: the cross-entropy of the
  low-entropy share of every predicted class against its own prediction, minus the inner product with the ``K`` nearest
  memory rows, plus the inner product with the memory rows of the other classes (``ops.cta_knn``,
  ``ops.cta_test_time_loss``).

``sample_final_edges`` restates the reference's lines as they are and runs once, eagerly, on ``data.x`` (not on the
perturbed features); its ``topk`` and ``torch.bernoulli`` are taken on the host, so that ties break as torch's CPU
``topk`` breaks them.  ``predict`` ignores its argument's graph and returns the eval-mode log-probabilities on the stored
``new_feat``, ``edge_index``, ``edge_weight`` beside ``data.y``.

On the GPU the structure is fixed after the first coalesce, so a fit builds one ``ops.wgcn_plan`` and every forward runs
on GTrans's kernels (``ops.wgcn_norm``, ``ops.weighted_propagate``, ``ops.gtrans_project``); the three losses are the
kernels of csrc/gda_graphcta.hip, which store no ``[N, N]`` array.  The layer-0 projection of the features is taken once
per iteration, after the model steps; a feature step adds ``delta_feat W0^T``.  Pretraining epochs and adaptation
iterations both go through ``epoch_graph.run_epochs``; an iteration has no host decision in it, and eager and captured
fits are bit-identical.  ``device='cpu'`` restates the reference's lines in torch (any dtype; both perturbations are
float32 there as well).

As they are in the reference: ``mem_fea = torch.rand(N, hid)`` is drawn from torch's CPU generator after ``init_model``
and ``mem_cls = 1 / C``; the neighbour mean is structural and unweighted -- over the target's edge list as given, with
multiplicity, until the first structure step has coalesced it, and over the coalesced list (with the reverse pairs that
``make_undirected`` adds at weight 1e-7) from then on; the row that ``idx_near`` drops is rank 1, whichever it is.

THE FLIP WEIGHTS DO NOT MOVE BY DEFAULT, because they do not move in the reference, by the mechanism of GTrans: its
``optimizer_adj`` holds the tensor ``fit`` creates, while the loop works on ``perturbed_edge_weight.detach()`` and on
what ``project`` returns, so ``update_edge_weights`` sets ``.grad`` on a tensor the optimiser does not hold.  The
fixtures recorded from the reference pin this.  The private keyword ``step_structure=True`` runs the step those lines
spell out instead (the gradient through the edge-gradient kernels, an Adam step whose moments persist, the clamp, the
projection); without it a structure step evaluates its loss only.  ``loop_adj > 1`` is refused: the reference's second
structure step backpropagates through the first one's freed graph and stops with torch's "backward through the graph a
second time" (tests/golden/make_golden_graphcta.py runs it and prints the message).  ``make_undirected=False`` is taken
as the reference takes it, to the end: its ``sample_final_edges`` then allows exactly ``n_perturbations`` changed edges
and flips that many pairs in its first round, so a target with a duplicate or a one-way edge fails its range assertion
after the twenty rounds (a symmetric target without duplicates passes).  The assertion is restated here as it is, and
``graphcta_fit_b.npz`` records such a fit of the reference up to its message.

Private keywords: ``record=True`` keeps every model step's ``[loss, loss_local, cl]`` in ``model_log`` with its pseudo
labels in ``pred_log``, every ``test_time_loss`` call's ``[loss, ce, nb, ng]`` in ``parts_log`` (the twenty calls of the
final sampling behind them) with ``[pred, selected, the K neighbours]`` in ``choice_log``, and the flip weights and raw
edge weights after every iteration in ``p_log`` / ``w_log``.

Only ``gnn='gcn'`` (the reference hands ``edge_weight`` to the other convolutions in their ``size`` slot),
``batch_size=0`` and ``loop_adj <= 1`` are supported; anything else raises NotImplementedError naming the argument."""
import time

import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn import GNNBase
from ..ops import first_argmax as _first_argmax
from ..utils.perturb import get_modified_adj, linear_to_triu_idx, project
from .gtrans import EPS, FINAL_ROUNDS, GTrans
from .own_epoch import OwnEpochGDA, refuse_data_parallel


class GraphCTA(OwnEpochGDA):
    _unroll_env = "PYGDA_AMD_GRAPH_UNROLL"

    def __init__(self, in_dim, hid_dim, num_classes, num_layers=3, dropout=0., act=F.relu, loop_model=3, loop_adj=1,
                 loop_feat=4, ratio=0.1, K=5, tau=0.2, lamb=0.2, momentum=0.9, make_undirected=True, weight_decay=0.,
                 lr=1e-4, epoch=500, gnn='gcn', device='cuda:0', batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        self.record = bool(kwargs.pop("record", False))
        self.step_structure = bool(kwargs.pop("step_structure", False))
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        if gnn != 'gcn':
            raise NotImplementedError("GraphCTA: gnn != 'gcn' is not supported (the reference passes edge_weight into "
                                      "the other convolutions' size argument)")
        if batch_size != 0:
            raise NotImplementedError("GraphCTA: batch_size != 0 is not supported (only full-batch training, "
                                      "batch_size=0; the reference asserts it)")
        if loop_adj > 1:
            raise NotImplementedError("GraphCTA: loop_adj > 1 is not supported (the reference's second structure step "
                                      "backpropagates through the first one's freed graph and stops with an error)")
        if loop_adj < 0 or loop_feat < 0 or loop_model < 0 or loop_adj + loop_feat == 0:
            raise ValueError("GraphCTA: loop_feat + loop_adj must be positive")
        if K < 1:
            raise ValueError("GraphCTA: K must be at least 1")
        self.gnn, self.loop_model, self.loop_adj, self.loop_feat = gnn, loop_model, loop_adj, loop_feat
        self.ratio, self.tau, self.lamb, self.momentum, self.K = ratio, tau, lamb, momentum, K
        self.make_undirected = make_undirected
        self._reset_logs()

    def _reset_logs(self):
        self.model_log, self.pred_log, self.parts_log, self.choice_log, self.p_log, self.w_log = [], [], [], [], [], []
        self._phase = "source"

    def init_model(self, **kwargs):
        return GNNBase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes,
                       num_layers=self.num_layers, dropout=self.dropout, gnn=self.gnn, **kwargs).to(self.device)

    def forward_model(self, data, **kwargs):
        pass

    def process_graph(self, data):
        pass

    def _check(self, source_data, target_data):
        from ..ops import CTA_MAX_CLASSES, CTA_MAX_K1, WGCN_MAX_WIDTH, graphcta_bytes
        refuse_data_parallel(self)
        self._check_edges(source_data, target_data)
        y = source_data.y
        if y.numel() and (int(y.min()) < 0 or int(y.max()) >= self.num_classes):
            raise ValueError(f"GraphCTA: a source label is outside [0, {self.num_classes})")
        n, f = target_data.x.shape
        if n < self.K + 1:
            raise ValueError(f"GraphCTA: K + 1 = {self.K + 1} neighbours need as many target nodes, got {n}")
        dev = torch.device(self.device)
        if dev.type == "cuda":
            if self.hid_dim > WGCN_MAX_WIDTH or self.num_classes > CTA_MAX_CLASSES or self.K + 1 > CTA_MAX_K1:
                raise ValueError(f"GraphCTA: the kernels cover hidden widths up to {WGCN_MAX_WIDTH}, {CTA_MAX_CLASSES} "
                                 f"classes and K up to {CTA_MAX_K1 - 1}, got {self.hid_dim}, {self.num_classes}, {self.K}")
            e = target_data.edge_index.shape[1]
            resident, per_loss = graphcta_bytes(n, f, 2 * e + n, e, self.hid_dim, self.num_classes, self.K)
            free = torch.cuda.mem_get_info(dev)[0]
            if resident + per_loss > free:
                raise MemoryError(f"GraphCTA: a fit takes {(resident + per_loss) / 2 ** 30:.1f} GiB -- {4 * 4 * n * f / 2 ** 30:.1f} "
                                  f"GiB for the dense [{n}, {f}] perturbation with its gradient and two Adam moments, the "
                                  f"rest for the plan, the two memory banks and the losses' workspaces (up to eight "
                                  f"[{n}, {self.hid_dim}] gradient partials, the top-k candidate lists); "
                                  f"{free / 2 ** 30:.1f} GiB are free on {dev}")

    def _report(self, epoch, loss, acc, start):
        super()._report(epoch, loss, acc if self._phase == "source" else None, start)

    def _dom(self, data, dev):
        d = super()._dom(data, dev)
        ew = getattr(data, "edge_weight", None)
        d.edge_weight = None if ew is None else ew.to(dev)
        return d

    def _init_fit(self, s, t):
        self.graphcta = self.init_model(**self.kwargs)
        self._reset_logs()
        # the reference draws the feature memory on the host, after init_model and before anything else
        self._mem0 = torch.rand(t.n, self.hid_dim)
        return self.graphcta.parameters()

    # -- what both devices share ---------------------------------------------------------------------------------------
    def _setup(self, t):
        n, ei = t.n, t.edge_index
        m_ei = ei[:, ei[0] < ei[1]]
        row, col = m_ei[0], m_ei[1]
        edge_index_id = ((2 * n - row - 1) * row // 2 + col - row - 1).long()
        modified_edge_index = linear_to_triu_idx(n, edge_index_id)
        return modified_edge_index, int(self.ratio * ei.shape[1] // 2), self.epoch // (self.loop_feat + self.loop_adj)

    def _forward(self, feat, edge_index, edge_weight):
        """``(feat_bottleneck, feat_classifier of it)`` on any weighted edge list: the network's own kernels on the GPU,
        torch on the host."""
        net = self.graphcta
        if feat.is_cuda:
            out = net.feat_bottleneck(feat, edge_index, edge_weight)
            return out, net.feat_classifier(out, edge_index, edge_weight)
        n, x, last = feat.size(0), feat, len(net.convs) - 1
        for i, conv in enumerate(net.convs):
            x = GTrans._host_conv(conv, x, edge_index, edge_weight, n)
            if i < last:
                x = F.dropout(net.act(x), p=net.dropout, training=net.training)
        return x, GTrans._host_conv(net.cls, x, edge_index, edge_weight, n)

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

    @torch.no_grad()
    def sample_final_edges(self, n_perturbations, perturbed_edge_weight, t, modified_edge_index, mem_fea, mem_cls):
        """The reference's lines as they are: top-k in the first round, ``torch.bernoulli`` of the resulting 0/1 vector
        in the nineteen that follow, each applied (without ``make_undirected``) to the pair carried from the round
        before, on ``data.x``; the edges of weight exactly 1 are kept."""
        dev = t.x.device
        best_loss = float('Inf')
        perturbed_edge_weight = perturbed_edge_weight.detach().clone()
        perturbed_edge_weight[perturbed_edge_weight <= EPS] = 0
        feat, edge_index = t.x, t.edge_index
        edge_weight = torch.ones(edge_index.shape[1], dtype=feat.dtype, device=dev)
        for i in range(FINAL_ROUNDS):
            if best_loss == float('Inf'):
                sampled_edges = torch.zeros_like(perturbed_edge_weight)
                sampled_edges[torch.topk(perturbed_edge_weight.cpu(), n_perturbations).indices.to(dev)] = 1
            else:
                sampled_edges = torch.bernoulli(perturbed_edge_weight.cpu()).float().to(dev)
            perturbed_edge_weight = sampled_edges
            edge_index, edge_weight = get_modified_adj(modified_edge_index, perturbed_edge_weight, t.n, dev, edge_index,
                                                       edge_weight)
            loss, parts, choices = self.test_time_loss(feat, edge_index, edge_weight, mem_fea, mem_cls)
            if self.record:
                self.parts_log.append(parts.tolist())
                self.choice_log.append(choices.cpu())
            if best_loss > loss:
                best_loss = loss
                best_edges = perturbed_edge_weight.clone()
        perturbed_edge_weight.copy_(best_edges)
        edge_index, edge_weight = get_modified_adj(modified_edge_index, perturbed_edge_weight, t.n, dev, edge_index,
                                                   edge_weight)
        edge_mask = edge_weight == 1
        allowed = 2 * n_perturbations if self.make_undirected else n_perturbations
        kept, clean = int(edge_mask.sum()), edge_index.shape[1]
        assert clean - allowed <= kept <= clean + allowed, \
            f'{kept} out of range with {clean} clean edges and {n_perturbations} pertutbations'
        return edge_index[:, edge_mask], edge_weight[edge_mask]

    # -- the host fit: the reference's lines ---------------------------------------------------------------------------
    def _host_logits(self, x, edge_index, edge_weight=None):
        return F.log_softmax(self._forward(x, edge_index, edge_weight)[1], dim=1)

    def _host_fit(self, s, t, optimizer):
        from ..ops import cta_model_loss
        start = time.time()
        net = self.graphcta
        delta_feat = torch.nn.Parameter(torch.full(tuple(t.x.shape), EPS, dtype=torch.float32))
        optimizer_feat = torch.optim.Adam([delta_feat], lr=self.lr)
        modified_edge_index, n_perturbations, iters = self._setup(t)
        p = torch.full((modified_edge_index.shape[1],), EPS, dtype=torch.float32, requires_grad=True)
        held = p                                              # the tensor optimizer_adj holds
        optimizer_adj = torch.optim.Adam([held], lr=self.lr)
        mem_fea = self._mem0.to(t.x.dtype)
        mem_cls = torch.ones(t.n, self.num_classes, dtype=t.x.dtype) / self.num_classes

        def source_epoch(epoch):
            net.train()
            logits = self._host_logits(s.x, s.edge_index)
            return (F.nll_loss(F.log_softmax(logits, dim=1), s.y),
                    lambda: eval_micro_f1(s.y, logits.detach().argmax(dim=1)))

        self._host_epochs(optimizer, source_epoch, start)
        self._phase = "target"
        edge_index = t.edge_index
        edge_weight = torch.ones(edge_index.shape[1], dtype=t.x.dtype) if t.edge_weight is None else t.edge_weight
        feat = t.x

        def note(parts, choices):
            if self.record:
                self.parts_log.append(parts.tolist())
                self.choice_log.append(choices)

        loss = None
        for it in range(iters):
            for _ in range(self.loop_model):
                for v in net.parameters():
                    v.requires_grad = True
                net.train()
                feat, edge_weight = feat.detach(), edge_weight.detach()
                optimizer.zero_grad()
                feat_output, cls_output = self._forward(feat, edge_index, edge_weight)
                proto = self._prototypes(mem_fea, cls_output)
                pred = _first_argmax(self._neighprop(mem_cls, edge_index))
                loss, parts = cta_model_loss(feat_output, cls_output, proto, pred, self.tau, self.lamb)
                loss.backward()
                optimizer.step()
                if self.record:
                    self.model_log.append(parts.tolist())
                    self.pred_log.append(pred.clone())
                net.eval()
                with torch.no_grad():
                    feat_output, cls_output = self._forward(feat, edge_index, edge_weight)
                    mem_fea, mem_cls = mem_fea.clone(), mem_cls.clone()
                    self._memory_update(mem_fea, mem_cls, feat_output, cls_output)
            for v in net.parameters():
                v.requires_grad = False
            p = p.detach()
            for _ in range(self.loop_feat):
                optimizer_feat.zero_grad()
                loss, parts, choices = self.test_time_loss(t.x + delta_feat, edge_index, edge_weight, mem_fea, mem_cls)
                loss.backward()
                optimizer_feat.step()
                note(parts, choices)
            new_feat = (t.x + delta_feat).detach()
            for _ in range(self.loop_adj):
                p.requires_grad = True
                edge_index, edge_weight = get_modified_adj(modified_edge_index, p, t.n, "cpu", edge_index, edge_weight,
                                                           self.make_undirected)
                loss, parts, choices = self.test_time_loss(new_feat, edge_index, edge_weight, mem_fea, mem_cls)
                note(parts, choices)
                with torch.no_grad():
                    if self.step_structure:
                        (gradient,) = torch.autograd.grad(loss, p)
                        held.data.copy_(p)
                        optimizer_adj.zero_grad()
                        held.grad = gradient
                        optimizer_adj.step()
                        p = held.detach().clone()
                    else:                                     # the reference: optimizer_adj does not hold this tensor
                        p = p.detach()
                    p.data[p < EPS] = EPS
                    p = project(n_perturbations, p, EPS)
            if self.loop_adj != 0:
                edge_index, edge_weight = get_modified_adj(modified_edge_index, p, t.n, "cpu", edge_index, edge_weight,
                                                           self.make_undirected)
                edge_weight = edge_weight.detach()
            if self.loop_feat != 0:
                feat = (t.x + delta_feat).detach()
            if self.record:
                self.p_log.append(p.detach().clone())
                self.w_log.append((edge_index.clone(), edge_weight.detach().clone()))
            self._report(it, float(loss.detach()), None, start)
        self.new_feat = (t.x + delta_feat).detach()
        self.p_final = p.detach().clone()
        self.mem_fea, self.mem_cls = mem_fea, mem_cls
        self.edge_index, self.edge_weight = self.sample_final_edges(n_perturbations, p, t, modified_edge_index, mem_fea,
                                                                    mem_cls)

    # -- the device fit ------------------------------------------------------------------------------------------------
    def _device_fit(self, s, t):
        from ..epoch_graph import run_epochs
        U, use_graph = self._slots(), self._want_hip_graph()
        run_epochs(self, lambda u: self._source_epoch(s, u), s.n, U, use_graph)
        self._phase = "target"
        self._adapt(t, U, use_graph)

    def _source_epoch(self, s, u):
        from ..ops import ce_stats_for, source_ce
        self.graphcta.train()
        logits = self.graphcta(s.x, s.edge_index)
        loss = source_ce(logits, s.y)
        stats = ce_stats_for(logits, s.y)
        self._step(u, loss, hit=stats[1] if stats is not None else (logits.detach().argmax(dim=1) == s.y).sum())

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
        from ..ops import dropout_state, wgcn_plan, wgcn_view
        dev, net = t.x.device, self.graphcta
        modified_edge_index, n_perturbations, iters = self._setup(t)
        steps, m, c = self.loop_feat + self.loop_adj, modified_edge_index.shape[1], self.num_classes
        plan = wgcn_plan(t.edge_index, t.n, modified_edge_index, t.edge_weight, self.make_undirected, dev)
        (raw_mean, raw_cnt), coalesced_mean = self._mean_values(plan, dev)
        mean_graph, mean_cnt = wgcn_view(plan, raw_mean), raw_cnt.clone()
        st = self._st = dict(
            plan=plan, n_pert=n_perturbations, mean_graph=mean_graph, mean_cnt=mean_cnt, coalesced_mean=coalesced_mean,
            delta=torch.nn.Parameter(torch.full(tuple(t.x.shape), EPS, dtype=torch.float32, device=dev)),
            p=torch.nn.Parameter(torch.full((m,), EPS, dtype=torch.float32, device=dev)),
            w=plan.entry_weights(plan.w0.to(dev, torch.float32)), feat=t.x.clone(),
            mem_fea=self._mem0.to(dev), mem_cls=torch.ones(t.n, c, dtype=torch.float32, device=dev) / c)
        self._slots(parts=(steps, 4), mparts=(max(self.loop_model, 1), 3))
        if self.record:
            self._slots(pl=(max(m, 1),), wl=(plan.ec,))
            self._slots(dtype=torch.int64, mpred=(max(self.loop_model, 1), t.n), choice=(steps, 2 + self.K, t.n))

        def record(k):
            if self.record:
                self.model_log.extend(row for it in self._mparts_buf[:k, :self.loop_model].tolist() for row in it)
                self.pred_log.extend(r for it in self._mpred_buf[:k, :self.loop_model].clone().cpu().unbind(0)
                                     for r in it.unbind(0))
                self.parts_log.extend(row for it in self._parts_buf[:k].tolist() for row in it)
                self.choice_log.extend(r for it in self._choice_buf[:k].clone().cpu().unbind(0) for r in it.unbind(0))
                self.p_log.extend(self._pl_buf[:k, :m].clone().cpu().unbind(0))
                self.w_log.extend((plan.edge_index.cpu(), w) for w in self._wl_buf[:k].clone().cpu().unbind(0))

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
        for v in net.parameters():
            v.requires_grad = False
        self.new_feat = (t.x + st["delta"]).detach()
        self.p_final = st["p"].detach().clone()
        self.mem_fea, self.mem_cls = st["mem_fea"], st["mem_cls"]
        self.edge_index, self.edge_weight = self.sample_final_edges(n_perturbations, st["p"], t, modified_edge_index,
                                                                    st["mem_fea"], st["mem_cls"])
        self._st = None

    def _device_forward(self, h, val, view):
        """``(feat_bottleneck, feat_classifier of it)`` from the layer-0 projection ``h`` on, on the plan's view."""
        from ..ops import linear_nt, weighted_propagate
        net, plan = self.graphcta, self._st["plan"]
        last = len(net.convs) - 1
        for i, conv in enumerate(net.convs):
            if i:
                h = linear_nt(h, conv.lin.weight)
            h = weighted_propagate(h, plan, val, conv.bias, view)
            if i < last:
                h = F.dropout(net.act(h), p=net.dropout, training=net.training)
        return h, weighted_propagate(linear_nt(h, net.cls.lin.weight), plan, val, net.cls.bias, view)

    def _tt_step(self, h0, val, view, u, j):
        from ..ops import cta_knn, cta_test_time_loss
        st = self._st
        feat_output, cls_output = self._device_forward(h0, val, view)
        idx_near, _ = cta_knn(feat_output.detach(), st["mem_fea"], self.K + 1)
        loss, parts, pred, sel = cta_test_time_loss(cls_output, feat_output, st["mem_fea"], st["mem_cls"], idx_near)
        self._parts_buf[u, j].copy_(parts)
        if self.record:
            self._choice_buf[u, j].copy_(self._choices(pred, sel, idx_near))
        return loss

    def _iteration(self, t, u):
        """One adaptation iteration into slot ``u``: ``loop_model`` steps of the network with the memory updates,
        ``loop_feat`` steps on ``delta_feat``, ``loop_adj`` on the flip weights, the carried raw weights folded once
        more.  No host decision."""
        from ..ops import GEMM_NT, cta_model_loss, gemm, gtrans_project, linear_nt, spmm_kstep, wgcn_norm
        st, net, opt = self._st, self.graphcta, self.optimizer
        plan, delta, p = st["plan"], st["delta"], st["p"]
        w0 = net.convs[0].lin.weight
        with torch.no_grad():
            val, _ = wgcn_norm(plan, st["w"], None, view=1)              # the weights as they stand, for this iteration
        loss = None
        for j in range(self.loop_model):
            for v in net.parameters():
                v.requires_grad = True
            net.train()
            feat_output, cls_output = self._device_forward(linear_nt(st["feat"], w0), val, 1)
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
                feat_output, cls_output = self._device_forward(gemm(GEMM_NT, st["feat"], w0.detach()), val, 1)
                self._memory_update(st["mem_fea"], st["mem_cls"], feat_output, cls_output)
        for v in net.parameters():
            v.requires_grad = False
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
            with torch.set_grad_enabled(self.step_structure):
                val0, w_new = wgcn_norm(plan, st["w"], p, view=0)
                loss = self._tt_step(h0, val0, 0, u, j)
            if self.step_structure:
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
            st["w"].copy_(w_new)
            gtrans_project(p, st["n_pert"], EPS)
        with torch.no_grad():
            if self.loop_adj != 0:
                _, w_new = wgcn_norm(plan, st["w"], p.detach(), view=1)
                st["w"].copy_(w_new)
                st["mean_graph"].val.copy_(st["coalesced_mean"][0])
                st["mean_cnt"].copy_(st["coalesced_mean"][1])
            if self.loop_feat != 0:
                st["feat"].copy_(t.x + delta)
        self._loss_buf[u].copy_(loss.detach())
        if self.record:
            self._pl_buf[u, :p.numel()].copy_(p.detach())
            self._wl_buf[u].copy_(st["w"][plan.entry_of_edge])

    # -- predict -------------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(log-probabilities of the network in eval mode on the transformed target graph, data.y)``."""
        self.graphcta.eval()
        with torch.no_grad():
            if self.new_feat.is_cuda:
                logits = self.graphcta(self.new_feat, self.edge_index, self.edge_weight)
            else:
                logits = self._host_logits(self.new_feat, self.edge_index, self.edge_weight)
        return logits, data.y
