"""``GraphTransformGDA``: what GTrans and GraphCTA share -- the source-free trainers that pretrain a
:class:`~pygda_amd.nn.GNNBase` on the source graph and then transform the TARGET GRAPH: ``epoch // (loop_feat +
loop_adj)`` iterations of ``loop_feat`` Adam steps on a dense feature perturbation ``delta_feat [N, F]`` and ``loop_adj``
steps on one flip weight per target edge with ``row < col``, each followed by the clamp to ``>= 1e-7`` and
``perturb.project`` onto the budget ``int(ratio * E // 2)``, and at the end ``sample_final_edges``.  The class owns the
constructor's shared half, the source pretraining on either device, ``_setup``, the host structure step and iteration
tail, the device layer loop, structure step, fold and slot copies, the final sampling's body, the memory check's frame
and ``predict``.  A trainer supplies its ``test_time_loss``, the loop of feature steps around it (and whatever runs
before them), its optimiser handling, ``_check_limits`` / ``_fit_bytes`` and ``sample_final_edges`` as a call of
``_sample_final_edges`` with its loss; it names its network's attribute in ``_net_name``.

On the GPU the structure is fixed after the first coalesce, so a fit builds one ``ops.wgcn_plan`` and every step runs on
the kernels of csrc/gda_gtrans.hip: ``ops.wgcn_norm`` refreshes the values of the plan's CSRs from the carried raw
weights and the flip weights, ``ops.weighted_propagate`` aggregates with the gradient to the values,
``ops.gtrans_project`` is the projection without a host read.  Pretraining epochs and adaptation iterations both go
through ``epoch_graph.run_epochs``; an iteration has no host decision in it, and eager and captured fits are
bit-identical.  ``device='cpu'`` restates the reference's lines in torch (any dtype; both perturbations are float32
there as well).

THE FLIP WEIGHTS DO NOT MOVE BY DEFAULT, because they do not move in the reference: its ``optimizer_adj`` holds the
tensor ``fit`` creates, while the loop works on ``perturbed_edge_weight.detach()`` and on what ``project`` returns, so
``update_edge_weights`` sets ``.grad`` on a tensor the optimiser does not hold and ``step()`` moves nothing.  The flip
weights stay at 1e-7 and the raw weights wobble by 1e-7 under the repeated fold.  The fixtures recorded from the
reference pin this.  The private keyword ``step_structure=True`` runs the step those lines spell out instead -- the
gradient with respect to the flip weights through the kernels, an Adam step whose moments persist, the clamp, the
projection; without it a structure step evaluates its loss (for the log) and no gradient.

``loop_adj > 1`` is refused: the reference's second structure step backpropagates through the first one's freed graph
and stops with torch's "backward through the graph a second time" (tests/golden/make_golden_graphcta.py runs it and
prints the message).

THE FINAL SAMPLING restates the reference's lines as they are and runs once, eagerly: top-k in the first round,
``torch.bernoulli`` of the resulting 0/1 vector in the nineteen that follow, each applied (without ``make_undirected``)
to the pair carried from the round before; the edges of weight exactly 1 are kept.  With flip weights that never moved
the ``topk`` runs over ties; it and ``torch.bernoulli`` are taken on the host on either device, so that ties break as
torch's CPU ``topk`` breaks them.  ``make_undirected=False`` is taken as the reference takes it, to the end: the sampling
then allows exactly ``n_perturbations`` changed edges and flips that many pairs in its first round, so a target with a
duplicate or a one-way edge fails its range assertion after the twenty rounds (a symmetric target without duplicates
passes).  The assertion is restated as it is, and ``graphcta_fit_b.npz`` records such a fit of the reference up to its
message.

Private keywords: ``record=True`` keeps every ``test_time_loss`` call's parts in ``parts_log`` (the twenty calls of the
final sampling behind them) and the flip weights and raw edge weights after every iteration in ``p_log`` / ``w_log``.

Only ``gnn='gcn'`` (the reference hands ``edge_weight`` to the other convolutions in their ``size`` slot),
``batch_size=0`` and ``loop_adj <= 1`` are supported; anything else raises NotImplementedError naming the argument."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn import GNNBase
from ..nn.host import _host_bottleneck, _host_conv
from ..utils.perturb import get_modified_adj, linear_to_triu_idx, project
from .own_epoch import SourceFreeGDA, refuse_data_parallel

EPS = 1e-7             # the floor of a flip weight
FINAL_ROUNDS = 20


class GraphTransformGDA(SourceFreeGDA):
    _net_name = None              # the attribute that holds the network: the reference's name for it

    def __init__(self, *, gnn, loop_adj, loop_feat, ratio, make_undirected, batch_size, **kwargs):
        self.record = bool(kwargs.pop("record", False))
        self.step_structure = bool(kwargs.pop("step_structure", False))
        super().__init__(batch_size=batch_size, **kwargs)
        name = type(self).__name__
        if gnn != 'gcn':
            raise NotImplementedError(f"{name}: gnn != 'gcn' is not supported (the reference passes edge_weight into the "
                                      "other convolutions' size argument)")
        if batch_size != 0:
            raise NotImplementedError(f"{name}: batch_size != 0 is not supported (only full-batch training, "
                                      "batch_size=0)")
        if loop_adj > 1:
            raise NotImplementedError(f"{name}: loop_adj > 1 is not supported (the reference's second structure step "
                                      "backpropagates through the first one's freed graph and stops with an error)")
        if loop_adj < 0 or loop_feat < 0 or loop_adj + loop_feat == 0:
            raise ValueError(f"{name}: loop_feat + loop_adj must be positive")
        self.gnn, self.loop_adj, self.loop_feat, self.ratio = gnn, loop_adj, loop_feat, ratio
        self.make_undirected = make_undirected
        self._reset_logs()

    _net = property(lambda self: getattr(self, self._net_name))

    def _reset_logs(self):
        self.parts_log, self.p_log, self.w_log, self._phase = [], [], [], "source"

    def init_model(self, **kwargs):
        return GNNBase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes,
                       num_layers=self.num_layers, dropout=self.dropout, gnn=self.gnn, **kwargs).to(self.device)

    def _check(self, source_data, target_data):
        refuse_data_parallel(self)
        self._check_edges(source_data, target_data)
        self._check_labels(source_data.y)
        n, f = target_data.x.shape
        dev = torch.device(self.device)
        self._check_limits(n, dev.type == "cuda")
        if dev.type == "cuda":
            e = target_data.edge_index.shape[1]
            need, free = sum(self._fit_bytes(n, f, 2 * e + n, e)), torch.cuda.mem_get_info(dev)[0]
            if need > free:
                raise MemoryError(f"{type(self).__name__}: a fit takes {need / 2 ** 30:.1f} GiB, "
                                  f"{4 * 4 * n * f / 2 ** 30:.1f} GiB of them for the dense [{n}, {f}] perturbation "
                                  f"with its gradient and two Adam moments; {free / 2 ** 30:.1f} GiB are free on {dev}")

    def _dom(self, data, dev):
        d = super()._dom(data, dev)
        ew = getattr(data, "edge_weight", None)
        d.edge_weight = None if ew is None else ew.to(dev)
        return d

    def _init_fit(self, s, t):
        setattr(self, self._net_name, self.init_model(**self.kwargs))
        self._reset_logs()
        return self._net.parameters()

    def _freeze(self, frozen=True):
        for v in self._net.parameters():
            v.requires_grad = not frozen

    def _setup(self, t):
        """The flip weights' node pairs, the budget and the number of iterations, as the reference computes them."""
        n, ei = t.n, t.edge_index
        m_ei = ei[:, ei[0] < ei[1]]
        row, col = m_ei[0], m_ei[1]
        edge_index_id = ((2 * n - row - 1) * row // 2 + col - row - 1).long()
        modified_edge_index = linear_to_triu_idx(n, edge_index_id)
        n_perturbations = int(self.ratio * ei.shape[1] // 2)
        iters = self.epoch // (self.loop_feat + self.loop_adj)
        return modified_edge_index, n_perturbations, iters

    # -- the network on any weighted edge list: its own kernels on the GPU, torch on the host ---------------------------
    def _bottleneck(self, feat, edge_index, edge_weight):
        if feat.is_cuda:
            return self._net.feat_bottleneck(feat, edge_index, edge_weight)
        return _host_bottleneck(self._net, feat, edge_index, edge_weight)

    def _forward(self, feat, edge_index, edge_weight):
        """``(feat_bottleneck, feat_classifier of it)``."""
        out = self._bottleneck(feat, edge_index, edge_weight)
        if feat.is_cuda:
            return out, self._net.feat_classifier(out, edge_index, edge_weight)
        return out, _host_conv(self._net.cls, out, edge_index, edge_weight)

    def _host_logits(self, x, edge_index, edge_weight=None):
        return F.log_softmax(self._forward(x, edge_index, edge_weight)[1], dim=1)

    def predict(self, data):
        """``(log-probabilities of the network in eval mode on the transformed target graph, data.y)``."""
        self._net.eval()
        with torch.no_grad():
            if self.new_feat.is_cuda:
                logits = self._net(self.new_feat, self.edge_index, self.edge_weight)
            else:
                logits = self._host_logits(self.new_feat, self.edge_index, self.edge_weight)
        return logits, data.y

    @torch.no_grad()
    def _sample_final_edges(self, n_perturbations, perturbed_edge_weight, t, modified_edge_index, loss_of):
        """The reference's lines as they are (see the module's docstring), on ``data.x``; ``loss_of(i, feat, edge_index,
        edge_weight)`` is the trainer's ``test_time_loss`` of round ``i``."""
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
            loss = loss_of(i, feat, edge_index, edge_weight)
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
    def _host_state(self, t):
        """Both perturbations with their optimisers, ``_setup``'s three figures and the carried edge list."""
        delta_feat = torch.nn.Parameter(torch.full(tuple(t.x.shape), EPS, dtype=torch.float32))
        pairs, budget, iters = self._setup(t)
        p = torch.full((pairs.shape[1],), EPS, dtype=torch.float32, requires_grad=True)
        edge_weight = torch.ones(t.edge_index.shape[1], dtype=t.x.dtype) if t.edge_weight is None else t.edge_weight
        return SimpleNamespace(delta_feat=delta_feat, optimizer_feat=torch.optim.Adam([delta_feat], lr=self.lr),
                               pairs=pairs, budget=budget, iters=iters, p=p,
                               held=p, optimizer_adj=torch.optim.Adam([p], lr=self.lr),   # the tensor optimizer_adj holds
                               edge_index=t.edge_index, edge_weight=edge_weight, feat=t.x)

    def _host_pretrain(self, s, optimizer, start):
        net = self._net

        def source_epoch(epoch):
            net.train()
            logits = self._host_logits(s.x, s.edge_index)
            return (F.nll_loss(F.log_softmax(logits, dim=1), s.y),
                    lambda: eval_micro_f1(s.y, logits.detach().argmax(dim=1)))

        self._host_epochs(optimizer, source_epoch, start)
        self._phase = "target"

    def _host_fold(self, st, t):
        st.edge_index, st.edge_weight = get_modified_adj(st.pairs, st.p, t.n, "cpu", st.edge_index, st.edge_weight,
                                                         self.make_undirected)

    def _host_structure(self, st, t, it, loss, loss_of, start):
        """The structure half of host iteration ``it``: ``loop_adj`` steps on ``loss_of(feat)`` over the folded edge
        list, then the iteration's tail -- the carried weights folded once more, ``st.feat``, the logs."""
        new_feat = (t.x + st.delta_feat).detach()
        for _ in range(self.loop_adj):
            st.p.requires_grad = True
            self._host_fold(st, t)
            loss = loss_of(new_feat)
            with torch.no_grad():
                if self.step_structure:
                    (gradient,) = torch.autograd.grad(loss, st.p)
                    st.held.data.copy_(st.p)
                    st.optimizer_adj.zero_grad()
                    st.held.grad = gradient
                    st.optimizer_adj.step()
                    p = st.held.detach().clone()
                else:                                         # the reference: optimizer_adj does not hold this tensor
                    p = st.p.detach()
                p.data[p < EPS] = EPS
                st.p = project(st.budget, p, EPS)
        if self.loop_adj != 0:
            self._host_fold(st, t)
            st.edge_weight = st.edge_weight.detach()
        if self.loop_feat != 0:
            st.feat = new_feat
        if self.record:
            self.p_log.append(st.p.detach().clone())
            self.w_log.append((st.edge_index.clone(), st.edge_weight.detach().clone()))
        self._report(it, float(loss.detach()), None, start)

    # -- the device fit ------------------------------------------------------------------------------------------------
    def _device_fit(self, s, t):
        from ..epoch_graph import run_epochs
        U, use_graph = self._slots(), self._want_hip_graph()
        run_epochs(self, lambda u: self._source_epoch(s, u), s.n, U, use_graph)
        self._phase = "target"
        self._adapt(t, U, use_graph)

    def _source_epoch(self, s, u):
        from ..ops import ce_stats_for, source_ce
        self._net.train()
        logits = self._net(s.x, s.edge_index)
        loss = source_ce(logits, s.y)
        stats = ce_stats_for(logits, s.y)
        self._step(u, loss, hit=stats[1] if stats is not None else (logits.detach().argmax(dim=1) == s.y).sum())

    def _device_state(self, t, parts):
        """``self._st``: the plan, the budget, both perturbations and the carried raw weights; the slot buffers of the
        ``parts``-wide loss parts and, when recording, of the flip and raw weights.  Returns ``_setup``'s figures."""
        from ..ops import wgcn_plan
        dev = t.x.device
        pairs, budget, iters = self._setup(t)
        plan = wgcn_plan(t.edge_index, t.n, pairs, t.edge_weight, self.make_undirected, dev)
        m = pairs.shape[1]
        self._st = dict(
            plan=plan, n_pert=budget,
            delta=torch.nn.Parameter(torch.full(tuple(t.x.shape), EPS, dtype=torch.float32, device=dev)),
            p=torch.nn.Parameter(torch.full((m,), EPS, dtype=torch.float32, device=dev)),
            w=plan.entry_weights(plan.w0.to(dev, torch.float32)))
        self._slots(parts=(self.loop_feat + self.loop_adj, parts))
        if self.record:
            self._slots(pl=(max(m, 1),), wl=(plan.ec,))
        return pairs, budget, iters

    def _record_weights(self, k):
        """``after_group``'s shared half: the ``k`` iterations' flip and raw weights from their slots."""
        plan, m = self._st["plan"], self._st["p"].numel()
        self.p_log.extend(self._pl_buf[:k, :m].clone().cpu().unbind(0))
        self.w_log.extend((plan.edge_index.cpu(), w) for w in self._wl_buf[:k].clone().cpu().unbind(0))

    def _device_layers(self, h, val, view, head=False):
        """``feat_bottleneck`` from the layer-0 projection ``h`` on, on the plan's view; with ``head`` also
        ``feat_classifier`` of it."""
        from ..ops import linear_nt, weighted_propagate
        net, plan = self._net, self._st["plan"]
        last = len(net.convs) - 1
        for i, conv in enumerate(net.convs):
            if i:
                h = linear_nt(h, conv.lin.weight)
            h = weighted_propagate(h, plan, val, conv.bias, view)
            if i < last:
                h = F.dropout(net.act(h), p=net.dropout, training=net.training)
        if not head:
            return h
        return h, weighted_propagate(linear_nt(h, net.cls.lin.weight), plan, val, net.cls.bias, view)

    def _structure_step(self, loss_of):
        """One step on the flip weights: ``loss_of(p)`` gives the loss and the folded raw weights; the Adam step only
        under ``step_structure``; the clamp and the projection."""
        from ..ops import gtrans_project
        st = self._st
        with torch.set_grad_enabled(self.step_structure):
            loss, w_new = loss_of(st["p"])
        if self.step_structure:
            self.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            self.optimizer.step()
        st["w"].copy_(w_new)
        gtrans_project(st["p"], st["n_pert"], EPS)
        return loss

    def _fold_weights(self):
        """The carried raw weights folded once more behind the structure steps."""
        from ..ops import wgcn_norm
        st = self._st
        if self.loop_adj != 0:
            with torch.no_grad():
                _, w_new = wgcn_norm(st["plan"], st["w"], st["p"].detach(), view=1)
                st["w"].copy_(w_new)

    def _close_iteration(self, u, loss):
        """The iteration's loss and, when recording, its flip and raw weights into slot ``u``."""
        st = self._st
        self._loss_buf[u].copy_(loss.detach())
        if self.record:
            self._pl_buf[u, :st["p"].numel()].copy_(st["p"].detach())
            self._wl_buf[u].copy_(st["w"][st["plan"].entry_of_edge])
