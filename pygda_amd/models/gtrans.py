"""``GTrans`` trainer (pygda/models/gtrans.py): Empowering Graph Representation Learning with Test-Time Graph
Transformation (source-free, node level).

``fit`` pretrains a :class:`~pygda_amd.nn.GNNBase` on the source graph -- ``epoch`` epochs of the cross-entropy --,
freezes it (it stays in training mode, as in the reference: ``dropout > 0`` remains active) and then adapts the TARGET
GRAPH: ``epoch // (loop_feat + loop_adj)`` iterations of ``loop_feat`` Adam steps on a dense feature perturbation
``delta_feat [N, F]`` and ``loop_adj`` steps on one flip weight per target edge with ``row < col``, each followed by the
clamp to ``>= 1e-7`` and ``perturb.project`` onto the budget ``int(ratio * E // 2)``.  Both descend
``test_time_loss = inner(o1, o2) - inner(o2, o3)`` (``inner_margin`` on the second term when ``margin != -1``) over the
bottleneck's output on the graph with 5 % of its edges dropped, on the whole graph and on the whole graph with the
feature rows shuffled.  ``sample_final_edges`` restates the reference's lines as they are.  ``predict`` ignores its
argument's graph and returns the eval-mode log-probabilities on the stored ``new_feat``, ``edge_index``,
``edge_weight`` beside ``data.y``.

On the GPU the structure is fixed after the first coalesce, so a fit builds one ``ops.wgcn_plan`` and every step runs
on the kernels of csrc/gda_gtrans.hip: ``ops.wgcn_norm`` refreshes the values of the two views' CSRs from the carried
raw weights and the flip weights, ``ops.weighted_propagate`` aggregates (the SpMM kernels) with the gradient to the
values (the SDDMM), ``ops.gtrans_loss`` is the loss with its three gradients, ``ops.gtrans_project`` the projection
without a host read.  The network is frozen, so ``x W0^T`` is taken once; a step adds ``delta_feat W0^T``
(``ops.linear_nt``) and the shuffled pass gathers rows of that sum.  Pretraining epochs and adaptation iterations both
go through ``epoch_graph.run_epochs``; an iteration has no host decision in it, and eager and captured fits are
bit-identical.  The permutations are drawn from ``np.random`` before the first iteration, one per ``test_time_loss``
call including the twenty of the final sampling, and uploaded once; the final sampling runs once, eagerly, and draws
its masks and ``torch.bernoulli`` from torch's CPU generator.  Edge keep bits of the adaptation steps come from the
fused-dropout stream on the GPU, one bit per coalesced edge (before the first coalesce the reference's ``dropout_adj``
draws one per listed copy of a duplicate edge; a replayed mask of that length is folded into the kept share of the
coalesced weight), and from ``torch.rand`` on the host.  ``device='cpu'`` restates the reference's lines in
torch (any dtype; both perturbations are float32 there as well).

THE FLIP WEIGHTS DO NOT MOVE BY DEFAULT, because they do not move in the reference: its ``optimizer_adj`` holds the
tensor ``fit`` creates, while the loop works on ``perturbed_edge_weight.detach()`` and on what ``project`` returns, so
``update_edge_weights`` sets ``.grad`` on a tensor the optimiser does not hold and ``step()`` moves nothing.  The flip
weights stay at 1e-7, the raw weights wobble by 1e-7 under the repeated fold, and ``sample_final_edges`` takes ``topk``
over ties (taken on the host on either device, so that ties break as torch's CPU ``topk`` breaks them).  The fixtures
recorded from the reference pin this.  The private keyword ``step_structure=True`` runs the step those lines spell out
instead -- the gradient with respect to the flip weights through the kernels, an Adam step whose moments persist, the
clamp, the projection; without it a structure step evaluates its loss (for the log) and no gradient.

Private keywords: ``record=True`` keeps every step's ``[loss, part1, part2]`` in ``parts_log`` (the twenty calls of the
final sampling behind them) and the flip weights and
raw edge weights after every iteration in ``p_log`` / ``w_log``; ``replay=dict(masks=[...], perms=[...])`` feeds
recorded edge keep masks (one per ``test_time_loss`` call, over the edge list the call sees) and permutations instead of
drawing them.

Only ``gnn='gcn'`` (the reference hands ``edge_weight`` to the other convolutions in their ``size`` slot),
``batch_size=0``, ``loop_adj <= 1`` and ``strategy='dropedge'`` (the reference leaves ``output1`` undefined otherwise) are
supported;
anything else raises NotImplementedError naming the argument."""
import time

import numpy as np
import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn import GNNBase
from ..nn.pagerank import host_gcn_graph
from ..utils.perturb import get_modified_adj, inner, inner_margin, linear_to_triu_idx, project
from .own_epoch import OwnEpochGDA, refuse_data_parallel

DROP_P = 0.05          # test_time_loss's dropedge rate
EPS = 1e-7             # the floor of a flip weight
FINAL_ROUNDS = 20


class _PermRows(torch.autograd.Function):
    """``x[perm]`` for a permutation whose inverse is at hand: both directions are row gathers."""

    @staticmethod
    def forward(ctx, x, perm, inv):
        from ..ops import gather_rows
        ctx.save_for_backward(inv)
        return gather_rows(x, perm)

    @staticmethod
    def backward(ctx, g):
        from ..ops import gather_rows
        (inv,) = ctx.saved_tensors
        return gather_rows(g.contiguous(), inv), None, None


class GTrans(OwnEpochGDA):
    _unroll_env = "PYGDA_AMD_GRAPH_UNROLL"

    def __init__(self, in_dim, hid_dim, num_classes, num_layers=3, dropout=0., act=F.relu, loop_adj=1, loop_feat=4,
                 ratio=0.1, margin=-1, make_undirected=True, strategy='dropedge', weight_decay=0., lr=1e-4, epoch=500,
                 gnn='gcn', device='cuda:0', batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        self.record = bool(kwargs.pop("record", False))
        self.replay = kwargs.pop("replay", None)
        self.step_structure = bool(kwargs.pop("step_structure", False))
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        if gnn != 'gcn':
            raise NotImplementedError("GTrans: gnn != 'gcn' is not supported (the reference passes edge_weight into the "
                                      "other convolutions' size argument)")
        if batch_size != 0:
            raise NotImplementedError("GTrans: batch_size != 0 is not supported (only full-batch training, batch_size=0)")
        if strategy != 'dropedge':
            raise NotImplementedError("GTrans: strategy != 'dropedge' is not supported (the reference leaves output1 "
                                      "undefined for any other)")
        if loop_adj > 1:
            raise NotImplementedError("GTrans: loop_adj > 1 is not supported (the reference's second structure step "
                                      "backpropagates through the first one's freed graph and stops with an error)")
        if loop_adj < 0 or loop_feat < 0 or loop_adj + loop_feat == 0:
            raise ValueError("GTrans: loop_feat + loop_adj must be positive")
        self.gnn, self.loop_adj, self.loop_feat, self.ratio, self.margin = gnn, loop_adj, loop_feat, ratio, margin
        self.strategy, self.make_undirected = strategy, make_undirected
        self.parts_log, self.p_log, self.w_log, self._phase = [], [], [], "source"

    def init_model(self, **kwargs):
        return GNNBase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes,
                       num_layers=self.num_layers, dropout=self.dropout, gnn=self.gnn, **kwargs).to(self.device)

    def forward_model(self, data, **kwargs):
        pass

    def process_graph(self, data):
        pass

    def _check(self, source_data, target_data):
        from ..ops import WGCN_MAX_WIDTH, gtrans_bytes
        refuse_data_parallel(self)
        self._check_edges(source_data, target_data)
        y = source_data.y
        if y.numel() and (int(y.min()) < 0 or int(y.max()) >= self.num_classes):
            raise ValueError(f"GTrans: a source label is outside [0, {self.num_classes})")
        dev = torch.device(self.device)
        if dev.type == "cuda":
            if self.hid_dim > WGCN_MAX_WIDTH:
                raise ValueError(f"GTrans: the edge-gradient kernel covers hidden widths up to {WGCN_MAX_WIDTH}, got "
                                 f"{self.hid_dim}")
            n, f = target_data.x.shape
            e = target_data.edge_index.shape[1]
            resident, per_loss = gtrans_bytes(n, f, 2 * e + n, e, self.hid_dim)
            free = torch.cuda.mem_get_info(dev)[0]
            if resident + per_loss > free:
                raise MemoryError(f"GTrans: the dense [{n}, {f}] perturbation, its gradient and its two Adam moments need "
                                  f"{4 * 4 * n * f / 2 ** 30:.1f} GiB of the {(resident + per_loss) / 2 ** 30:.1f} GiB a fit "
                                  f"takes; {free / 2 ** 30:.1f} GiB are free on {dev}")

    def _report(self, epoch, loss, acc, start):
        super()._report(epoch, loss, acc if self._phase == "source" else None, start)

    def _dom(self, data, dev):
        d = super()._dom(data, dev)
        ew = getattr(data, "edge_weight", None)
        d.edge_weight = None if ew is None else ew.to(dev)
        return d

    def _init_fit(self, s, t):
        self.gtrans = self.init_model(**self.kwargs)
        self.parts_log, self.p_log, self.w_log, self._phase = [], [], [], "source"
        return self.gtrans.parameters()

    # -- what both devices share ---------------------------------------------------------------------------------------
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

    def _draws(self, n, calls):
        """One permutation per ``test_time_loss`` call, in the reference's call order, all of them now."""
        if self.replay is not None:
            perms = [np.asarray(p, dtype=np.int64) for p in self.replay["perms"]]
            if len(perms) < calls:
                raise ValueError(f"GTrans: replay holds {len(perms)} permutations, the fit makes {calls} calls")
            return perms[:calls]
        return [np.random.permutation(n) for _ in range(calls)]

    def _mask(self, call, e, dev):
        """The keep mask of ``dropout_adj(p=0.05)`` over ``e`` edges for call number ``call``: recorded, or
        ``torch.rand(e) >= p`` from torch's CPU generator."""
        if self.replay is not None:
            mask = torch.as_tensor(np.asarray(self.replay["masks"][call])).bool()
            if mask.numel() != e:
                raise ValueError(f"GTrans: replayed mask {call} covers {mask.numel()} edges, the call sees {e}")
            return mask.to(dev)
        return (torch.rand(e) >= DROP_P).to(dev)

    def _bottleneck(self, feat, edge_index, edge_weight):
        """``feat_bottleneck`` on any weighted edge list: the network's own kernels on the GPU, torch on the host."""
        net = self.gtrans
        if feat.is_cuda:
            return net.feat_bottleneck(feat, edge_index, edge_weight)
        n, x, last = feat.size(0), feat, len(net.convs) - 1
        for i, conv in enumerate(net.convs):
            x = self._host_conv(conv, x, edge_index, edge_weight, n)
            if i < last:
                x = F.dropout(net.act(x), p=net.dropout, training=net.training)
        return x

    @staticmethod
    def _host_conv(conv, x, edge_index, edge_weight, n):
        row, col, norm = host_gcn_graph(edge_index, n, x.dtype, edge_weight)
        h = F.linear(x, conv.lin.weight.to(x.dtype))
        return torch.zeros(n, h.size(1), dtype=x.dtype).index_add_(0, col, norm[:, None] * h[row]) + conv.bias.to(x.dtype)

    def _host_logits(self, x, edge_index, edge_weight=None):
        net = self.gtrans
        z = self._host_conv(net.cls, self._bottleneck(x, edge_index, edge_weight), edge_index, edge_weight, x.size(0))
        return F.log_softmax(z, dim=1)

    def test_time_loss(self, feat, edge_index, edge_weight, perm, mask):
        """The reference's ``test_time_loss`` with its two draws handed in: ``(loss, [loss, part1, part2])``."""
        from ..ops import gtrans_loss
        o1 = self._bottleneck(feat, edge_index[:, mask], edge_weight[mask])
        o2 = self._bottleneck(feat, edge_index, edge_weight)
        idx = torch.as_tensor(perm, device=feat.device)
        o3 = self._bottleneck(feat[idx, :], edge_index, edge_weight)
        if feat.is_cuda:
            return gtrans_loss(o1, o2, o3, self.margin)
        a = inner(o1, o2)
        b = inner_margin(o2, o3, margin=self.margin) if self.margin != -1 else inner(o2, o3)
        return a - b, torch.stack([a - b, a, b]).detach()

    @torch.no_grad()
    def sample_final_edges(self, n_perturbations, perturbed_edge_weight, t, modified_edge_index, perms, first_call):
        """The reference's lines as they are: top-k in the first round, ``torch.bernoulli`` of the resulting 0/1 vector
        in the nineteen that follow, each applied (without ``make_undirected``) to the pair carried from the round
        before; the edges of weight exactly 1 are kept."""
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
            mask = self._mask(first_call + i, edge_index.shape[1], dev)
            loss, parts = self.test_time_loss(feat, edge_index, edge_weight, perms[first_call + i], mask)
            if self.record:
                self.parts_log.append(parts.tolist())
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
    def _host_fit(self, s, t, optimizer):
        start = time.time()
        net = self.gtrans
        delta_feat = torch.nn.Parameter(torch.full(tuple(t.x.shape), EPS, dtype=torch.float32))
        optimizer_feat = torch.optim.Adam([delta_feat], lr=self.lr)
        modified_edge_index, n_perturbations, iters = self._setup(t)
        p = torch.full((modified_edge_index.shape[1],), EPS, dtype=torch.float32, requires_grad=True)
        held = p                                              # the tensor optimizer_adj holds
        optimizer_adj = torch.optim.Adam([held], lr=self.lr)

        def source_epoch(epoch):
            net.train()
            logits = self._host_logits(s.x, s.edge_index)
            return (F.nll_loss(F.log_softmax(logits, dim=1), s.y),
                    lambda: eval_micro_f1(s.y, logits.detach().argmax(dim=1)))

        self._host_epochs(optimizer, source_epoch, start)
        self._phase = "target"
        for v in net.parameters():
            v.requires_grad = False
        steps = self.loop_feat + self.loop_adj
        perms = self._draws(t.n, iters * steps + FINAL_ROUNDS)
        edge_index = t.edge_index
        edge_weight = torch.ones(edge_index.shape[1], dtype=t.x.dtype) if t.edge_weight is None else t.edge_weight
        call = 0

        def note(loss, parts):
            if self.record:
                self.parts_log.append(parts.tolist())

        for it in range(iters):
            p = p.detach()
            for _ in range(self.loop_feat):
                optimizer_feat.zero_grad()
                loss, parts = self.test_time_loss(t.x + delta_feat, edge_index, edge_weight, perms[call],
                                                  self._mask(call, edge_index.shape[1], "cpu"))
                call += 1
                loss.backward()
                optimizer_feat.step()
                note(loss, parts)
            new_feat = (t.x + delta_feat).detach()
            for _ in range(self.loop_adj):
                p.requires_grad = True
                edge_index, edge_weight = get_modified_adj(modified_edge_index, p, t.n, "cpu", edge_index, edge_weight,
                                                           self.make_undirected)
                loss, parts = self.test_time_loss(new_feat, edge_index, edge_weight, perms[call],
                                                  self._mask(call, edge_index.shape[1], "cpu"))
                call += 1
                note(loss, parts)
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
                self.new_feat = (t.x + delta_feat).detach()
            if self.record:
                self.p_log.append(p.detach().clone())
                self.w_log.append((edge_index.clone(), edge_weight.detach().clone()))
            self._report(it, float(loss.detach()), None, start)
        if self.loop_feat == 0:
            self.new_feat = t.x
        self.p_final = p.detach().clone()
        self.edge_index, self.edge_weight = self.sample_final_edges(n_perturbations, p, t, modified_edge_index, perms,
                                                                    iters * steps)

    # -- the device fit ------------------------------------------------------------------------------------------------
    def _device_fit(self, s, t):
        from ..epoch_graph import run_epochs
        U, use_graph = self._slots(), self._want_hip_graph()
        run_epochs(self, lambda u: self._source_epoch(s, u), s.n, U, use_graph)
        self._phase = "target"
        for v in self.gtrans.parameters():
            v.requires_grad = False
        self._adapt(t, U, use_graph)

    def _source_epoch(self, s, u):
        from ..ops import ce_stats_for, source_ce
        self.gtrans.train()
        logits = self.gtrans(s.x, s.edge_index)
        loss = source_ce(logits, s.y)
        stats = ce_stats_for(logits, s.y)
        self._step(u, loss, hit=stats[1] if stats is not None else (logits.detach().argmax(dim=1) == s.y).sum())

    def _adapt(self, t, U, use_graph):
        from ..epoch_graph import run_epochs
        from ..ops import dropout_state, wgcn_plan
        from ..optim import Adam
        dev, net = t.x.device, self.gtrans
        modified_edge_index, n_perturbations, iters = self._setup(t)
        steps, m = self.loop_feat + self.loop_adj, modified_edge_index.shape[1]
        perms = self._draws(t.n, iters * steps + FINAL_ROUNDS)
        plan = wgcn_plan(t.edge_index, t.n, modified_edge_index, t.edge_weight, self.make_undirected, dev)
        first = net.convs[0]
        with torch.no_grad():
            xw0 = first.lin(t.x).contiguous()                 # the frozen layer-0 projection of the features, once
        st = self._st = dict(
            plan=plan, xw0=xw0, w0=first.lin.weight.detach().contiguous(), n_pert=n_perturbations,
            delta=torch.nn.Parameter(torch.full(tuple(t.x.shape), EPS, dtype=torch.float32, device=dev)),
            p=torch.nn.Parameter(torch.full((m,), EPS, dtype=torch.float32, device=dev)),
            w=plan.entry_weights(plan.w0.to(dev, torch.float32)),
            perm=torch.zeros(U, steps, t.n, dtype=torch.int64, device=dev),
            inv=torch.zeros(U, steps, t.n, dtype=torch.int64, device=dev),
            keep=torch.ones(U, steps, plan.ec, dtype=torch.float32, device=dev) if self.replay is not None else None)
        perm_all = torch.from_numpy(np.stack(perms[:iters * steps]).reshape(iters, steps, t.n)).to(dev) if iters else None
        inv_all = torch.argsort(perm_all, dim=2) if iters else None
        keep_all = None
        if self.replay is not None and iters:
            keep_all = torch.stack([plan.keep_factors(np.asarray(k)) for k in self.replay["masks"][:iters * steps]]) \
                .reshape(iters, steps, plan.ec).to(dev)
        self._slots(parts=(steps, 3))
        if self.record:
            self._slots(pl=(max(m, 1),), wl=(plan.ec,))

        def stage(first_iter, k):
            st["perm"][:k].copy_(perm_all[first_iter:first_iter + k])
            st["inv"][:k].copy_(inv_all[first_iter:first_iter + k])
            if keep_all is not None:
                st["keep"][:k].copy_(keep_all[first_iter:first_iter + k])

        def record(k):
            if self.record:
                self.parts_log.extend(row for it in self._parts_buf[:k].tolist() for row in it)
                self.p_log.extend(self._pl_buf[:k, :m].clone().cpu().unbind(0))
                self.w_log.extend((plan.edge_index.cpu(), w) for w in self._wl_buf[:k].clone().cpu().unbind(0))

        pretrain_optimizer, epochs = self.optimizer, self.epoch
        self.optimizer = Adam([st["delta"], st["p"]], lr=self.lr)      # one moment pair and step count per tensor: the
        self.epoch = iters                                              # reference's optimizer_feat and optimizer_adj
        try:
            run_epochs(self, lambda u: self._iteration(t, u), 1, U, use_graph, before_group=stage, after_group=record,
                       also=[st["w"], dropout_state.counter(dev)])
        finally:
            self.optimizer, self.epoch = pretrain_optimizer, epochs
        self.new_feat = (t.x + st["delta"]).detach() if self.loop_feat != 0 else t.x
        self.p_final = st["p"].detach().clone()
        self.edge_index, self.edge_weight = self.sample_final_edges(n_perturbations, st["p"], t, modified_edge_index,
                                                                    perms, iters * steps)
        self._st = None

    def _views(self, h0, u, j, p):
        """The three bottleneck outputs of one ``test_time_loss`` call on the plan's two views, and the new raw weights."""
        from ..ops import dropout_state, wgcn_norm
        st = self._st
        plan = st["plan"]
        if st["keep"] is None:
            dropout_state.next_step(h0.device)
            val1, _ = wgcn_norm(plan, st["w"], p, p_drop=DROP_P, view=0)
        else:
            val1, _ = wgcn_norm(plan, st["w"], p, keep=st["keep"][u, j], view=0)
        val2, w_new = wgcn_norm(plan, st["w"], p, view=1)
        h3 = _PermRows.apply(h0, st["perm"][u, j], st["inv"][u, j])
        return self._device_bottleneck(h0, val1, 0), self._device_bottleneck(h0, val2, 1), \
            self._device_bottleneck(h3, val2, 1), w_new

    def _device_bottleneck(self, h, val, view):
        """``feat_bottleneck`` from the layer-0 projection ``h`` on, on the plan's view."""
        from ..ops import linear_nt, weighted_propagate
        net, plan = self.gtrans, self._st["plan"]
        last = len(net.convs) - 1
        for i, conv in enumerate(net.convs):
            if i:
                h = linear_nt(h, conv.lin.weight)
            h = weighted_propagate(h, plan, val, conv.bias, view)
            if i < last:
                h = F.dropout(net.act(h), p=net.dropout, training=net.training)
        return h

    def _iteration(self, t, u):
        """One adaptation iteration into slot ``u``: ``loop_feat`` steps on ``delta_feat``, ``loop_adj`` on the flip
        weights, the carried raw weights folded once more.  No host decision."""
        from ..ops import GEMM_NT, gemm, gtrans_loss, gtrans_project, linear_nt, wgcn_norm
        st = self._st
        delta, p, opt = st["delta"], st["p"], self.optimizer
        loss = None
        for j in range(self.loop_feat):
            o1, o2, o3, _ = self._views(st["xw0"] + linear_nt(delta, st["w0"]), u, j, None)
            loss, parts = gtrans_loss(o1, o2, o3, self.margin)
            self._parts_buf[u, j].copy_(parts)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        with torch.no_grad():
            h0 = st["xw0"] + gemm(GEMM_NT, delta.detach(), st["w0"])
        for j in range(self.loop_feat, self.loop_feat + self.loop_adj):
            with torch.set_grad_enabled(self.step_structure):
                o1, o2, o3, w_new = self._views(h0, u, j, p)
                loss, parts = gtrans_loss(o1, o2, o3, self.margin)
            self._parts_buf[u, j].copy_(parts)
            if self.step_structure:
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
            st["w"].copy_(w_new)
            gtrans_project(p, st["n_pert"], EPS)
        if self.loop_adj != 0:
            with torch.no_grad():
                _, w_new = wgcn_norm(st["plan"], st["w"], p.detach(), view=1)
                st["w"].copy_(w_new)
        self._loss_buf[u].copy_(loss.detach())
        if self.record:
            self._pl_buf[u, :p.numel()].copy_(p.detach())
            self._wl_buf[u].copy_(st["w"][st["plan"].entry_of_edge])

    # -- predict -------------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(log-probabilities of the network in eval mode on the transformed target graph, data.y)``."""
        self.gtrans.eval()
        with torch.no_grad():
            if self.new_feat.is_cuda:
                logits = self.gtrans(self.new_feat, self.edge_index, self.edge_weight)
            else:
                logits = self._host_logits(self.new_feat, self.edge_index, self.edge_weight)
        return logits, data.y
