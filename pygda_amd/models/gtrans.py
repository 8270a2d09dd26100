"""``GTrans`` trainer (pygda/models/gtrans.py): Empowering Graph Representation Learning with Test-Time Graph
Transformation (source-free, node level).

The fit is :class:`~pygda_amd.models.graph_transform.GraphTransformGDA`'s -- pretraining, the frozen network (it stays
in training mode, as in the reference: ``dropout > 0`` remains active), the feature perturbation and the flip weights,
why the flip weights do not move by default, ``loop_adj > 1`` and the final sampling are explained there.  What is
GTrans's own: both perturbations descend ``test_time_loss = inner(o1, o2) - inner(o2, o3)`` (``inner_margin`` on the
second term when ``margin != -1``) over the bottleneck's output on the graph with 5 % of its edges dropped, on the whole
graph and on the whole graph with the feature rows shuffled; adaptation runs on a fresh Adam over both perturbations
(one moment pair and step count per tensor: the reference's ``optimizer_feat`` and ``optimizer_adj``).  ``predict``
ignores its argument's graph and returns the eval-mode log-probabilities on the stored ``new_feat``, ``edge_index``,
``edge_weight`` beside ``data.y``.

On the GPU ``ops.gtrans_loss`` is the loss with its three gradients.  The network is frozen, so ``x W0^T`` is taken once;
a step adds ``delta_feat W0^T`` (``ops.linear_nt``) and the shuffled pass gathers rows of that sum.  The permutations
are drawn from ``np.random`` before the first iteration, one per ``test_time_loss`` call including the twenty of the
final sampling, and uploaded once; the final sampling draws its masks and ``torch.bernoulli`` from torch's CPU
generator.  Edge keep bits of the adaptation steps come from the fused-dropout stream on the GPU, one bit per coalesced
edge (before the first coalesce the reference's ``dropout_adj`` draws one per listed copy of a duplicate edge; a
replayed mask of that length is folded into the kept share of the coalesced weight), and from ``torch.rand`` on the
host.

Private keywords beside the shared ``record`` (a step's parts are ``[loss, part1, part2]``) and ``step_structure``:
``replay=dict(masks=[...], perms=[...])`` feeds recorded edge keep masks (one per ``test_time_loss`` call, over the edge
list the call sees) and permutations instead of drawing them.

Beside the shared refusals only ``strategy='dropedge'`` is supported (the reference leaves ``output1`` undefined
otherwise)."""
import time

import numpy as np
import torch
import torch.nn.functional as F

from .graph_transform import FINAL_ROUNDS, GraphTransformGDA

DROP_P = 0.05          # test_time_loss's dropedge rate


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


class GTrans(GraphTransformGDA):
    _net_name = "gtrans"

    def __init__(self, in_dim, hid_dim, num_classes, num_layers=3, dropout=0., act=F.relu, loop_adj=1, loop_feat=4,
                 ratio=0.1, margin=-1, make_undirected=True, strategy='dropedge', weight_decay=0., lr=1e-4, epoch=500,
                 gnn='gcn', device='cuda:0', batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        self.replay = kwargs.pop("replay", None)
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, gnn=gnn, loop_adj=loop_adj,
                         loop_feat=loop_feat, ratio=ratio, make_undirected=make_undirected, **kwargs)
        if strategy != 'dropedge':
            raise NotImplementedError("GTrans: strategy != 'dropedge' is not supported (the reference leaves output1 "
                                      "undefined for any other)")
        self.margin, self.strategy = margin, strategy

    def _check_limits(self, n, on_gpu):
        from ..ops import WGCN_MAX_WIDTH
        if on_gpu and self.hid_dim > WGCN_MAX_WIDTH:
            raise ValueError(f"GTrans: the edge-gradient kernel covers hidden widths up to {WGCN_MAX_WIDTH}, got "
                             f"{self.hid_dim}")

    def _fit_bytes(self, n, f, nnz, m):
        from ..ops import gtrans_bytes
        return gtrans_bytes(n, f, nnz, m, self.hid_dim)

    # -- what both devices share ---------------------------------------------------------------------------------------
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

    def test_time_loss(self, feat, edge_index, edge_weight, perm, mask):
        """The reference's ``test_time_loss`` with its two draws handed in: ``(loss, [loss, part1, part2])``."""
        from ..ops import gtrans_loss
        o1 = self._bottleneck(feat, edge_index[:, mask], edge_weight[mask])
        o2 = self._bottleneck(feat, edge_index, edge_weight)
        idx = torch.as_tensor(perm, device=feat.device)
        o3 = self._bottleneck(feat[idx, :], edge_index, edge_weight)
        return gtrans_loss(o1, o2, o3, self.margin)

    def _logged_loss(self, perms, call, feat, edge_index, edge_weight):
        """``test_time_loss`` call number ``call`` -- its mask drawn now --, its parts logged."""
        loss, parts = self.test_time_loss(feat, edge_index, edge_weight, perms[call],
                                          self._mask(call, edge_index.shape[1], feat.device))
        if self.record:
            self.parts_log.append(parts.tolist())
        return loss

    def sample_final_edges(self, n_perturbations, perturbed_edge_weight, t, modified_edge_index, perms, first_call):
        return self._sample_final_edges(
            n_perturbations, perturbed_edge_weight, t, modified_edge_index,
            lambda i, feat, edge_index, edge_weight: self._logged_loss(perms, first_call + i, feat, edge_index,
                                                                       edge_weight))

    # -- the host fit: the reference's lines ---------------------------------------------------------------------------
    def _host_fit(self, s, t, optimizer):
        start = time.time()
        st = self._host_state(t)
        self._host_pretrain(s, optimizer, start)
        self._freeze()
        steps = self.loop_feat + self.loop_adj
        perms = self._draws(t.n, st.iters * steps + FINAL_ROUNDS)
        call, loss = 0, None

        def loss_of(feat):
            nonlocal call
            call += 1
            return self._logged_loss(perms, call - 1, feat, st.edge_index, st.edge_weight)

        for it in range(st.iters):
            st.p = st.p.detach()
            for _ in range(self.loop_feat):
                st.optimizer_feat.zero_grad()
                loss = loss_of(t.x + st.delta_feat)
                loss.backward()
                st.optimizer_feat.step()
            self._host_structure(st, t, it, loss, loss_of, start)
        self.new_feat = st.feat
        self.p_final = st.p.detach().clone()
        self.edge_index, self.edge_weight = self.sample_final_edges(st.budget, st.p, t, st.pairs, perms,
                                                                    st.iters * steps)

    # -- the device fit ------------------------------------------------------------------------------------------------
    def _adapt(self, t, U, use_graph):
        from ..epoch_graph import run_epochs
        from ..ops import dropout_state
        from ..optim import Adam
        self._freeze()
        dev = t.x.device
        modified_edge_index, n_perturbations, iters = self._device_state(t, parts=3)
        st, steps = self._st, self.loop_feat + self.loop_adj
        plan, first = st["plan"], self.gtrans.convs[0]
        perms = self._draws(t.n, iters * steps + FINAL_ROUNDS)
        with torch.no_grad():
            xw0 = first.lin(t.x).contiguous()                 # the frozen layer-0 projection of the features, once
        st.update(xw0=xw0, w0=first.lin.weight.detach().contiguous(),
                  perm=torch.zeros(U, steps, t.n, dtype=torch.int64, device=dev),
                  inv=torch.zeros(U, steps, t.n, dtype=torch.int64, device=dev),
                  keep=torch.ones(U, steps, plan.ec, dtype=torch.float32, device=dev) if self.replay is not None else None)
        perm_all = torch.from_numpy(np.stack(perms[:iters * steps]).reshape(iters, steps, t.n)).to(dev) if iters else None
        inv_all = torch.argsort(perm_all, dim=2) if iters else None
        keep_all = None
        if self.replay is not None and iters:
            keep_all = torch.stack([plan.keep_factors(np.asarray(k)) for k in self.replay["masks"][:iters * steps]]) \
                .reshape(iters, steps, plan.ec).to(dev)

        def stage(first_iter, k):
            st["perm"][:k].copy_(perm_all[first_iter:first_iter + k])
            st["inv"][:k].copy_(inv_all[first_iter:first_iter + k])
            if keep_all is not None:
                st["keep"][:k].copy_(keep_all[first_iter:first_iter + k])

        def record(k):
            if self.record:
                self.parts_log.extend(row for it in self._parts_buf[:k].tolist() for row in it)
                self._record_weights(k)

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

    def _loss_into_slot(self, h0, u, j, p):
        """``test_time_loss`` of step ``j`` on the plan's two views, its parts into slot ``u``: the loss and the new raw
        weights."""
        from ..ops import dropout_state, gtrans_loss, wgcn_norm
        st = self._st
        plan = st["plan"]
        if st["keep"] is None:
            dropout_state.next_step(h0.device)
            val1, _ = wgcn_norm(plan, st["w"], p, p_drop=DROP_P, view=0)
        else:
            val1, _ = wgcn_norm(plan, st["w"], p, keep=st["keep"][u, j], view=0)
        val2, w_new = wgcn_norm(plan, st["w"], p, view=1)
        h3 = _PermRows.apply(h0, st["perm"][u, j], st["inv"][u, j])
        loss, parts = gtrans_loss(self._device_layers(h0, val1, 0), self._device_layers(h0, val2, 1),
                                  self._device_layers(h3, val2, 1), self.margin)
        self._parts_buf[u, j].copy_(parts)
        return loss, w_new

    def _iteration(self, t, u):
        """One adaptation iteration into slot ``u``: ``loop_feat`` steps on ``delta_feat``, ``loop_adj`` on the flip
        weights, the carried raw weights folded once more.  No host decision."""
        from ..ops import GEMM_NT, gemm, linear_nt
        st = self._st
        delta, opt = st["delta"], self.optimizer
        loss = None
        for j in range(self.loop_feat):
            loss, _ = self._loss_into_slot(st["xw0"] + linear_nt(delta, st["w0"]), u, j, None)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        with torch.no_grad():
            h0 = st["xw0"] + gemm(GEMM_NT, delta.detach(), st["w0"])
        for j in range(self.loop_feat, self.loop_feat + self.loop_adj):
            loss = self._structure_step(lambda p: self._loss_into_slot(h0, u, j, p))
        self._fold_weights()
        self._close_iteration(u, loss)
