"""``KBL`` trainer (pygda/models/kbl.py): Bridged-GNN, knowledge bridge learning (node level).

``fit`` runs three stages.

1. THE BRIDGE MODEL (``BridgedGraph.fit`` / ``train_adv_few_shot``): ``bridge_epochs`` full-batch epochs of a SAGE
   encoder per domain.  Per epoch the source side gives the pair loss -- ``PairEnumerator.sampling`` draws two lists of
   train-mask nodes (two classes, 100 nodes with replacement per class and list) and the loss is the mean BCE of
   ``sigmoid(cos(u_i, u_j))`` against ``[y_i == y_j]`` over the 40000 pairs of their Cartesian product, ``u = z +
   biasatt(z)``, ``z = lin_self(h)`` -- and the classifier's NLL on the train mask; the target side an auto-encoder
   (``0.1 MSE(recons, h0)``) and the generator's BCE against a discriminator, which a second Adam step then trains on
   the detached embeddings of both domains.  The trainer's own ``hid_dim``, ``num_layers``, ``dropout``, ``lr`` and
   ``weight_decay`` do not reach this stage, as in the reference, whose ``init_model`` hard-codes them; the keywords
   ``bridge_epochs=400``, ``bridge_hidden=64``, ``bridge_lr=1e-3``, ``bridge_weight_decay=5e-3``,
   ``encoder_dropout=0.5``, ``clf_dropout=0.6`` and ``gnn_dropout=0.1`` default to those constants.
2. THE BRIDGED GRAPH (``gen_bridged_graph``), in eval mode (BatchNorm on its running statistics, which only saw the
   source): the ``k_cross`` pairs of largest ``sigmoid(cos(u_src_i, u_tar_j))`` over ALL source-target pairs
   (``k_cross`` is the total number of bridge edges, not a per-node count) and the within-domain edges below are joined
   to both graphs' edges, coalesced and made undirected; ``central_mask`` marks the source rows.
3. THE CLASSIFIER: a ``GNNBase`` (gcn, ``bridge_hidden`` wide, 2 layers) on the merged graph, ``epoch`` epochs of the
   NLL of the central rows with Adam(``lr``, ``weight_decay``); the log's accuracy is the training-mode forward's.

``predict(data)`` ignores ``data``'s graph, as the reference does: it returns the eval-mode log-probabilities of the LAST
``data.x.shape[0]`` rows of the stored merged graph beside ``data.y``.

THE WITHIN-DOMAIN EDGES ARE A QUIRK THAT IS KEPT.  The reference calls ``Similar.similarity`` with ``[N, 1]`` index
tensors, so ``CosineSimilarity(dim=1)`` reduces a dimension of size one: the result is an ``[N, 128]`` array that is 1
where the entry of ``u`` is non-zero and 0 where it is zero.  After the sigmoid it is viewed as ``[128, N]``, flattened,
and ``topk(k_within)`` is taken over values that (nearly) all tie; torch's CPU ``topk`` returns the flat indices
``0 .. k_within - 1``, the edges ``(0, 0 .. k_within - 1)`` in each domain.  The indicator is computed on the device of
the fit and its ``topk`` is taken on the host on either device, so that ties break as torch's CPU ``topk`` breaks them
(the convention of ``gtrans.py`` and ``graphcta.py``).  A domain with fewer than 128 nodes could name a node that does
not exist; that is refused.

On the GPU stage 1 goes through ``epoch_graph.run_epochs``: the index lists of every bridge epoch are drawn up front
(the draws do not depend on the model) and uploaded once, a replay reads its epochs' lists from slot buffers, and an
epoch has no host decision in it.  The pair loss is ``ops.kbl_pair_bce`` (no ``[40000, 128]`` gathers), the bridge edges
``ops.kbl_bridge_topk`` (no ``[N_src, N_tar]`` array), dropout the keep-bit stream of csrc/gda_dropout.h, stage 3 the
GCN path of the ``GNN`` trainer.  One Adam holds the reference's three optimisers as parameter groups (a step moves the
parameters that hold a gradient).  Eager and captured fits are bit-identical.  ``device='cpu'`` restates the
reference's lines in torch, in its call order (any dtype): a seeded host fit follows the reference, dropout included.

``loss_sim.backward()`` also leaves gradients on the discriminator, which ``optimizer_d.zero_grad()`` clears before the
discriminator's own step: here they are dropped before the first step.

Refused with a message: ``batch_size != 0`` (the reference asserts it), data-parallel runs, edge indices out of range, a
source without ``train_mask`` (a missing ``val_mask`` / ``test_mask`` counts as all false).  The private keyword
``init_hook(model)`` runs once after ``init_model`` (tests load a recorded state there)."""
import time

import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn.host import _host_bottleneck, _host_conv
from ..nn.kbl_base import KBLBase, PairEnumerator
from .own_epoch import OwnEpochGDA, refuse_data_parallel

EMBED = 128                                    # the width of lin_self's output, a constant of the reference


def _coalesce(edge_index, n):
    key = torch.unique(edge_index[0] * n + edge_index[1])
    return torch.stack([key // n, key % n])


class KBL(OwnEpochGDA):
    def __init__(self, in_dim, hid_dim, num_classes, k_cross=50, k_within=10, num_layers=2, dropout=0., act=F.relu,
                 weight_decay=5e-3, lr=1e-3, epoch=200, device='cuda:0', batch_size=0, num_neigh=-1, verbose=2, *,
                 bridge_epochs=400, bridge_hidden=64, bridge_lr=1e-3, bridge_weight_decay=5e-3, encoder_dropout=0.5,
                 clf_dropout=0.6, gnn_dropout=0.1, **kwargs):
        self.init_hook = kwargs.pop("init_hook", None)
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        if batch_size != 0:
            raise NotImplementedError("KBL: batch_size != 0 is not supported (only full-batch training, batch_size=0; "
                                      "the reference asserts it)")
        if k_cross < 1 or k_within < 0 or bridge_epochs < 0:
            raise ValueError("KBL: k_cross must be positive, k_within and bridge_epochs non-negative")
        self.k_cross, self.k_within = int(k_cross), int(k_within)
        self.bridge_epochs, self.bridge_hidden, self.bridge_lr = int(bridge_epochs), int(bridge_hidden), bridge_lr
        self.bridge_weight_decay = bridge_weight_decay
        self.encoder_dropout, self.clf_dropout, self.gnn_dropout = encoder_dropout, clf_dropout, gnn_dropout
        self._reset_logs()

    def _reset_logs(self):
        self.bridge_log, self.train_log, self._phase = [], [], "bridge"

    def init_model(self, **kwargs):
        return KBLBase(data_src=self.source_data, data_tar=self.target_data, device=self.device, k_cross=self.k_cross,
                       k_within=self.k_within, bridge_batch_size=1000, dim_hidden=self.bridge_hidden, num_layer=2,
                       num_epoch=self.bridge_epochs, lr=self.bridge_lr, weight_decay=self.bridge_weight_decay,
                       source_clf=True, norm_mode='None', norm_scale=1., encoder_dropout=self.encoder_dropout,
                       clf_dropout=self.clf_dropout, gnn_dropout=self.gnn_dropout, **kwargs).to(self.device)

    def forward_model(self, source_data, target_data):
        pass

    def process_graph(self, data):
        pass

    def _check(self, source_data, target_data):
        refuse_data_parallel(self)
        self._check_edges(source_data, target_data)
        mask = getattr(source_data, "train_mask", None)
        if mask is None:
            raise ValueError("KBL: the source graph needs a train_mask (the pairs and the classifier's loss are drawn "
                             "from it)")
        if source_data.y.numel() and int(source_data.y.min()) < 0:
            raise ValueError("KBL: a source label is negative")
        if self.k_cross > source_data.x.shape[0] * target_data.x.shape[0]:
            raise ValueError(f"KBL: k_cross = {self.k_cross} exceeds the number of source-target pairs")
        for d in (source_data, target_data):
            if self.k_within > 0 and d.x.shape[0] < EMBED:
                raise ValueError(f"KBL: k_within > 0 needs at least {EMBED} nodes per domain (the reference's "
                                 f"within-domain edges name nodes up to {EMBED - 1}), got {d.x.shape[0]}")

    def _dom(self, data, dev):
        d = super()._dom(data, dev)
        for name in ("train_mask", "val_mask", "test_mask"):
            m = getattr(data, name, None)
            setattr(d, name, torch.zeros(d.n, dtype=torch.bool, device=dev) if m is None else m.to(dev).bool())
        return d

    def _report(self, epoch, loss, acc, start):
        if self._phase == "gnn":
            self.train_log.append((loss, acc))
        super()._report(epoch, loss, acc if self._phase == "gnn" else None, start)

    def _init_fit(self, s, t):
        self.source_data, self.target_data = s, t
        self.kbl = self.init_model(**self.kwargs)
        if not s.x.is_cuda:
            self.kbl = self.kbl.to(s.x.dtype)
        if self.init_hook is not None:
            self.init_hook(self.kbl)
        self._reset_logs()
        # the draws do not depend on the model: every bridge epoch's two index lists, in the reference's order
        enum = PairEnumerator(s, mode='train')
        lists = [enum.sampling_lists(max_class_num=2, sample_size=40000) for _ in range(self.bridge_epochs)]
        self.pair_lists = (torch.stack([a for a, _ in lists]) if lists else torch.zeros(0, 1, dtype=torch.long),
                           torch.stack([b for _, b in lists]) if lists else torch.zeros(0, 1, dtype=torch.long))
        return self.kbl.bridged_graph.param_groups() + [dict(params=list(self.kbl.gnn.parameters()))]

    # -- what both devices share ---------------------------------------------------------------------------------------
    def _bridge_losses(self, s, t, ia, ib):
        """One epoch's forward in the reference's call order (source encoder, classifier, similarity, target):
        ``(loss_sim, [loss_sim, loss_ae, loss_g, loss_recons], h_src, h_tar)``."""
        from ..ops import kbl_pair_bce
        model = self.kbl.bridged_graph.model
        sim = model.source_learner.sim_net
        h_src = model.source_learner.backbone(s.x, s.edge_index)
        log_probs = sim.classify(h_src)
        loss_pair = kbl_pair_bce(sim.embed(h_src), ia, ib, s.y)
        h0_tar, h_tar, recons = model.target_learner(t)
        loss_recons = F.mse_loss(recons, h0_tar)
        loss_g = F.binary_cross_entropy(model.discriminator(h_tar), torch.ones_like(h_tar[:, :1]))
        loss_ae = loss_g + loss_recons * 0.1
        loss_sim = loss_pair + loss_ae + F.nll_loss(log_probs[self._train_idx], self._train_y)
        return loss_sim, [loss_sim, loss_ae, loss_g, loss_recons], h_src, h_tar

    def _disc_loss(self, h_src, h_tar):
        disc = self.kbl.bridged_graph.model.discriminator
        real = F.binary_cross_entropy(disc(h_src.detach()), torch.ones_like(h_src[:, :1]))
        fake = F.binary_cross_entropy(disc(h_tar.detach()), torch.zeros_like(h_tar[:, :1]))
        return (real + fake) / 2

    def _bridge_step(self, optimizer, s, t, ia, ib):
        """``train_adv_few_shot``: ``[loss_sim, loss_d, loss_ae, loss_g, loss_recons]`` (detached), both steps taken."""
        model = self.kbl.bridged_graph.model
        model.train()
        optimizer.zero_grad(set_to_none=True)
        loss_sim, parts, h_src, h_tar = self._bridge_losses(s, t, ia, ib)
        loss_sim.backward()
        for p in model.discriminator.parameters():         # optimizer_d.zero_grad() clears these before its own step
            p.grad = None
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        loss_d = self._disc_loss(h_src, h_tar)
        loss_d.backward()
        optimizer.step()
        return torch.stack([parts[0].detach(), loss_d.detach()] + [p.detach() for p in parts[1:]])

    @torch.no_grad()
    def _within_edges(self, u):
        """The reference's within-domain ``topk`` (see the module docstring): ``u [N, 128]`` -> a coalesced ``[2, k]``."""
        n = u.size(0)
        if u.is_cuda:
            sign = u / u.abs().clamp_min(1e-8)             # CosineSimilarity over a dimension of size one
            alpha = torch.sigmoid(sign * sign)
        else:
            idx = torch.arange(n).unsqueeze(-1)
            alpha = torch.sigmoid(F.cosine_similarity(u[idx], u[idx], dim=1))
        mat = alpha.cpu().reshape(-1)
        val, flat = mat.topk(k=self.k_within)              # on the host on either device: torch's CPU tie order
        edges = _coalesce(torch.stack([flat // n, flat % n]), n)
        return edges, val, flat

    @torch.no_grad()
    def _gen_bridged_graph(self, s, t):
        from ..ops import kbl_bridge_topk
        from types import SimpleNamespace
        model = self.kbl.bridged_graph.model
        model.eval()
        dev = s.x.device
        u_src, u_tar = model.embeddings(s, t)
        row, col, val = kbl_bridge_topk(u_src, u_tar, self.k_cross)
        self.bridge_edges = (row.long().cpu(), col.long().cpu(), val.cpu())
        cross = _coalesce(torch.stack([row.long(), col.long()]), t.n).to(dev)
        parts = [s.edge_index, t.edge_index + s.n, torch.stack([cross[0], cross[1] + s.n])]
        self.within_edges = None
        if self.k_within > 0:
            added_src, val_src, _ = self._within_edges(u_src)
            added_tar, val_tar, _ = self._within_edges(u_tar)
            self.within_edges, self.within_values = (added_src, added_tar), (val_src, val_tar)
            parts += [added_src.to(dev), added_tar.to(dev) + s.n]
        n = s.n + t.n
        edge_index = _coalesce(torch.cat(parts, dim=1), n)                     # Data.coalesce()
        edge_index = _coalesce(torch.cat([edge_index, edge_index.flip(0)], dim=1), n)      # to_undirected
        central = torch.zeros(n, dtype=torch.bool, device=dev)
        central[:s.n] = True
        pad = torch.zeros(t.n, dtype=torch.bool, device=dev)
        return SimpleNamespace(x=torch.cat((s.x, t.x), dim=0), edge_index=edge_index, y=torch.cat((s.y, t.y), dim=0),
                               train_mask=torch.cat((s.train_mask, pad)), val_mask=torch.cat((s.val_mask, pad)),
                               test_mask=torch.cat((s.test_mask, pad)), central_mask=central, n=n)

    def _prepare(self, s):
        self._train_idx = torch.nonzero(s.train_mask).squeeze(1)
        self._train_y = s.y[self._train_idx]

    # -- the host fit: the reference's lines ---------------------------------------------------------------------------
    def _host_log_probs(self, x, edge_index):
        net = self.kbl.gnn
        return F.log_softmax(_host_conv(net.cls, _host_bottleneck(net, x, edge_index), edge_index), dim=1)

    def _host_fit(self, s, t, optimizer):
        start = time.time()
        self._prepare(s)
        ia_all, ib_all = self.pair_lists
        for epoch in range(self.bridge_epochs):
            parts = self._bridge_step(optimizer, s, t, ia_all[epoch], ib_all[epoch])
            self.bridge_log.append(parts.tolist())
            self._report(epoch, float(parts[0]), None, start)
        self.stored_data = merged = self._gen_bridged_graph(s, t)
        self._phase = "gnn"
        y_c = merged.y[:s.n]

        def gnn_epoch(epoch):
            self.kbl.gnn.train()
            log_probs = self._host_log_probs(merged.x, merged.edge_index)[:s.n]
            return F.nll_loss(log_probs, y_c), lambda: eval_micro_f1(y_c, log_probs.detach().argmax(dim=1))

        self._host_epochs(optimizer, gnn_epoch, start)

    # -- the device fit ------------------------------------------------------------------------------------------------
    def _device_fit(self, s, t):
        from ..epoch_graph import run_epochs
        from ..ops import dropout_state
        dev = s.x.device
        self._prepare(s)
        U, use_graph = self._slots(), self._want_hip_graph()
        ia_all, ib_all = (v.to(dev, torch.int32) for v in self.pair_lists)
        m = ia_all.size(1)
        self._slots(parts=(5,))
        self._slots(dtype=torch.int32, ia=(m,), ib=(m,))

        def stage(epoch, k):
            self._ia_buf[:k].copy_(ia_all[epoch:epoch + k])
            self._ib_buf[:k].copy_(ib_all[epoch:epoch + k])

        def record(k):
            self.bridge_log.extend(self._parts_buf[:k].tolist())

        epochs, self.epoch = self.epoch, self.bridge_epochs
        try:
            run_epochs(self, lambda u: self._bridge_epoch(s, t, u), 1, U, use_graph, before_group=stage,
                       after_group=record, also=list(self.kbl.bridged_graph.model.buffers()) + [dropout_state.counter(dev)])
        finally:
            self.epoch = epochs
        self.stored_data = merged = self._gen_bridged_graph(s, t)
        self._phase = "gnn"
        y_c = merged.y[:s.n].contiguous()
        run_epochs(self, lambda u: self._gnn_epoch(merged, s.n, y_c, u), s.n, U, use_graph,
                   also=[dropout_state.counter(dev)])

    def _bridge_epoch(self, s, t, u):
        """One bridge epoch into slot ``u``, its index lists read from the slot's buffers.  No host decision."""
        from ..ops import dropout_state
        dropout_state.next_step(s.x.device)
        parts = self._bridge_step(self.optimizer, s, t, self._ia_buf[u], self._ib_buf[u])
        self._parts_buf[u].copy_(parts)
        self._loss_buf[u].copy_(parts[0])

    def _device_log_probs(self, x, edge_index):
        """``GNNBase.forward`` on its own layers with the activation and the dropout between them in one kernel, the
        keep bits from the project's stream (``GNNBase`` itself calls torch's dropout, whose generator a capture's
        warm-up advances)."""
        from ..ops import relu_dropout
        net = self.kbl.gnn
        last = len(net.convs) - 1
        for i, conv in enumerate(net.convs):
            x = conv(x, edge_index)
            if i < last:
                x = relu_dropout(x, net.dropout, net.training)
        return F.log_softmax(net.cls(x, edge_index), dim=1)

    def _gnn_epoch(self, merged, ns, y_c, u):
        from ..ops import ce_stats_for, dropout_state, source_ce
        dropout_state.next_step(merged.x.device)
        self.kbl.gnn.train()
        log_probs = self._device_log_probs(merged.x, merged.edge_index)[:ns]
        loss = source_ce(log_probs, y_c)
        stats = ce_stats_for(log_probs, y_c)
        self._step(u, loss, hit=stats[1] if stats is not None else (log_probs.detach().argmax(dim=1) == y_c).sum())

    # -- predict -------------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(the eval-mode log-probabilities of the last data.x.shape[0] rows of the stored merged graph, data.y)``."""
        self.kbl.gnn.eval()
        merged = self.stored_data
        with torch.no_grad():
            if merged.x.is_cuda:
                log_probs = self._device_log_probs(merged.x, merged.edge_index)
            else:
                log_probs = self._host_log_probs(merged.x, merged.edge_index)
        return log_probs[-data.x.shape[0]:, ], data.y
