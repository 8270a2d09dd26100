"""``DGDA`` trainer (pygda/models/dgda.py): Graph Domain Adaptation, A Generative View.

Full batch only.  Every epoch takes TWO optimiser steps with one Adam: the plain pass on ``A + I`` of both domains, then
the "manipulated" pass on the adjacency ``drop_edges`` returns.  The logged loss and source accuracy are the plain
pass's.  ``alpha = 2 / (1 + exp(-10 epoch / E)) - 1``.

``drop_edges`` draws both masks with ``torch.bernoulli(adj, p=...)``, where ``p`` overrides ``adj``: the masks are
Bernoulli draws over all N^2 pairs, so the manipulated adjacency is about ``add_rate`` dense whatever the graph.  On
the GPU it is one bit per pair (ops.DgdaBits, csrc/gda_dgda.hip): built by gda_dgda_manip_bits from the project's
Philox, aggregated by a GEMM over the nodes on the 16-bit matrix cores (ops.dgda_bit_propagate; the 0/1 operand is
expanded in registers, the features enter as three bf16 terms) and read as labels by the all-pairs reconstruction
kernel (ops.dgda_recon_loss).  No ``[N, N]`` float array exists.  The plain pass runs ``propagate`` on the CSR of
``D^-1/2 (A + I) D^-1/2`` and the ASN operators (reparameterisation, KLD, reconstruction).  The three heads ``d_gnn2``,
``y_gnn2``, ``m_gnn2`` run as one projection and one aggregation of width ``2 (d + y + m)``; the two ``x`` blocks of
``gnn0.weight`` are folded into one product (both receive their gradient).  ``epochs_per_graph`` (default 4) epochs
are captured into one hipGraph with alpha in a device slot; eager and captured fits are bit-identical, the capture's
warm-up epoch is rolled back with the Philox step.

Kept from the reference on purpose (the fixture ``dgda_fit3.npz`` shows each):
- the encoder mutates its adjacency argument in place (``adj += I``), so the losses see ``A + I`` in the first pass
  (``n_edges = E + N``) and ``nadj + I`` -- diagonal 2 -- in the second;
- ``kl_loss`` divides by ``mu.shape[1]`` (the latent width, not the node count);
- every domain's loss is clamped at 0, and so is the reconstruction term;
- the second pass calls ``DGDA_loss`` with ``manipulate=False``: ``m_recons`` and ``dadj`` are never used, the noise
  decoder and the graph discriminator never receive a gradient;
- the encoder's input is ``cat(x, emb, x)`` (the vertex-feature table is ``x`` again);
- ``predict`` ignores its argument's graph and uses the stored target adjacency, which gains another ``I`` at every
  call (``A + 2 I`` at the first, ``A + 3 I`` at the second ...);
- a duplicate edge survives its drop (``adj - drop > 0``).

Hooks for tests: ``eps_hook(epoch)`` returns the 12 noise tensors of an epoch in call order (per pass: source d, y, m,
target d, y, m), ``manip_hook(epoch)`` the two dense ``nadj`` (source, target), ``pretrained_emb=(emb_s, emb_t)`` skips
DeepWalk.  The device noise and masks come from Philox, so they differ from torch's stream.

Raised before any device work: ``batch_size != 0`` and an ``edge_index`` whose largest index is not ``N - 1``
(ValueError), data-parallel runs (NotImplementedError), and on the GPU a ``dec_dim`` beyond ops.DGDA_MAX_K or a head
width beyond ops.DGDA_MAX_C (ValueError)."""
import math
import time

import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn.dgda_base import DGDABase
from ..nn.reverse_layer import GradReverse
from ..ops import (DGDA_MAX_C, DGDA_MAX_K, DGDA_MAX_N, AsnLabels, DgdaBits, asn_kld, asn_recon_loss, asn_reparam,
                   dgda_bit_propagate, dgda_manip_bits, dgda_manip_host, dgda_norm_graph, dgda_p_add, dgda_pack_bits,
                   dgda_recon_loss, source_ce)
from .own_epoch import OwnEpochGDA, refuse_data_parallel


def max_entropy(x):
    return 0.693148 + torch.mean(torch.sigmoid(x) * F.logsigmoid(x))


def dense_adj(edge_index, n):
    """``to_dense_adj(edge_index).squeeze()``: the edge counts, float32."""
    adj = torch.zeros(n, n, dtype=torch.float32, device=edge_index.device)
    adj.index_put_((edge_index[0], edge_index[1]), torch.ones(edge_index.size(1), device=edge_index.device),
                   accumulate=True)
    return adj


class DGDA(OwnEpochGDA):
    _host_dtype = torch.float32

    def __init__(self, in_dim, hid_dim, num_classes, num_layers=3, dropout=0., act=F.relu, dec_dim=64, d_dim=64,
                 y_dim=256, m_dim=128, recons_w=1.0, beta=0.5, ent_w=1.0, d_w=1.0, y_w=1.0, m_w=0.1,
                 edge_drop_rate=0.1, edge_add_rate=0.1, weight_decay=5e-4, lr=0.001, epoch=400, device='cuda:0',
                 batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        self.eps_hook = kwargs.pop("eps_hook", None)
        self.manip_hook = kwargs.pop("manip_hook", None)
        self.pretrained_emb = kwargs.pop("pretrained_emb", None)
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        if batch_size != 0:
            raise ValueError("DGDA: only full-batch training (batch_size=0) is supported")
        self.dec_dim, self.y_dim, self.d_dim, self.m_dim = dec_dim, y_dim, d_dim, m_dim
        self.recons_w, self.ent_w, self.beta, self.d_w, self.y_w, self.m_w = recons_w, ent_w, beta, d_w, y_w, m_w
        self.edge_add_rate, self.edge_drop_rate = edge_add_rate, edge_drop_rate

    def init_model(self, **kwargs):
        return DGDABase(in_dim=self.in_dim, num_class=self.num_classes, enc_hs=self.hid_dim, dec_hs=self.dec_dim,
                        dim_d=self.d_dim, dim_y=self.y_dim, dim_m=self.m_dim, droprate=self.dropout, backbone='gcn',
                        source_pretrained_emb=self.source_pretrained_emb, source_vertex_feats=self.source_data.x,
                        target_pretrained_emb=self.target_pretrained_emb, target_vertex_feats=self.target_data.x,
                        **kwargs).to(self.device)

    def forward_model(self, source_data, target_data):
        pass

    def process_graph(self, data):
        pass

    # -- checks ------------------------------------------------------------------------------------------------------
    def _check(self, *datas):
        refuse_data_parallel(self)
        if torch.device(self.device).type == "cuda":
            if self.dec_dim > DGDA_MAX_K:
                raise ValueError(f"DGDA: the reconstruction kernel covers dec_dim <= {DGDA_MAX_K}, got {self.dec_dim}")
            if 2 * (self.d_dim + self.y_dim + self.m_dim) > DGDA_MAX_C or self.hid_dim > DGDA_MAX_C:
                raise ValueError(f"DGDA: the bit-adjacency GEMM covers widths up to {DGDA_MAX_C}")
        for d in datas:
            self._check_edges(d, empty_ok=False)
            n = d.x.shape[0]
            if int(d.edge_index.max()) + 1 != n:
                raise ValueError(f"DGDA: edge_index.max() + 1 = {int(d.edge_index.max()) + 1} but the graph has {n} "
                                 "nodes: the reference's to_dense_adj sizes the adjacency by the largest index")
            if n > DGDA_MAX_N:
                raise ValueError(f"DGDA: the bit adjacency covers N <= {DGDA_MAX_N}, got {n}")

    def _dom(self, data, dev):
        d = super()._dom(data, dev)
        d.vts = torch.arange(d.n, device=dev)
        if dev.type == "cuda":
            d.labels = AsnLabels(d.edge_index, d.n)
            s = torch.tensor(float(d.edge_index.size(1) + d.n), dtype=torch.float32)     # (A + I).sum()
            nn_ = d.n * d.n
            d.labels.pos_weight = float((nn_ - s) / s)
            d.labels.norm = float(nn_ / ((nn_ - s) * 2))
            dgda_p_add(d.labels, self.edge_add_rate)                                     # caches the edge count
            d.graph = dgda_norm_graph(d.labels, 1)
            d.bits = DgdaBits(d.n, dev)
        return d

    # -- fit ---------------------------------------------------------------------------------------------------------
    def _init_fit(self, s, t):
        self.num_source_nodes, self.num_target_nodes = s.n, t.n
        dev = torch.device(self.device)
        if self.pretrained_emb is not None:
            emb_s, emb_t = self.pretrained_emb
        else:
            from ..nn.deepwalk_pretrain import DWPretrain
            emb = []
            for name, d in (("Source", s), ("Target", t)):
                if self.verbose > 1:
                    print(f"{name} data pretraining...")
                pre = DWPretrain(d, verbose=self.verbose > 1)
                pre.fit()
                emb.append(pre.get_embedding().detach())
            emb_s, emb_t = emb
        self.source_pretrained_emb = emb_s.detach().to(dev, torch.float32).contiguous()
        self.target_pretrained_emb = emb_t.detach().to(dev, torch.float32).contiguous()
        self.source_data, self.target_data = s, t
        self.dgda = self.init_model(**self.kwargs)
        self._s, self._t, self._t_loops = s, t, 1
        return [p for p in self.dgda.parameters() if p.requires_grad]

    def _alpha(self, epoch):
        return 2. / (1. + math.exp(-10. * float(epoch) / self.epoch)) - 1

    # -- host path: the reference's lines -------------------------------------------------------------------------
    def recons_loss(self, recons, adjs):
        total = recons.shape[0] * recons.shape[1]
        n_edges = adjs.sum()
        pos_weight = torch.zeros(()) if n_edges == 0 else float(total - n_edges) / n_edges
        norm = float(total) / (2 * (total - n_edges))
        rl = norm * F.binary_cross_entropy_with_logits(input=recons, target=adjs, pos_weight=pos_weight)
        return torch.maximum(rl, torch.zeros_like(rl))

    @staticmethod
    def kl_loss(mu, lv):
        return -0.5 / mu.shape[1] * torch.mean(torch.sum(1 + 2 * lv - mu.pow(2) - lv.exp().pow(2), dim=-1))

    def DGDA_loss(self, res, labels, adj, domain):
        recon = self.recons_w * self.recons_loss(res['a_recons'], adj)
        kld = (self.kl_loss(res['dmu'], res['dlv']) + self.kl_loss(res['ymu'], res['ylv'])
               + self.kl_loss(res['mmu'], res['mlv']))
        ent = max_entropy(res['d']) + max_entropy(res['y']) + max_entropy(res['m'])
        if domain == 0:
            class_loss = F.cross_entropy(input=res['cls_output'], target=labels)
            dom_labels = torch.zeros_like(labels).float()
        else:
            class_loss = torch.zeros(())
            dom_labels = torch.ones_like(labels).float()
        dom = F.binary_cross_entropy_with_logits(input=res['dom_output'].view(-1), target=dom_labels)
        loss = recon + self.beta * kld + self.y_w * class_loss + self.d_w * dom + self.ent_w * ent
        return torch.maximum(loss, torch.zeros_like(loss))

    def drop_edges(self, adj, drop_rate=0.0, add_rate=0.0):
        """``nadj`` of the reference's drop_edges on the host (its two ``torch.bernoulli(adj, p=...)`` draws in the same
        order), through the bit rule."""
        n = adj.shape[1]
        sparsity = (adj.sum() + n * n) / (n * n)
        drop = torch.bernoulli(adj, p=drop_rate) if drop_rate > 0.0 else torch.zeros_like(adj)
        add = torch.bernoulli(adj, p=float(sparsity * add_rate)) if add_rate > 0.0 else torch.zeros_like(adj)
        return dgda_manip_host(adj, drop, add)

    def _host_pass(self, s, t, s_adj, t_adj, alpha, eps):
        s_out = self.dgda(s.x, s.vts, s_adj, 0, alpha=alpha, eps=eps[0:3])
        t_out = self.dgda(t.x, t.vts, t_adj, 1, alpha=alpha, eps=eps[3:6])
        return self.DGDA_loss(s_out, s.y, s_adj, 0) + self.DGDA_loss(t_out, t.y, t_adj, 1), s_out['cls_output']

    def _host_fit(self, s, t, optimizer):
        start = time.time()
        for epoch in range(self.epoch):
            alpha = self._alpha(epoch)
            s_adj, t_adj = dense_adj(s.edge_index, s.n), dense_adj(t.edge_index, t.n)
            self.t_adj = t_adj
            eps = self.eps_hook(epoch) if self.eps_hook is not None else [None] * 12
            self.dgda.train()
            loss, logits = self._host_pass(s, t, s_adj, t_adj, alpha, eps[0:6])       # s_adj, t_adj are A + I from here
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            preds = logits.detach().argmax(dim=1)
            if self.manip_hook is not None:
                s_nadj, t_nadj = (a.clone() for a in self.manip_hook(epoch))
            else:
                s_nadj = self.drop_edges(s_adj, self.edge_drop_rate, self.edge_add_rate)
                t_nadj = self.drop_edges(t_adj, self.edge_drop_rate, self.edge_add_rate)
            optimizer.zero_grad()
            mn_loss, _ = self._host_pass(s, t, s_nadj, t_nadj, alpha, eps[6:12])
            mn_loss.backward()
            optimizer.step()
            self._report(epoch, loss.item(), eval_micro_f1(s.y, preds), start)

    # -- device path -------------------------------------------------------------------------------------------------
    def _device_fit(self, s, t):
        from ..epoch_graph import run_epochs
        from ..ops import dropout_state
        U = self._slots(alpha=())
        fed = dict(eps=[None] * 12, nadj=None)      # rebound by schedule() ahead of each eager epoch

        def schedule(epoch, k):
            self._alpha_buf[:k].copy_(torch.tensor([self._alpha(e) for e in range(epoch, epoch + k)],
                                                   dtype=torch.float32), non_blocking=True)
            if self.eps_hook is not None:
                fed["eps"] = self.eps_hook(epoch)
            if self.manip_hook is not None:
                fed["nadj"] = self.manip_hook(epoch)

        eager = self.eps_hook is not None or self.manip_hook is not None
        run_epochs(self, lambda u: self._device_epoch(s, t, u, fed["eps"], fed["nadj"]), s.n, U,
                   not eager and self._want_hip_graph(), before_group=schedule,
                   also=[dropout_state.counter(torch.device(self.device))])

    def _device_epoch(self, s, t, u, eps, nadj):
        from ..ops import dropout_state, propagate
        dropout_state.next_step(torch.device(self.device))
        self.dgda.train()
        alpha = self._alpha_buf[u]
        plain = [(lambda h, b, g=d.graph: propagate(h, g, 1, b), lambda z, l=d.labels: asn_recon_loss(z, l))
                 for d in (s, t)]
        loss, logits = self._device_pass(s, t, plain, alpha, eps[0:6])
        self._step(u, loss, hit=lambda: (logits.detach().argmax(dim=1) == s.y).sum())
        if nadj is None:
            dgda_manip_bits(s.labels, self.edge_drop_rate, self.edge_add_rate, out=s.bits)
            dgda_manip_bits(t.labels, self.edge_drop_rate, self.edge_add_rate, out=t.bits)
        else:
            dgda_pack_bits(nadj[0], out=s.bits)
            dgda_pack_bits(nadj[1], out=t.bits)
        manip = [(lambda h, b, m=d.bits: dgda_bit_propagate(h, m, b), lambda z, m=d.bits: dgda_recon_loss(z, m))
                 for d in (s, t)]
        mn_loss, _ = self._device_pass(s, t, manip, alpha, eps[6:12])
        self.optimizer.zero_grad(set_to_none=True)
        mn_loss.backward()
        self.optimizer.step()

    def _device_pass(self, s, t, fns, alpha, eps):
        ls, logits = self._device_domain(s, 0, *fns[0], alpha, eps[0:3])
        lt, _ = self._device_domain(t, 1, *fns[1], alpha, eps[3:6])
        return ls + lt, logits

    def _encode(self, d, domain, agg, eps):
        """The encoder on the device: ``[(z, mu, lv)]`` for d, y, m (z = mu in eval) -- the two ``x`` blocks of
        ``gnn0.weight`` as one product, the three heads as one projection and one aggregation."""
        from ..nn.linear import tall_matmul
        from ..ops import relu_dropout
        net, enc = self.dgda, self.dgda.encoder
        emb = (net.semb if domain == 0 else net.temb).weight
        f, e = net.feat_dim, emb.size(1)
        W0, p, training = enc.gnn0.weight, enc.dropout.p, enc.training
        h = tall_matmul(d.x, W0[:f] + W0[f + e:]) + tall_matmul(emb, W0[f:f + e])
        h = relu_dropout(agg(h, enc.gnn0.bias), p, training)
        h = relu_dropout(agg(tall_matmul(h, enc.gnn1.weight), enc.gnn1.bias), p, training)
        heads = (enc.d_gnn2, enc.y_gnn2, enc.m_gnn2)
        o = agg(tall_matmul(h, torch.cat([c.weight for c in heads], 1)), torch.cat([c.bias for c in heads]))
        out, at = [], 0
        for k, w in enumerate(enc.dims):
            mu, lv = o[:, at:at + w].contiguous(), o[:, at + w:at + 2 * w].contiguous()
            at += 2 * w
            out.append((asn_reparam(mu, lv, eps[k]) if training else mu, mu, lv))
        return out

    def _classify(self, y):
        from ..ops import relu_dropout
        c = self.dgda.classClassifier
        return c.lin1(relu_dropout(c.lin0(y), c.dropout.p, c.training))

    def _device_domain(self, d, domain, agg, recon, alpha, eps):
        from ..ops import relu_dropout
        net = self.dgda
        (zd, dmu, dlv), (zy, ymu, ylv), (zm, mmu, mlv) = self._encode(d, domain, agg, eps)
        dec = net.graph_decoder
        p, training = dec.dropout.p, dec.training
        dym = dec.dym_lin1(torch.cat([relu_dropout(dec.d_lin0(zd), p, training),
                                      relu_dropout(dec.y_lin0(zy), p, training),
                                      relu_dropout(dec.m_lin0(zm), p, training)], dim=-1))
        rec = self.recons_w * torch.clamp(recon(dym), min=0)
        kld = (asn_kld(dmu, dlv, dmu.size(1)) + asn_kld(ymu, ylv, ymu.size(1)) + asn_kld(mmu, mlv, mmu.size(1)))
        ent = max_entropy(zd) + max_entropy(zy) + max_entropy(zm)
        dom_logit = net.domainClassifier(GradReverse.apply(zd, alpha)).view(-1)
        dom = F.binary_cross_entropy_with_logits(dom_logit, torch.full_like(dom_logit, float(domain)))
        loss = rec + self.beta * kld + self.d_w * dom + self.ent_w * ent
        logits = None
        if domain == 0:
            logits = self._classify(zy)
            loss = loss + self.y_w * source_ce(logits, d.y)
        return torch.clamp(loss, min=0), logits

    # -- predict -----------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(classifier logits, data.y)``.  As in the reference the graph is the STORED target's: its adjacency gains
        another ``I`` with every call."""
        self.dgda.eval()
        t = self._t
        with torch.no_grad():
            if torch.device(self.device).type == "cuda":
                from ..ops import propagate
                self._t_loops += 1
                g = dgda_norm_graph(t.labels, self._t_loops)
                (_, _, _), (zy, _, _), _ = self._encode(t, 1, lambda h, b: propagate(h, g, 1, b), None)
                logits = self._classify(zy)
            else:
                logits = self.dgda(t.x, t.vts, self.t_adj, 1, recon=False)['cls_output']
        return logits, data.y
