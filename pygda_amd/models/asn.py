"""``ASN`` trainer (pygda/models/asn.py): Adversarial Separation Network for cross-network node classification.

Full batch only.  ``fit`` builds each domain's global adjacency once (process_graph: ACDNE's PPMI, row-scaled, as
GCNConv's sparse adjacency) and the labels ``A + I`` of its reconstruction loss, then trains every epoch on
``cls + lambda_d grl + lambda_r (recon_s + recon_t) + lambda_f (diff_s + diff_t) + entropy * epoch / E * 0.01`` with one
Adam over all modules.  ``alpha = min((epoch + 1) / epoch_count, 0.05)`` as written.

On the GPU:
- the four first-layer projections that read one domain's ``x`` run as ONE product with the stacked weights; the mu and
  logvar heads of an encoder run as one product and one aggregation of width ``2 hid_dim_vae``;
- the reconstruction term never forms the N x N logits (ops.asn_recon_loss: one pass over the pairs);
- KLD, the reparameterisation, the decoder's dropout and DiffLoss are row kernels of csrc/gda_asn.hip; the noise and
  dropout masks come from the project's Philox, so they differ from torch's stream.  ``eps_hook(epoch)`` (a callable
  returning the eight ``eps`` tensors in the reference's encoder call order) feeds given noise instead;
- the attention heads at a width that is not a multiple of 4 run on the fused attention kernels with the views
  zero-padded to the next multiple of 4 (the padding columns score 0 and are dropped);
- ``epochs_per_graph`` (default 4) epochs are captured into one hipGraph and replayed; alpha and the entropy weight
  are device scalars, and the log (loss, source accuracy) is read back once per replay.  Eager and captured fits are
  bit-identical.

Kept from the reference on purpose: the hidden dropout is always on (also in ``predict``), ``exp(logvar)`` in the
reparameterisation, the target's KLD with ``n_nodes = 2 * nt``, the log's source micro-F1 of the epoch's pre-step logits.
Raised before any device work: data-parallel runs (NotImplementedError), ``batch_size != 0``, ``num_layers != 3``, an
``edge_index`` outside ``[0, n)`` or whose largest index is not ``n - 1`` (the reference's ``to_dense_adj`` then sizes
the labels wrongly and fails), and on the GPU a decoder width ``2 hid_dim_vae`` beyond ops.ASN_MAX_K or a
``hid_dim_vae`` beyond ops.ASN_DIFF_MAX_K (ValueError)."""
import itertools

import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn.asn_base import ASNBase
from ..ops import (ASN_DIFF_MAX_K, ASN_MAX_K, AsnLabels, asn_dropout, asn_ppmi_graph, asn_recon_loss, asn_kld,
                   asn_reparam, asn_diff_loss, softmax_entropy, source_ce, grl_mlp_ce)
from ..nn.reverse_layer import GradReverse
from .own_epoch import OwnEpochGDA, refuse_data_parallel


def _pad4(t):
    r = (-t.size(-1)) % 4
    return F.pad(t, (0, r)) if r else t


def _attention(att, a, b):
    """``att([a, b])`` on the device, zero-padded to a multiple of 4 columns for the fused kernel."""
    w, bias = att.dense_weight.weight, att.dense_weight.bias
    k = a.size(1)
    if k % 4 == 0:
        return att([a, b])
    from ..ops import attention_fuse
    return attention_fuse([_pad4(a), _pad4(b)], _pad4(w), bias)[:, :k]


class ASN(OwnEpochGDA):
    _host_dtype = torch.float32

    def __init__(self, in_dim, hid_dim, hid_dim_vae, num_classes, num_layers=3, step=3, dropout=0., act=F.relu,
                 lambda_r=1.0, lambda_d=0.1, lambda_f=0.001, adv_dim=10, weight_decay=5e-4, lr=3e-2, epoch=200,
                 device='cuda:0', batch_size=0, num_neigh=-1, verbose=2, **kwargs):
        self.eps_hook = kwargs.pop("eps_hook", None)
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        if batch_size != 0:
            raise ValueError("ASN: only full-batch training (batch_size=0) is supported, as in the reference")
        if num_layers != 3:
            raise ValueError("ASN: num_layers must be 3 (GNNVAE asserts it)")
        self.hid_dim_vae, self.adv_dim = hid_dim_vae, adv_dim
        self.lambda_r, self.lambda_d, self.lambda_f = lambda_r, lambda_d, lambda_f
        self.step = step
        self._ppmi_cache = {}

    def init_model(self, **kwargs):
        return ASNBase(in_dim=self.in_dim, hid_dim=self.hid_dim, hid_dim_vae=self.hid_dim_vae,
                       num_classes=self.num_classes, num_layers=self.num_layers, dropout=self.dropout, act=self.act,
                       adv_dim=self.adv_dim, **kwargs).to(self.device)

    def forward_model(self, source_data, target_data):
        pass

    # -- checks and preprocessing --------------------------------------------------------------------------------------
    def _check(self, *datas):
        refuse_data_parallel(self)
        cuda = torch.device(self.device).type == "cuda"
        if cuda and 2 * self.hid_dim_vae > ASN_MAX_K:
            raise ValueError(f"ASN: the reconstruction kernel covers decoder widths up to {ASN_MAX_K} "
                             f"(hid_dim_vae <= {ASN_MAX_K // 2}), got hid_dim_vae = {self.hid_dim_vae}")
        if cuda and self.hid_dim_vae > ASN_DIFF_MAX_K:
            raise ValueError(f"ASN: DiffLoss covers hid_dim_vae <= {ASN_DIFF_MAX_K} on the device")
        for d in datas:
            self._check_edges(d, empty_ok=False)
            n, ei = d.x.shape[0], d.edge_index
            if int(ei.max()) + 1 != n:
                raise ValueError(f"ASN: edge_index.max() + 1 = {int(ei.max()) + 1} but the graph has {n} nodes: the "
                                 "reference's to_dense_adj sizes the adjacency by the largest index and fails")

    def process_graph(self, data):
        """The global encoders' adjacency (normalised PPMI): a CSRGraph on the device, a dense matrix on the host.
        Cached per (edge_index storage, version, n, step)."""
        ei = data.edge_index.to(self.device)
        key = (data.edge_index.data_ptr(), data.edge_index._version, data.x.shape[0], self.step, str(ei.device))
        hit = self._ppmi_cache.get(key)
        if hit is None:
            hit = self._ppmi_cache[key] = asn_ppmi_graph(ei, data.x.shape[0], self.step)
        return hit

    # -- fit ---------------------------------------------------------------------------------------------------------
    def _init_fit(self, s, t):
        self.num_source_nodes, self.num_target_nodes = s.n, t.n
        self.asn = self.init_model(**self.kwargs)
        return itertools.chain(*[m.parameters() for m in self.asn.models])

    def _host_epoch(self, s, t, epoch):
        alpha = min((epoch + 1) / self.epoch, 0.05)
        for m in self.asn.models:
            m.train()
        eps = self.eps_hook(epoch) if self.eps_hook is not None else [None] * 8
        loss, source_logits = self._host_loss(s, t, alpha, epoch / self.epoch * 0.01, eps)
        return loss, lambda: eval_micro_f1(s.y, source_logits.detach().argmax(dim=1))

    def _device_fit(self, s, t):
        """Epochs on the device (epoch_graph.run_epochs).  Each epoch writes its loss and its count of correct source
        predictions into slot ``u`` of small device buffers and reads alpha and the entropy weight from slot ``u`` of
        two more, so that ``epochs_per_graph`` epochs can be captured into one hipGraph and replayed; the host reads the
        buffers once per replay (the log runs one replay behind the device work).  With ``eps_hook`` set, or the graph
        off, every epoch runs eagerly through the same slots.  The capture's warm-up epoch is rolled back with the
        Philox step counter, so the fit takes exactly the eager epochs."""
        from ..epoch_graph import run_epochs
        from ..ops import dropout_state
        U = self._slots(alpha=(), went=())
        eps = [None] * 8      # rebound by schedule() ahead of each eager epoch; the lambda below reads it at call time

        def schedule(epoch, k):
            nonlocal eps
            sched = [(min((e + 1) / self.epoch, 0.05), e / self.epoch * 0.01) for e in range(epoch, epoch + k)]
            self._alpha_buf[:k].copy_(torch.tensor([a for a, _ in sched], dtype=torch.float32), non_blocking=True)
            self._went_buf[:k].copy_(torch.tensor([w for _, w in sched], dtype=torch.float32), non_blocking=True)
            if self.eps_hook is not None:
                eps = self.eps_hook(epoch)

        run_epochs(self, lambda u: self._device_epoch(s, t, u, eps), s.n, U,
                   self.eps_hook is None and self._want_hip_graph(), before_group=schedule,
                   also=[dropout_state.counter(torch.device(self.device))])

    def _device_epoch(self, s, t, u, eps):
        from ..ops import dropout_state
        dropout_state.next_step(torch.device(self.device))
        for m in self.asn.models:
            m.train()
        loss, source_logits = self._device_loss(s, t, self._alpha_buf[u], self._went_buf[u], eps)
        self._step(u, loss, hit=lambda: (source_logits.detach().argmax(dim=1) == s.y).sum())

    def _dom(self, data, dev):
        d = super()._dom(data, dev)
        d.ppmi, d.labels = self.process_graph(data), AsnLabels(d.edge_index, d.n)
        return d

    def _host_loss(self, s, t, alpha, went, eps):
        """The reference's epoch, line by line (host tensors)."""
        a = self.asn
        rec_s, mu_s, lv_s = a.private_encoder_s_l(s.x, s.edge_index, eps[0])
        rec_t, mu_t, lv_t = a.private_encoder_t_l(t.x, t.edge_index, eps[1])
        rec_s_p, mu_s_p, lv_s_p = a.private_encoder_s_g(s.x, s.ppmi, eps[2])
        rec_t_p, mu_t_p, lv_t_p = a.private_encoder_t_g(t.x, t.ppmi, eps[3])
        z_s, sh_s1, sh_s2 = a.shared_encoder_l(s.x, s.edge_index, eps[4])
        z_t, sh_t1, sh_t2 = a.shared_encoder_l(t.x, t.edge_index, eps[5])
        z_s_p, pp_s1, pp_s2 = a.shared_encoder_g(s.x, s.ppmi, eps[6])
        z_t_p, pp_t1, pp_t2 = a.shared_encoder_g(t.x, t.ppmi, eps[7])
        enc_s = a.att_model([sh_s1, pp_s1])
        enc_t = a.att_model([sh_t1, pp_t1])
        diff = a.loss_diff(mu_s, sh_s1) + a.loss_diff(mu_t, sh_t1)
        zc_s = torch.cat((a.att_model_self_s([rec_s, rec_s_p]), a.att_model_self_s([z_s, z_s_p])), 1)
        zc_t = torch.cat((a.att_model_self_t([rec_t, rec_t_p]), a.att_model_self_t([z_t, z_t_p])), 1)
        zc_s = F.dropout(zc_s, a.decoder_s.dropout, training=a.decoder_s.training)
        zc_t = F.dropout(zc_t, a.decoder_t.dropout, training=a.decoder_t.training)
        mu_cat_s = torch.cat((mu_s, mu_s_p, sh_s1, pp_s1), 1)
        mu_cat_t = torch.cat((mu_t, mu_t_p, sh_t1, pp_t1), 1)
        lv_cat_s = torch.cat((lv_s, lv_s_p, sh_s2, pp_s2), 1)
        lv_cat_t = torch.cat((lv_t, lv_t_p, sh_t2, pp_t2), 1)
        recon = (a.recon_loss_fused(zc_s, s.labels, mu_cat_s, lv_cat_s, s.n)
                 + a.recon_loss_fused(zc_t, t.labels, mu_cat_t, lv_cat_t, t.n * 2))
        source_logits = a.cls_model(enc_s)
        cls = a.cls_loss(source_logits, s.y)
        d_s = a.domain_model(GradReverse.apply(enc_s, alpha))
        d_t = a.domain_model(GradReverse.apply(enc_t, alpha))
        grl = (a.cls_loss(d_s, torch.zeros(d_s.size(0), dtype=torch.int64))
               + a.cls_loss(d_t, torch.ones(d_t.size(0), dtype=torch.int64)))
        target_logits = a.cls_model(enc_t)
        p = torch.clamp(F.softmax(target_logits, dim=-1), min=1e-9, max=1.0)
        ent = torch.mean(torch.sum(-p * torch.log(p), dim=-1))
        loss = (cls + self.lambda_d * grl + self.lambda_r * recon + self.lambda_f * diff
                + ent * went)
        return loss, source_logits

    # -- device path ---------------------------------------------------------------------------------------------------
    def _encode(self, x, encs, graphs, eps, hidden=True):
        """The first layer of every encoder in ``encs`` that reads ``x`` as one product with the stacked weights, then
        per encoder the aggregation, ReLU + hidden dropout, and the mu / logvar heads as one product and one
        aggregation.  Returns ``[(z, mu, logvar)]`` (z = mu when ``eps`` is False)."""
        from ..nn.linear import _TallLinear
        from ..ops import propagate, relu_dropout
        hid, vae = self.hid_dim, self.hid_dim_vae
        W0 = torch.cat([e.conv_layers[0].lin.weight for e in encs], 0)
        H = _TallLinear.apply(x, W0)
        out = []
        for k, (e, g) in enumerate(zip(encs, graphs)):
            h = propagate(H[:, k * hid:(k + 1) * hid].contiguous(), g, 1, e.conv_layers[0].bias)
            h = relu_dropout(h, e.dropout_layers[0].p, True) if self.act is F.relu else \
                F.dropout(self.act(h), e.dropout_layers[0].p)
            Wh = torch.cat([e.conv_layers[1].lin.weight, e.conv_layers[2].lin.weight], 0)
            bh = torch.cat([e.conv_layers[1].bias, e.conv_layers[2].bias], 0)
            o = propagate(_TallLinear.apply(h, Wh), g, 1, bh)
            mu, lv = o[:, :vae].contiguous(), o[:, vae:].contiguous()
            z = mu if eps is False else asn_reparam(mu, lv, eps[k])
            out.append((z, mu, lv))
        return out

    def _graph_l(self, d):
        return self.asn.shared_encoder_l.conv_layers[0]._graph(d.x, d.edge_index, None)

    def _device_loss(self, s, t, alpha, went, eps):
        a = self.asn
        gs, gt = self._graph_l(s), self._graph_l(t)
        # encoder call order of the reference: s_l, t_l, s_g, t_g, shared_l (s, t), shared_g (s, t)
        (rec_s, mu_s, lv_s), (rec_s_p, mu_s_p, lv_s_p), (z_s, sh_s1, sh_s2), (z_s_p, pp_s1, pp_s2) = self._encode(
            s.x, [a.private_encoder_s_l, a.private_encoder_s_g, a.shared_encoder_l, a.shared_encoder_g],
            [gs, s.ppmi, gs, s.ppmi], [eps[0], eps[2], eps[4], eps[6]])
        (rec_t, mu_t, lv_t), (rec_t_p, mu_t_p, lv_t_p), (z_t, sh_t1, sh_t2), (z_t_p, pp_t1, pp_t2) = self._encode(
            t.x, [a.private_encoder_t_l, a.private_encoder_t_g, a.shared_encoder_l, a.shared_encoder_g],
            [gt, t.ppmi, gt, t.ppmi], [eps[1], eps[3], eps[5], eps[7]])
        enc_s = _attention(a.att_model, sh_s1, pp_s1)
        enc_t = _attention(a.att_model, sh_t1, pp_t1)
        diff = asn_diff_loss(mu_s, sh_s1) + asn_diff_loss(mu_t, sh_t1)
        zc_s = torch.cat((_attention(a.att_model_self_s, rec_s, rec_s_p), _attention(a.att_model_self_s, z_s, z_s_p)), 1)
        zc_t = torch.cat((_attention(a.att_model_self_t, rec_t, rec_t_p), _attention(a.att_model_self_t, z_t, z_t_p)), 1)
        zc_s = asn_dropout(zc_s.contiguous(), a.decoder_s.dropout)
        zc_t = asn_dropout(zc_t.contiguous(), a.decoder_t.dropout)
        mu_cat_s = torch.cat((mu_s, mu_s_p, sh_s1, pp_s1), 1)
        mu_cat_t = torch.cat((mu_t, mu_t_p, sh_t1, pp_t1), 1)
        lv_cat_s = torch.cat((lv_s, lv_s_p, sh_s2, pp_s2), 1)
        lv_cat_t = torch.cat((lv_t, lv_t_p, sh_t2, pp_t2), 1)
        recon = (asn_recon_loss(zc_s, s.labels) + asn_kld(mu_cat_s, lv_cat_s, s.n)
                 + asn_recon_loss(zc_t, t.labels) + asn_kld(mu_cat_t, lv_cat_t, t.n * 2))
        source_logits = a.cls_model(enc_s)
        cls = source_ce(source_logits, s.y)
        W1, b1 = a.domain_model[0].weight, a.domain_model[0].bias
        W2, b2 = a.domain_model[3].weight, a.domain_model[3].bias
        grl = grl_mlp_ce(enc_s, enc_t, W1, b1, W2, b2, alpha, dropout_p=a.domain_model[2].p)
        target_logits = a.cls_model(enc_t)
        ent = softmax_entropy(target_logits)
        loss = (cls + self.lambda_d * grl + self.lambda_r * recon + self.lambda_f * diff
                + ent * went)
        return loss, source_logits

    # -- predict -------------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(classifier logits, data.y)`` from the shared encoders' ``mu`` (no noise; the hidden dropout stays on)."""
        self._check(data)
        for m in self.asn.models:
            m.eval()
        dev = torch.device(self.device)
        ppmi = self.process_graph(data)
        d = super()._dom(data, dev)
        x, a = d.x, self.asn
        with torch.no_grad():
            if dev.type == "cuda":
                from ..ops import dropout_state
                dropout_state.next_step(dev)
                (_, sh1, _), (_, pp1, _) = self._encode(x, [a.shared_encoder_l, a.shared_encoder_g],
                                                        [self._graph_l(d), ppmi], False)
                logits = a.cls_model(_attention(a.att_model, sh1, pp1))
            else:
                _, sh1, _ = a.shared_encoder_l(x, data.edge_index)
                _, pp1, _ = a.shared_encoder_g(x, ppmi)
                logits = a.cls_model(a.att_model([sh1, pp1]))
        return logits, data.y
