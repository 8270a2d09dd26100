"""``JHGDA`` trainer (pygda/models/jhgda.py): Improving Graph Domain Adaptation with Network Hierarchy (CIKM-23).

Full batch only: every epoch is one forward of :class:`~pygda_amd.nn.JHGDABase` over both domains and one Adam step on
``CE_src + d_weight (g_mmd sum_i exp(-0.1 ||mean z_s - mean z_t||) + c_mmd sum_i classwise) + the five weighted pooling
sums``.  The log's loss is the epoch's loss before the step; its source micro-F1 comes from ``predict`` after it.
``lm_log`` keeps each epoch's label_matching sum (the argmax count inside the loss) beside the log.

``pseudo='gmm'`` (private, default ``'classifier'``: the reference's path) replaces the level-0 target pseudo-labels by
those of a Gaussian mixture on the target embeddings, started from the classifier's labels and assigned to the source's
class centres (the steps of ``GMMClustering.forward``; ``gmm_max_iter``, ``gmm_tol``, ``gmm_reg_covar``, and
``gmm_smooth_r`` for the 20 smoothing steps).  On the GPU the whole fit -- EM, the assignment solver, the relabelling --
is enqueued without a host read and captured with the epoch; an ill-defined fit falls back to the classifier's labels.
``gmm_log`` keeps ``(n_iter, converged, fell_back, lower_bound)`` per epoch, read once per replay.

On the GPU:
- the level-0 proximity term runs on gda_jhgda_prox_f32: loss and dS from tiles of ``S S^T`` formed on the matrix
  cores and consumed in registers, never an N x N buffer; the dense levels take the same kernel with dA as well;
- the assignment rows (relu, softmax, entropy) are one row kernel each way; every product runs on the project's GEMM
  and the level-0 products with the edge list on its SpMM;
- pseudo-labels, empty classes and argmaxes stay on the device, so ``epochs_per_graph`` (default 4) epochs are
  captured into one hipGraph and replayed; the log is read back once per replay.  Eager and captured fits are
  bit-identical.

Kept from the reference on purpose: ``predict`` is ``cls_model(gnn_emb[0](x))`` with NO activation (training applies
``act``); with ``classwise=False`` the target's TRUE labels enter the pooling; ``lm`` (label_matching) is an argmax
count, a constant in the loss; ``dropout`` is accepted and never used.
Raised before any device work: data-parallel runs (NotImplementedError), ``batch_size != 0``, ``classwise=False`` with
``pool_ratio < 1`` (the reference then indexes the label list one level off and fails), a level whose pooled width
comes out as 0, and on the GPU a level-0 width beyond ops.JHGDA_PROX_MAX_K (ValueError)."""
import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn.jhgda_base import JHGDABase, check_pseudo
from ..ops import JHGDA_PROX_MAX_K, JhgdaEdges
from .own_epoch import OwnEpochGDA, refuse_data_parallel


class JHGDA(OwnEpochGDA):
    def __init__(self, in_dim, hid_dim, num_classes, num_layers=3, dropout=0., act=F.relu, weight_decay=0.,
                 share=False, sparse=False, classwise=True, pool_ratio=0.2, g_mmd=0.5, c_mmd=0.5, d_weight=0.1,
                 ce_weight=0.1, prox_weight=0.1, cce_weight=0.1, lm_weight=0.1, ls_weight=0.1, lr=4e-3, epoch=200,
                 device='cuda:0', batch_size=0, num_neigh=-1, verbose=2, pseudo='classifier', gmm_max_iter=100,
                 gmm_tol=1e-3, gmm_reg_covar=1e-6, gmm_smooth_r=None, **kwargs):
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        if batch_size != 0:
            raise ValueError("JHGDA: only full-batch training (batch_size=0) is supported")
        if not classwise and pool_ratio < 1:
            raise ValueError("JHGDA: classwise=False needs pool_ratio >= 1 (the reference pairs level i's embeddings "
                             "with level i+1's labels and fails on the shapes)")
        check_pseudo(pseudo, classwise, hid_dim, num_classes, device)
        self.sparse, self.share, self.classwise, self.pool_ratio = sparse, share, classwise, pool_ratio
        self.pseudo, self.gmm_smooth_r = pseudo, gmm_smooth_r
        self.gmm_max_iter, self.gmm_tol, self.gmm_reg_covar = gmm_max_iter, gmm_tol, gmm_reg_covar
        self.g_mmd, self.c_mmd, self.d_weight = g_mmd, c_mmd, d_weight
        self.ce_weight, self.prox_weight, self.cce_weight = ce_weight, prox_weight, cce_weight
        self.lm_weight, self.ls_weight = lm_weight, ls_weight

    def init_model(self, **kwargs):
        return JHGDABase(in_dim=self.in_dim, hid_dim=self.hid_dim, num_classes=self.num_classes, device=self.device,
                         pool_ratio=self.pool_ratio, num_layers=self.num_layers, num_s=self.num_s, num_t=self.num_t,
                         dropout=self.dropout, act=self.act, share=self.share, sparse=self.sparse,
                         classwise=self.classwise, pseudo=self.pseudo, gmm_max_iter=self.gmm_max_iter,
                         gmm_tol=self.gmm_tol, gmm_reg_covar=self.gmm_reg_covar, gmm_smooth_r=self.gmm_smooth_r,
                         **kwargs).to(self.device)

    def process_graph(self, data):
        pass

    # -- checks --------------------------------------------------------------------------------------------------------
    def _check(self, source_data, target_data):
        refuse_data_parallel(self)
        ns, nt = source_data.x.shape[0], target_data.x.shape[0]
        ws = JHGDABase.level_widths(ns, self.pool_ratio, self.num_layers)
        wt = ws if self.share else JHGDABase.level_widths(nt, self.pool_ratio, self.num_layers)
        if min(ws + wt) < 1:
            raise ValueError(f"JHGDA: a pooling level has width 0 (source {ws}, target {wt}); raise pool_ratio or "
                             "lower num_layers")
        if torch.device(self.device).type == "cuda" and max(ws[0], wt[0]) > JHGDA_PROX_MAX_K:
            raise ValueError(f"JHGDA: the proximity kernel covers pooled widths up to {JHGDA_PROX_MAX_K}, got "
                             f"{max(ws[0], wt[0])}")
        self._check_edges(source_data, target_data)

    # -- loss ----------------------------------------------------------------------------------------------------------
    def forward_model(self, source_data, target_data, graphs=None):
        m = self.jhgda
        C = self.num_classes
        embeddings, pred, pooling_loss, label_matrix = m(
            source_data.x, source_data.edge_index, m.to_onehot(source_data.y, C),
            target_data.x, target_data.edge_index, m.to_onehot(target_data.y, C), graphs)
        if pred[0].is_cuda:
            from ..ops import source_ce
            loss = source_ce(pred[0], source_data.y)
        else:
            loss = m.loss_func(pred[0], source_data.y)
        dom, dom_c = [], []
        for i in range(self.num_layers):
            dom_c.append(m.classwise_simple_mmd(embeddings[i][0], embeddings[i][1], label_matrix[i][0],
                                                label_matrix[i][1]))
            dom.append(m.simple_mmd_kernel(embeddings[i][0], embeddings[i][1]))
        loss = loss + self.d_weight * (sum(dom) * self.g_mmd + sum(dom_c) * self.c_mmd)
        loss = loss + self.cce_weight * sum(x['cce'] for x in pooling_loss)
        lm = sum(x['lm'] for x in pooling_loss)
        self._lm = lm.detach()
        loss = loss + self.lm_weight * lm
        loss = loss + self.ls_weight * sum(x['ls'] for x in pooling_loss)
        loss = loss + self.ce_weight * sum(x['ce'] for x in pooling_loss)
        loss = loss + self.prox_weight * sum(x['prox'] for x in pooling_loss)
        return loss, pred[0], pred[1]

    # -- fit -----------------------------------------------------------------------------------------------------------
    def _graphs(self, d):
        """The device structures of one domain's level 0: the proximity kernel's edge CSRs and the unnormalised
        flipped edge graph of ``spmm`` (``out[row] += S[col]``)."""
        from ..graph import build_csr
        ei = d.edge_index
        return dict(edges=JhgdaEdges(ei, d.n),
                    spmm=build_csr(ei.flip(0).contiguous(), d.n, None, False, False, False, "col"))

    def _init_fit(self, s, t):
        self.num_s, self.num_t, self.lm_log, self.gmm_log = s.n, t.n, [], []
        self.jhgda = self.init_model(**self.kwargs)
        return self.jhgda.parameters()

    def _device_args(self, s, t):
        graphs = [self._graphs(s), self._graphs(t)]
        if self.pseudo == 'gmm' and self.gmm_smooth_r is not None:   # the smoothing step's CSR: once per fit
            from ..nn.gmm_clustering import smoothing_graph
            graphs[1]["smooth"] = smoothing_graph(t.edge_index, t.n, self.gmm_smooth_r, t.x.device)
        return (graphs,)

    def _host_epoch(self, s, t, epoch):
        self.jhgda.train()
        loss, _, _ = self.forward_model(s, t)
        self.lm_log.append(float(self._lm))
        if self.pseudo == 'gmm':
            n_iter, converged, fell_back, lower = self.jhgda.gmm_last
            self.gmm_log.append((int(n_iter), int(converged), int(fell_back), float(lower)))
        return loss, lambda: eval_micro_f1(s.y, self.predict(s)[0].argmax(dim=1))

    def _device_fit(self, s, t, graphs):
        """Epochs on the device (epoch_graph.run_epochs).  Epoch ``u`` of a replay writes its loss and its count of
        correct source predictions (``predict`` after the step) into slot ``u`` of two small buffers, read once per
        replay, and its label_matching sum into a third."""
        from ..epoch_graph import run_epochs
        U = self._slots(lm=())
        if self.pseudo == 'gmm':
            self._slots(dtype=torch.float64, gmm=(4,))

        def after_group(k):
            self.lm_log.extend(self._lm_buf[:k].tolist())
            if self.pseudo == 'gmm':
                self.gmm_log.extend((int(a), int(b >= 1), int(c), d) for a, b, c, d in self._gmm_buf[:k].tolist())

        run_epochs(self, lambda u: self._device_epoch(s, t, graphs, u), s.n, U, self._want_hip_graph(),
                   after_group=after_group)

    def _device_epoch(self, s, t, graphs, u):
        self.jhgda.train()
        loss, _, _ = self.forward_model(s, t, graphs)
        if self.pseudo == 'gmm':                                     # (n_iter, converged, failed, lower bound) of the fit
            from ..ops import gmm_state_fields
            bounds, ints = gmm_state_fields(self.jhgda.gmm_device.state)
            self._gmm_buf[u, :3].copy_(ints[0, :3])
            self._gmm_buf[u, 3].copy_(bounds[0, 0])
        self._step(u, loss, lm=self._lm)
        with torch.no_grad():
            logits = self.jhgda.inference(s)
            self._hit_buf[u].copy_((logits.argmax(dim=1) == s.y).sum())

    # -- predict -------------------------------------------------------------------------------------------------------
    def predict(self, data):
        """``(cls_model(gnn_emb[0](x)), data.y)``: no activation, as in the reference."""
        self.jhgda.eval()
        with torch.no_grad():
            logits = self.jhgda.inference(self._dom(data, torch.device(self.device)))
        return logits, data.y
