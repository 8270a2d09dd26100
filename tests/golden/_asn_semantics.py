"""ASN fixture support: the torch-sparse ``GCNConv`` shim the reference's global encoders need, and the drivers that run
the reference's own ``asn.py`` / ``asn_base.py`` (build container only, via ``make_golden_asn``).

SHIM (stated as the issue asks): torch_geometric is not installed, and ``_pyg_stub.GCNConv`` takes an ``edge_index``
only.  ASN feeds its global encoders the row-scaled PPMI as a ``torch.sparse_csr`` tensor.  ``GCNConv`` then takes
PyG's torch-sparse branch of ``gcn_norm`` (torch_geometric 2.3 - 2.6, ``torch_geometric/nn/conv/gcn_conv.py``):
``add_self_loops`` appends a unit loop per node and the coalesce SUMS it with an existing diagonal entry;
``deg = scatter(value, adj_t's row)``; ``value = deg^-1/2[col] * value * deg^-1/2[row]``; ``out = adj_t @ lin(x) + bias``.
The ``edge_index`` branch is the stub's (``add_remaining_self_loops``, destination degrees), with the edge weights in
the input's dtype so that the float64 run stays float64.

NUMPY 2: the reference's ``agg_tran_prob_mat`` divides a float32 array by an ``np.int64`` step (``a_k / k``), which
numpy 2 (NEP 50) promotes to float64, so its PPMI is float64 until ``sparse_mx_to_torch_sparse_tensor`` casts it to
float32.  The port computes the PPMI in float32 throughout, so entries near the ``ppmi < 0`` threshold may appear or
vanish; the fixture records the float64 matrix as well."""
import numpy as np
import torch

from . import _pyg_stub


class ShimGCNConv(_pyg_stub.GCNConv):
    def forward(self, x, edge_index, edge_weight=None):
        if edge_index.layout in (torch.sparse_csr, torch.sparse_coo):
            return self._sparse(x, edge_index)
        if edge_weight is None:
            edge_weight = torch.ones(edge_index.size(1), dtype=x.dtype)
        return super().forward(x, edge_index, edge_weight)

    def _sparse(self, x, adj_t):
        n = adj_t.size(0)
        coo = adj_t.to_sparse_coo().coalesce()
        i, j = coo.indices()
        loop = torch.arange(n)
        idx = torch.stack([torch.cat([i, loop]), torch.cat([j, loop])])
        v = torch.cat([coo.values().to(x.dtype), torch.ones(n, dtype=x.dtype)])
        a = torch.sparse_coo_tensor(idx, v, (n, n)).coalesce()            # the loop summed into the diagonal
        (r, c), v = a.indices(), a.values()
        deg = torch.zeros(n, dtype=x.dtype).index_add_(0, r, v)
        dis = deg.pow(-0.5)
        dis.masked_fill_(dis == float("inf"), 0)
        v = dis[c] * v * dis[r]
        h = self.lin(x)
        out = torch.zeros(n, h.size(1), dtype=h.dtype).index_add_(0, r, v[:, None] * h[c])
        return out + self.bias


def load_asn(ref):
    import sys
    from . import _ref_loader
    ab = _ref_loader._load("pygda.nn.asn_base", "pygda/nn/asn_base.py")
    ab.GCNConv = ShimGCNConv
    sys.modules["pygda.nn"].ASNBase = ab.ASNBase
    am = _ref_loader._load("pygda.models.asn", "pygda/models/asn.py")
    ref.ASNBase, ref.ASN, ref.GNNVAE = ab.ASNBase, am.ASN, ab.GNNVAE
    return ref


def scaled_ppmi64(m, data):
    """process_graph's matrix before the float32 cast (float64 under numpy 2), dense."""
    from scipy import sparse
    adj = _pyg_stub.to_dense_adj(data.edge_index).squeeze()
    g = sparse.csc_matrix(adj.detach().cpu().numpy())
    a = m.compute_ppmi(m.agg_tran_prob_mat(g, m.step))
    return np.asarray(m.my_scale_sim_mat(sparse.lil_matrix(a)).todense())


def run_fit(ref, s, t, kw, epochs, init_seed, dtype=torch.float32, eps_feed=None):
    """The reference's ``ASN.fit`` and both ``predict``s, with the hidden and discriminator dropout set to 0.  Records
    ``eps`` as drawn (``eps_feed`` None) or feeds the given draws.  ``dtype`` float64 runs the same lines in double:
    parameters, features and the PPMI (kept float64, not cast)."""
    import pygda.models.asn as amod
    m = ref.ASN(device="cpu", epoch=epochs, verbose=0, **kw)
    rec, log, eps = {}, [], []
    feed = list(eps_feed) if eps_feed is not None else None
    init = m.init_model

    def init_rec(**k):
        net = init(**k)
        for enc in (net.private_encoder_s_l, net.private_encoder_t_l, net.private_encoder_s_g,
                    net.private_encoder_t_g, net.shared_encoder_l, net.shared_encoder_g):
            for d in enc.dropout_layers:
                d.p = 0.0
        net.domain_model[2].p = 0.0
        rec["init"] = {k2: v.detach().numpy().copy() for k2, v in net.state_dict().items()}
        return net.to(dtype)

    def reparam(self, mu, logvar):
        if not self.training:
            return mu
        std = torch.exp(logvar)
        e = torch.randn_like(std) if feed is None else torch.as_tensor(feed.pop(0), dtype=std.dtype)
        eps.append(e.detach().to(torch.float32).numpy().copy())
        return e.mul(std).add_(mu)

    if dtype == torch.float64:
        def to_sparse64(mx):
            mx = mx.tocoo().astype(np.float64)
            idx = torch.from_numpy(np.vstack((mx.row, mx.col)).astype(np.int64))
            return torch.sparse_coo_tensor(idx, torch.from_numpy(mx.data), torch.Size(mx.shape)).coalesce().to_sparse_csr()
        m.sparse_mx_to_torch_sparse_tensor = to_sparse64
        s = _pyg_stub.Data(x=s.x.double(), edge_index=s.edge_index, y=s.y)
        t = _pyg_stub.Data(x=t.x.double(), edge_index=t.edge_index, y=t.y)
    m.init_model = init_rec
    old_rep, old_log = ref.GNNVAE.reparameterize, amod.logger
    ref.GNNVAE.reparameterize = reparam
    amod.logger = lambda **k: log.append((k["loss"], k["source_train_acc"]))
    try:
        torch.manual_seed(init_seed)
        m.fit(s, t)
        src_logits, _ = m.predict(s)
        tgt_logits, _ = m.predict(t)
    finally:
        ref.GNNVAE.reparameterize, amod.logger = old_rep, old_log
    final = {k: v.detach().double().numpy().copy() for k, v in m.asn.state_dict().items()}
    return dict(init=rec["init"], final=final, eps=eps, losses=np.array([l for l, _ in log], dtype=np.float64),
                accs=np.array([a for _, a in log], dtype=np.float64), src_logits=src_logits.detach().double().numpy(),
                tgt_logits=tgt_logits.detach().double().numpy(), ppmi_s=m.ppmi_s, ppmi_t=m.ppmi_t)
