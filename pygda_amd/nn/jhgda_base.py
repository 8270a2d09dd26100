"""``JHGDABase`` / ``GCNPooling`` (pygda/nn/jhgda_base.py): a GCN stack whose levels are coarsened by learned soft
assignments (DiffPool-style), with the pooling losses of JHGDA.  Same constructor signatures, module names, state dict
keys and init RNG stream as the reference: ``gnn_emb`` (GCNConv per level), ``gnn_pool`` (``share=True``) or
``gnn_pool_src`` / ``gnn_pool_tgt`` (GCNPooling per level, ``.gcn`` inside), ``cls_model`` (``Sequential(Linear)``),
built in that order.

Level i of one domain (``forward``):
- ``z = act(gnn_emb[i](x, graph))``: level 0 on the input edge list with unit weights, levels >= 1 on the dense pooled
  adjacency ``A_i`` as PyG's ``gcn_norm`` treats the complete graph ``adj2coo`` lists -- the diagonal weights kept, the
  degree the column sum: ``out = Ahat^T (x W^T) + b``, ``Ahat = D^-1/2 A D^-1/2`` (a zero degree gives 0);
- ``S = softmax(relu(pool.gcn(x, graph)))`` (one-hot of its argmax with ``sparse``), ``X_new = S^T z``,
  ``Yp_new = softmax(S^T Y_old)``, ``Y_new = onehot(argmax Yp_new)``, ``A_{i+1} = (A S)^T S`` (level 0, the edge list)
  or ``S^T A_i S``;
- the losses ``ce`` (row entropy of S), ``prox`` (proximity_loss), ``cce`` (entropy of Yp_new), ``lm``
  (label_matching: argmax only, a constant) and ``ls`` (label_stable), each the mean of the two domains.

Host tensors run these lines as the reference writes them; device tensors run them on the project's kernels:
the GCN layers on the GEMM + SpMM of GCNConv (the dense levels on the GEMM), every product (``S^T z``, ``S^T Y``,
``(A S)^T S``, ``S^T A S``, the class sums) on the GEMM, the assignment rows and their entropy on
``gda_jhgda_pool_rows_*``, and the proximity loss on ``gda_jhgda_prox_f32`` (no N x N buffer).  The levels' A_{L}
and X_new after the last level are not formed (they feed nothing)."""
import torch
import torch.nn.functional as F
from torch import nn

from ..ops import jhgda_pool_rows, jhgda_prox, mat_tn
from .gcn_conv import GCNConv
from .host import _mm
from .linear import DenseLinear


def host_gcn(conv, x, edge_index, edge_weight):
    """PyG ``GCNConv(x, edge_index, edge_weight)`` on the host: add_remaining_self_loops (a node's own loop keeps its
    weight, else 1), destination degrees, ``out[col] += dis[row] w dis[col] h[row]``."""
    n = x.size(0)
    h = F.linear(x, conv.lin.weight)
    row, col = edge_index[0], edge_index[1]
    keep = row != col
    loop_w = torch.ones(n, dtype=x.dtype, device=x.device)
    loop_w[row[~keep]] = edge_weight[~keep].to(x.dtype)
    loop = torch.arange(n, device=x.device)
    row, col = torch.cat([row[keep], loop]), torch.cat([col[keep], loop])
    w = torch.cat([edge_weight[keep].to(x.dtype), loop_w])
    deg = torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(0, col, w)
    dis = deg.pow(-0.5)
    dis = dis.masked_fill(dis == float("inf"), 0)
    norm = dis[row] * w * dis[col]
    out = torch.zeros(n, h.size(1), dtype=x.dtype, device=x.device).index_add_(0, col, norm[:, None] * h[row])
    return out + conv.bias


def dense_gcn(conv, x, A):
    """``GCNConv(x, *adj2coo(A))``: ``Ahat^T (x W^T) + b`` with ``Ahat = D^-1/2 A D^-1/2``, ``D`` the column sums of
    ``A`` (diagonal included), ``deg^-1/2 = 0`` where the degree is 0.  Differentiable in ``A``."""
    deg = A.sum(0)
    pos = deg > 0
    dis = torch.where(pos, deg.clamp_min(torch.finfo(A.dtype).tiny).pow(-0.5), torch.zeros_like(deg))
    ahat = dis[:, None] * A * dis[None, :]
    return mat_tn(ahat, conv.lin(x)) + conv.bias


def edge_spmm(edge_index, n, S, graph=None):
    """torch_sparse ``spmm(edge_index, ones, n, n, S)``: ``out[row] += S[col]`` (duplicates counted).  ``graph``: the
    flipped edge list as an unnormalised CSRGraph (device)."""
    if S.is_cuda:
        from ..ops import propagate
        return propagate(S, graph, 1)
    row, col = edge_index[0], edge_index[1]
    return torch.zeros(n, S.size(1), dtype=S.dtype, device=S.device).index_add_(0, row, S[col])


class GCNPooling(nn.Module):
    def __init__(self, in_dim, hid_dim, device, sparse):
        super().__init__()
        self.gcn = GCNConv(in_dim, hid_dim)
        self.softmax = nn.Softmax(dim=1)
        self.device = device
        self.sparse = sparse

    def to_onehot(self, label_matrix, num_classes):
        return _onehot(label_matrix, num_classes, self.gcn.bias.dtype)

    def assign(self, pre):
        """``(S, entropy(S))`` from the GCN's output ``pre``."""
        S, ce = jhgda_pool_rows(pre)
        if self.sparse:
            S = self.to_onehot(torch.argmax(S, dim=1), S.shape[1])
            ce = _entropy(S)
        return S, ce

    def forward(self, X_old, edge_index, edge_weight, A_old, Y_old, Z, use_sparse=False):
        """The reference's ``(S, X_new, A_new, Y_new, Y_new_prob)`` for an edge list (``use_sparse``) or a dense
        ``A_old`` (``edge_index`` / ``edge_weight`` unused then: the dense form of ``adj2coo``'s complete graph)."""
        if use_sparse:
            pre = self.gcn(X_old, edge_index) if X_old.is_cuda else host_gcn(self.gcn, X_old, edge_index, edge_weight)
        else:
            pre = dense_gcn(self.gcn, X_old, A_old)
        S, _ = self.assign(pre)
        return (S,) + pool_outputs(S, Z, Y_old, edge_index if use_sparse else A_old, use_sparse, X_old.size(0))


def pool_outputs(S, Z, Y_old, A, use_sparse, n, graph=None, last=False):
    """``(X_new, A_new, Y_new, Y_new_prob)`` of GCNPooling.forward; ``last`` leaves X_new and A_new out (None)."""
    Yp = torch.softmax(mat_tn(S, Y_old), dim=1)
    Y_new = _onehot(torch.argmax(Yp, dim=1), Y_old.shape[1], S.dtype)
    if last:
        return None, None, Y_new, Yp
    X_new = mat_tn(S, Z)
    A_new = mat_tn(edge_spmm(A, n, S, graph), S) if use_sparse else mat_tn(S, _mm(A, S))
    return X_new, A_new, Y_new, Yp


def _onehot(idx, num_classes, dtype):
    return torch.eye(num_classes, dtype=dtype, device=idx.device).index_select(0, idx)


def _entropy(x):
    return torch.mean(torch.sum(-x * torch.log(x + 1e-7), dim=1))


def check_pseudo(pseudo, classwise, hid_dim, num_classes, device):
    """ValueError, before any device work, for a ``pseudo`` setting that cannot run."""
    if pseudo not in ('classifier', 'gmm'):
        raise ValueError(f"JHGDA: pseudo must be 'classifier' or 'gmm', got {pseudo!r}")
    if pseudo == 'gmm':
        from ..ops import GMM_MAX_COMPONENTS, GMM_MAX_DIM
        if not classwise:
            raise ValueError("JHGDA: pseudo='gmm' needs classwise=True (with classwise=False the pseudo-labels are unused)")
        if torch.device(device).type == "cuda" and hid_dim > GMM_MAX_DIM:
            raise ValueError(f"JHGDA: pseudo='gmm' takes hid_dim up to {GMM_MAX_DIM} on the GPU, got hid_dim={hid_dim}")
        if torch.device(device).type == "cuda" and num_classes > GMM_MAX_COMPONENTS:
            raise ValueError(f"JHGDA: pseudo='gmm' takes num_classes up to {GMM_MAX_COMPONENTS} on the GPU, got "
                             f"num_classes={num_classes}")


class JHGDABase(nn.Module):
    def __init__(self, in_dim, hid_dim, num_classes, device, pool_ratio, num_s, num_t, num_layers=3, dropout=0.1,
                 act=F.relu, share=False, classwise=False, sparse=False, pseudo='classifier', gmm_max_iter=100,
                 gmm_tol=1e-3, gmm_reg_covar=1e-6, gmm_smooth_r=None, **kwargs):
        super().__init__()
        check_pseudo(pseudo, classwise, hid_dim, num_classes, device)
        self.pseudo, self.gmm_smooth_r = pseudo, gmm_smooth_r
        self.gmm_args = dict(max_iter=int(gmm_max_iter), tol=float(gmm_tol), reg_covar=float(gmm_reg_covar))
        self.gmm_device = None                # the DeviceGMMLabels of a device fit, built on its first epoch
        self.gmm_last = None                  # the host path's (n_iter, converged, fell_back, lower_bound) of the epoch
        self.num_layers, self.share, self.pool_ratio = num_layers, share, pool_ratio
        self.classwise, self.sparse, self.device, self.act = classwise, sparse, device, act
        self.num_s, self.num_t = num_s, num_t
        self.gnn_emb = nn.ModuleList()
        self.gnn_emb.append(GCNConv(in_dim, hid_dim))
        for _ in range(1, num_layers):
            self.gnn_emb.append(GCNConv(hid_dim, hid_dim))
        if share:
            self.gnn_pool = self._pools(in_dim, hid_dim, num_s)
        else:
            self.gnn_pool_src = self._pools(in_dim, hid_dim, num_s)
            self.gnn_pool_tgt = self._pools(in_dim, hid_dim, num_t)
        self.cls_model = nn.Sequential(DenseLinear(hid_dim, num_classes))
        self.loss_func = nn.CrossEntropyLoss()

    def _pools(self, in_dim, hid_dim, n):
        pools = nn.ModuleList()
        width = int(n * self.pool_ratio)
        pools.append(GCNPooling(in_dim, width, device=self.device, sparse=self.sparse))
        for _ in range(1, self.num_layers):
            pools.append(GCNPooling(hid_dim, int(width * self.pool_ratio), device=self.device, sparse=self.sparse))
            width = int(width * self.pool_ratio)
        return pools

    def pools(self, domain):
        return self.gnn_pool if self.share else (self.gnn_pool_src if domain == 0 else self.gnn_pool_tgt)

    @staticmethod
    def level_widths(num_nodes, pool_ratio, num_layers):
        """K_i of the pooling levels for a domain of ``num_nodes`` nodes (as the constructor sizes them)."""
        out, w = [], int(num_nodes * pool_ratio)
        out.append(w)
        for _ in range(1, num_layers):
            w = int(w * pool_ratio)
            out.append(w)
        return out

    # -- forward -------------------------------------------------------------------------------------------------------
    def forward(self, x_s, edge_index_s, y_s, x_t, edge_index_t, y_t, graphs=None):
        """``(embeddings, pred, pooling_loss, y)`` as the reference returns them.  ``graphs``: per domain a dict of the
        device structures (``edges`` the proximity CSR, ``spmm`` the flipped edge graph), built by the trainer."""
        doms = [dict(x=x_s, ei=edge_index_s, A=edge_index_s, yp=y_s, n=x_s.size(0)),
                dict(x=x_t, ei=edge_index_t, A=edge_index_t, yp=y_t, n=x_t.size(0))]
        graphs = graphs or [{}, {}]
        self.embedddings, self.pooling_loss, self.y = [], [], []
        for i in range(self.num_layers):
            if i == 0 and x_s.is_cuda:                         # both level-0 GCNs of a domain: one stacked product
                pre0 = [self._level0(k, d) for k, d in enumerate(doms)]
                zs = [self.act(h) for h, _ in pre0]
            else:
                zs = [self._emb(i, d) for d in doms]
            self.embedddings.append(zs)
            if self.classwise and i == 0:
                y_t_pseudo = self.pseudo_label(zs[0], y_s, zs[1], y_t, edge_index_t, None,
                                               smooth_graph=graphs[1].get("smooth"))
                doms[1]["yp"] = y_t_pseudo
                self.y.append([y_s, y_t_pseudo])
            last = i == self.num_layers - 1
            outs, terms = [], {"ce": [], "prox": [], "cce": [], "lm": [], "ls": []}
            for k, (d, z) in enumerate(zip(doms, zs)):
                pool = self.pools(k)[i]
                pre = (pre0[k][1] if d["x"].is_cuda else
                       host_gcn(pool.gcn, d["x"], d["ei"], _ones(d["ei"], d["x"]))) if i == 0 else \
                    dense_gcn(pool.gcn, d["x"], d["A"])
                S, ce = pool.assign(pre)
                X_new, A_new, Y_new, Yp = pool_outputs(S, z, d["yp"], d["A"], i == 0, d["n"],
                                                       graphs[k].get("spmm"), last)
                terms["ce"].append(ce)
                terms["prox"].append(jhgda_prox(d["A"], S, graphs[k].get("edges") if i == 0 else None))
                terms["cce"].append(_entropy(Yp))
                terms["lm"].append(self.label_matching(S, d["yp"], Yp, one_hot=i == 0))
                terms["ls"].append(self.label_stable(S, d["yp"], Yp))
                outs.append((X_new, A_new, Y_new, Yp))
            self.y.append([outs[0][2], outs[1][2]])
            self.pooling_loss.append({k: (v[0] + v[1]) / 2 for k, v in terms.items()})
            for d, (X_new, A_new, _, Yp) in zip(doms, outs):
                d.update(x=X_new, A=A_new, yp=Yp, n=None if X_new is None else X_new.size(0), ei=None)
        pred = [self.cls_model(self.embedddings[0][0]), self.cls_model(self.embedddings[0][1])]
        return self.embedddings, pred, self.pooling_loss, self.y

    def _level0(self, k, d):
        """``(gnn_emb[0](x), pool[0].gcn(x))`` on the device: ``x [W_emb; W_pool]^T`` as ONE product (ops.linear_nt: its
        weight gradient takes the GEMM form without split-K slabs), then one aggregation per half with its bias."""
        from ..ops import linear_nt, propagate
        emb, pool = self.gnn_emb[0], self.pools(k)[0].gcn
        hid = emb.out_channels
        H = linear_nt(d["x"], torch.cat([emb.lin.weight, pool.lin.weight], 0))
        g = emb._graph(d["x"], d["ei"], None)
        return (propagate(H[:, :hid].contiguous(), g, 1, emb.bias),
                propagate(H[:, hid:].contiguous(), g, 1, pool.bias))

    def _emb(self, i, d):
        conv = self.gnn_emb[i]
        if i == 0:
            h = conv(d["x"], d["ei"]) if d["x"].is_cuda else host_gcn(conv, d["x"], d["ei"], _ones(d["ei"], d["x"]))
        else:
            h = dense_gcn(conv, d["x"], d["A"])
        return self.act(h)

    def pseudo_label(self, z_s, y_s, z_t, y_t, edge_index_t, edge_weight_t, smooth_graph=None):
        """``onehot(argmax cls_model(z_t))``, no gradient (the reference's GMMClustering object is built and unused).
        With ``pseudo='gmm'`` those labels only start a Gaussian mixture on ``z_t`` (one run, no RNG), whose clusters
        are assigned to the source's class centres as ``GMMClustering.forward`` does; where the fit is ill-defined the
        classifier's labels stay (``fell_back``).  ``y_s`` is one-hot: the source's true labels."""
        with torch.no_grad():
            idx = torch.argmax(torch.log_softmax(self.cls_model(z_t), dim=-1), dim=1)
            if self.pseudo == 'gmm':
                return self._gmm_pseudo(z_s, y_s, z_t, idx, edge_index_t, smooth_graph)
        return self.to_onehot(idx, y_s.shape[1])

    def _gmm_pseudo(self, z_s, y_s, z_t, idx, edge_index_t, smooth_graph):
        from .gmm_clustering import DeviceGMMLabels, GMMClustering, get_emb_centers
        C = y_s.shape[1]
        if z_t.is_cuda:
            if self.gmm_device is None:
                self.gmm_device = DeviceGMMLabels(C, smooth_graph=smooth_graph, **self.gmm_args)
            hot, _ = self.gmm_device(z_s, torch.argmax(y_s, dim=1), z_t, idx)
            return hot.to(self.cls_model[0].weight.dtype)
        g = GMMClustering(C, z_t.device, n_init=1, **self.gmm_args)
        smooth = self.gmm_smooth_r is not None
        try:                                   # an ill-defined covariance and a non-finite cost both raise ValueError
            out = g.forward(get_emb_centers(z_s.detach(), y_s, C), z_t, None, edge_index_t, None, smooth,
                            self.gmm_smooth_r, resp0=self.to_onehot(idx, C).to(z_t.dtype))
            labels = out["label"]
            self.gmm_last = (g.gmm.n_iter_, int(g.gmm.converged_), 0, g.gmm.lower_bound_)
        except ValueError:
            labels = idx
            self.gmm_last = (0, 0, 1, float("-inf"))
        return self.to_onehot(labels.long(), C)

    def entropy(self, x, reduction='mean'):
        return _entropy(x)

    def proximity_loss(self, A, S, adj_hop=1):
        if adj_hop != 1:
            raise NotImplementedError("JHGDABase.proximity_loss: adj_hop = 1 only (the reference's value)")
        return jhgda_prox(A, S)

    def label_matching(self, S, Y_old, Y_new, one_hot=False):
        """``1 - #{i : argmax_k (Y_old Y_new^T)_ik == argmax_k S_ik} / N`` (argmax only: no gradient).
        ``one_hot`` (level 0, where ``Y_old`` holds labels or pseudo-labels): row i of ``Y_old Y_new^T`` is exactly the
        column ``Y_new[:, c_i]``, so its first argmax is that column's -- a count in O(N C + K C) with no N x K matrix.
        Above level 0 ``Y_old`` holds probabilities and the small N_i x K_i product is formed on the device GEMM."""
        with torch.no_grad():
            if S.is_cuda and one_hot:
                pick = torch.argmax(Y_new, dim=0)[torch.argmax(Y_old, dim=1)]
            elif S.is_cuda:
                from ..ops import GEMM_NT, gemm
                pick = torch.argmax(gemm(GEMM_NT, Y_old.detach(), Y_new.detach()), dim=1)
            else:
                pick = torch.argmax(Y_old @ Y_new.T, dim=1)
            c = (pick == torch.argmax(S, dim=1)).sum().to(S.dtype)
        return 1 - c / S.shape[0]

    def label_stable(self, S, Y_old, Y_new):
        mat = torch.softmax(_mm(mat_tn(Y_old, S), Y_new), dim=1)
        return 1 - torch.mean(torch.diag(mat))

    def adj2coo(self, A):
        n = A.shape[0]
        idx = torch.arange(n, device=A.device)
        edge_index = torch.stack([idx.repeat_interleave(n), idx.repeat(n)])
        return edge_index, A.reshape(-1)

    def classwise_simple_mmd(self, source, target, src_y, tgt_y):
        """sum over classes of ``||mean_s(c) - mean_t(c)||``, a class left out where it is empty in either domain (the
        reference's NaN test) -- decided on the device, without a host read."""
        if not source.is_cuda:
            mmd = 0.
            for c in range(src_y.shape[1]):
                v = self.simple_mmd(source[src_y[:, c].to(torch.bool)], target[tgt_y[:, c].to(torch.bool)])
                if not torch.isnan(v):
                    mmd += v
            return mmd
        cs, ct = src_y.sum(0), tgt_y.sum(0)
        ms = mat_tn(src_y.contiguous(), source) / cs.clamp_min(1)[:, None]
        mt = mat_tn(tgt_y.contiguous(), target) / ct.clamp_min(1)[:, None]
        d = torch.norm(ms - mt, dim=1)
        return torch.where((cs > 0) & (ct > 0), d, torch.zeros_like(d)).sum()

    def simple_mmd(self, source, target):
        return torch.norm(torch.mean(source, dim=0) - torch.mean(target, dim=0))

    def simple_mmd_kernel(self, source, target):
        return torch.exp(-0.1 * torch.norm(torch.mean(source, dim=0) - torch.mean(target, dim=0)))

    def inference(self, data):
        """``cls_model(gnn_emb[0](x))`` -- no activation, as the reference writes it."""
        x = data.x
        z = self.gnn_emb[0](x, data.edge_index) if x.is_cuda else \
            host_gcn(self.gnn_emb[0], x, data.edge_index, _ones(data.edge_index, x))
        return self.cls_model(z)

    def to_onehot(self, label_matrix, num_classes):
        return _onehot(label_matrix, num_classes, self.cls_model[0].weight.dtype)


def _ones(edge_index, x):
    return torch.ones(edge_index.shape[1], dtype=x.dtype, device=x.device)
