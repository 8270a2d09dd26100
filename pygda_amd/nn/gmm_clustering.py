"""``GMMClustering`` / ``Clustering`` and their helpers (pygda/nn/gmm_clustering.py): the pseudo-labelling step of JHGDA.

Names, signatures and return values are the reference's; the bodies are ours.  The reference fits
``sklearn.mixture.GaussianMixture(n_components, n_init=5)`` on the host; here the same EM loop (full covariances, sklearn's
M-step, precision Cholesky factors, log-sum-exp E-step, ``|change of the lower bound| < tol``) runs on the device for all
restarts at once (csrc/gda_gmm.hip), with no host read inside the loop: every run carries its own state, and a run that
has converged is left untouched by the kernels, so iterations are enqueued ``check_every`` at a time.  Tensors on the
CPU take the same loop restated in torch, in the input's dtype.

The reference's mixture is unseeded (``random_state=None``), so there is no stream to reproduce: the initial
responsibilities are this project's own draw -- k-means++ seeding from a ``torch.Generator`` and a fixed number of Lloyd
sweeps on the k-means step kernel.  ``fit_em`` starts from given responsibilities instead.

``SparseTensor`` inputs of ``gcn_norm`` are out of scope.
"""
import math

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment
from torch.nn import functional as F

from .prop_gcn_conv import gcn_norm as _gcn_norm_edges

INIT_SWEEPS = 10            # Lloyd sweeps of the initial k-means
SMOOTH_STEPS = 20           # reference :331

_ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for "
                "instance caused by singleton or collapsed samples). Try to decrease the number of components, increase "
                "reg_covar, or scale the input data.")
_ILL_DEFINED_F32 = " The numerical accuracy can also be improved by passing float64 data instead of float32."


class DIST(object):
    """``get_dist(A, B, cross=False)`` for ``'cos'`` (``0.5 (1 - cos)``) and ``'euc'`` (reference :16-100).  Both normalise
    their operands first, and ``euc`` without ``cross`` returns ONE Frobenius norm, not a vector -- as the reference does."""

    def __init__(self, dist_type):
        self.dist_type = dist_type

    def get_dist(self, pointA, pointB, cross=False):
        return getattr(self, self.dist_type)(pointA, pointB, cross)

    def cos(self, pointA, pointB, cross):
        pointA = F.normalize(pointA, dim=1)
        pointB = F.normalize(pointB, dim=1)
        if not cross:
            return 0.5 * (1.0 - torch.sum(pointA * pointB, dim=1))
        assert pointA.size(1) == pointB.size(1)
        return 0.5 * (1.0 - torch.matmul(pointA, pointB.transpose(0, 1)))

    def euc(self, pointA, pointB, cross):
        pointA = F.normalize(pointA, dim=1)
        pointB = F.normalize(pointB, dim=1)
        if not cross:
            return torch.norm(pointA - pointB)
        return torch.cdist(pointA, pointB, p=2)


def onehot(label_matrix, num_classes):
    """Rows of the identity picked by ``label_matrix`` (reference :103-123)."""
    identity = torch.eye(num_classes).to(label_matrix.device)
    return torch.index_select(identity, 0, label_matrix)


def get_emb_centers(embeddings, label_array, n_label):
    """``label_array^T @ embeddings``: the per-label SUMS of the embeddings.  The reference (:148-150) computes the
    reciprocal counts and does not use them, so its "centers" are sums; that is kept."""
    if len(label_array.shape) == 1:
        label_array = onehot(label_array, n_label).to(embeddings.device)
    return torch.matmul(label_array.T.to(embeddings.dtype), embeddings)


def gcn_norm(edge_index, edge_weight=None, num_nodes=None, improved=False, add_self_loops=True, dtype=None):
    """The ``edge_index`` branch of the reference's ``gcn_norm`` (:211-229), which is the arithmetic of
    :func:`pygda_amd.nn.prop_gcn_conv.gcn_norm` (remaining self loops, degree by destination, both sides).  A
    ``SparseTensor`` is not accepted."""
    if not isinstance(edge_index, torch.Tensor):
        raise NotImplementedError("gcn_norm takes an edge_index tensor; SparseTensor inputs are out of scope")
    return _gcn_norm_edges(edge_index, edge_weight, num_nodes, improved, add_self_loops, dtype)


def _on_device(t):
    return t.is_cuda


def _assign(x, centers, metric, want_dist=True):
    """``(labels, dist, sums, counts)`` of one k-means assignment: the kernel on the device, torch on the CPU."""
    from .. import ops
    if _on_device(x):
        return ops.kmeans_step(x, centers.to(torch.float32), metric, want_dist)
    if metric == ops.KMEANS_SQEUC:
        dist = ((x[:, None, :] - centers[None, :, :]) ** 2).sum(2)
    else:
        dist = DIST("cos" if metric == ops.KMEANS_COS else "euc").get_dist(x, centers, cross=True)
    labels = torch.min(dist, dim=1)[1]
    hot = F.one_hot(labels, centers.size(0)).to(x.dtype)
    return labels, dist, hot.T @ x, hot.sum(0)


class FittedMixture(object):
    """The kept run of a fit, under the names of ``sklearn.mixture.GaussianMixture``: tensors on the device of the data."""

    def __init__(self, weights, means, covariances, precisions_cholesky, log_det, lower_bound, n_iter, converged):
        self.weights_, self.means_, self.covariances_ = weights, means, covariances
        self.precisions_cholesky_, self.log_det_ = precisions_cholesky, log_det
        self.lower_bound_, self.n_iter_, self.converged_ = float(lower_bound), int(n_iter), bool(converged)

    def predict_proba(self, x):
        """One more E-step with the kept parameters: ``[N, K]`` responsibilities."""
        if _on_device(x):
            from .. import ops
            return ops.gmm_estep(x.detach().to(torch.float32), self.weights_[None], self.means_[None],
                                 self.precisions_cholesky_[None], self.log_det_[None])[0]
        lp = _cpu_log_prob(x, self.weights_, self.means_, self.precisions_cholesky_, self.log_det_)
        return torch.exp(lp - torch.logsumexp(lp, dim=1, keepdim=True))

    def predict(self, x):
        return self.predict_proba(x).argmax(dim=1)


def _cpu_mstep(x, resp, reg_covar):
    nk = resp.sum(0) + 10 * torch.finfo(resp.dtype).eps
    means = (resp.T @ x) / nk[:, None]
    cov = torch.empty(means.size(0), x.size(1), x.size(1), dtype=x.dtype)
    eye = torch.eye(x.size(1), dtype=x.dtype)
    for k in range(means.size(0)):
        diff = x - means[k]                                        # centred, as sklearn's full covariance
        cov[k] = ((resp[:, k] * diff.T) @ diff) / nk[k] + reg_covar * eye
    return nk / nk.sum(), means, cov


def _cpu_factor(cov):
    L, info = torch.linalg.cholesky_ex(cov)
    if bool((info != 0).any()) or not bool(torch.isfinite(L).all()):
        raise ValueError(_ILL_DEFINED + (_ILL_DEFINED_F32 if cov.dtype == torch.float32 else ""))
    eye = torch.eye(cov.size(-1), dtype=cov.dtype).expand_as(cov)
    prec = torch.linalg.solve_triangular(L, eye, upper=False).mT.contiguous()
    return prec, torch.log(torch.diagonal(prec, dim1=-2, dim2=-1)).sum(-1)


def _cpu_log_prob(x, weights, means, prec, log_det):
    d = x.size(1)
    sq = torch.stack([(((x - means[k]) @ prec[k]) ** 2).sum(1) for k in range(means.size(0))], dim=1)
    return -0.5 * (d * math.log(2 * math.pi) + sq) + log_det + torch.log(weights)


class GMMClustering(object):
    """Full-covariance Gaussian mixture over the target embeddings, aligned to the source class centres with a linear
    assignment and optionally smoothed over the target graph (reference :232-358).

    Private keywords: ``n_init``, ``max_iter``, ``tol``, ``reg_covar`` are sklearn's defaults; ``seed`` (None: torch's
    default generator) seeds the ``torch.Generator`` of the initial k-means; ``check_every`` is the number of EM
    iterations enqueued between two reads of the run flags -- the result does not depend on it."""

    def __init__(self, num_class, device, dist_type='cos', n_init=5, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=None,
                 check_every=8):
        self.Dist = DIST(dist_type)
        self.num_class = num_class
        self.device = device
        self.n_init, self.max_iter, self.tol, self.reg_covar = int(n_init), int(max_iter), float(tol), float(reg_covar)
        self.seed, self.check_every = seed, max(1, int(check_every))

    # ------------------------------------------------------------------------------------------------ the mixture --
    def _generator(self):
        return None if self.seed is None else torch.Generator().manual_seed(int(self.seed))

    def init_resp(self, x):
        """``[n_init, N, K]`` one-hot responsibilities: per run a Euclidean k-means (k-means++ seeding, ``INIT_SWEEPS``
        Lloyd sweeps).  The draws are this project's own."""
        from .. import ops
        gen, n, K = self._generator(), x.size(0), self.num_class
        runs = []
        for _ in range(self.n_init):
            first = int(torch.randint(n, (1,), generator=gen))
            centers = x[first:first + 1].clone()
            for _k in range(1, K):
                d2 = _assign(x, centers, ops.KMEANS_SQEUC)[1].min(dim=1)[0].double().cpu().clamp_(min=0)
                if float(d2.sum()) <= 0:                             # fewer distinct rows than components
                    d2 = torch.ones(n, dtype=torch.float64)
                pick = int(torch.multinomial(d2, 1, generator=gen))
                centers = torch.cat([centers, x[pick:pick + 1]])
            for _s in range(INIT_SWEEPS):
                _, _, sums, counts = _assign(x, centers, ops.KMEANS_SQEUC, want_dist=False)
                centers = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], centers)
            labels = _assign(x, centers, ops.KMEANS_SQEUC, want_dist=False)[0]
            runs.append(F.one_hot(labels, K).to(x.dtype))
        return torch.stack(runs)

    def fit_em(self, x, resp0):
        """EM from the responsibilities ``resp0 [R, N, K]`` (or ``[N, K]``), one run per leading entry; keeps the run
        with the largest lower bound in ``self.gmm`` and returns it."""
        x = x.detach()
        resp0 = resp0.detach()
        if resp0.dim() == 2:
            resp0 = resp0[None]
        if resp0.dim() != 3 or resp0.size(1) != x.size(0):
            raise ValueError(f"resp0 must be [R, N={x.size(0)}, K], got {tuple(resp0.shape)}")
        self.gmm = self._fit_device(x, resp0) if _on_device(x) else self._fit_cpu(x, resp0)
        return self.gmm

    def _fit_device(self, x, resp0):
        from .. import ops
        x = x.to(torch.float32)
        R, _, K = resp0.shape
        ops.gmm_check_limits(x.size(1), K, R)
        state = ops.gmm_state(R, x.device)
        bounds, flags = ops.gmm_state_fields(state)
        resp = resp0.to(torch.float32).clone()
        par = ops.gmm_mstep(x, resp, self.reg_covar, state)
        fac = ops.gmm_factor(par[2], state)
        done = 0
        while done < self.max_iter:
            m = min(self.check_every, self.max_iter - done)
            for _ in range(m):                                       # blind: a finished run is left untouched
                ops.gmm_estep(x, par[0], par[1], fac[0], fac[1], self.tol, state, out=resp)
                ops.gmm_mstep(x, resp, self.reg_covar, state, out=par)
                ops.gmm_factor(par[2], state, out=fac)
            done += m
            f = flags.cpu()                                          # the one host read per `check_every` iterations
            if bool(((f[:, 1] >= 1) | (f[:, 2] != 0)).all()):
                break
        f, lower = flags.cpu().numpy(), bounds[:, 0].cpu().numpy()
        if (f[:, 2] != 0).any():
            raise ValueError(_ILL_DEFINED + _ILL_DEFINED_F32)
        best = int(np.argmax(lower))                                 # the first of equal maxima, as sklearn's loop
        return FittedMixture(par[0][best].clone(), par[1][best].clone(), par[2][best].clone(), fac[0][best].clone(),
                             fac[1][best].clone(), lower[best], f[best, 0], f[best, 1] >= 1)

    def _fit_cpu(self, x, resp0):
        best = None
        for r in range(resp0.size(0)):
            w, mu, cov = _cpu_mstep(x, resp0[r].to(x.dtype), self.reg_covar)
            prec, logdet = _cpu_factor(cov)
            lower, n_iter, converged = float("-inf"), 0, False
            for n_iter in range(1, self.max_iter + 1):
                prev = lower
                lp = _cpu_log_prob(x, w, mu, prec, logdet)
                lse = torch.logsumexp(lp, dim=1)
                w, mu, cov = _cpu_mstep(x, torch.exp(lp - lse[:, None]), self.reg_covar)
                prec, logdet = _cpu_factor(cov)
                lower = float(lse.mean())
                if abs(lower - prev) < self.tol:
                    converged = True
                    break
            if best is None or lower > best.lower_bound_:
                best = FittedMixture(w, mu, cov, prec, logdet, lower, n_iter, converged)
        return best

    # ---------------------------------------------------------------------------------------------------- forward --
    def forward(self, src_centers, emb_t, y_t, target_edge_index, target_edge_attr, smooth, smooth_r, resp0=None):
        """Reference :282-307.  ``resp0`` (not in the reference): start the runs from these responsibilities instead of
        the seeded k-means."""
        n_label = src_centers.shape[0]
        self.gt = y_t
        x = emb_t.detach()
        model = self.fit_em(x, self.init_resp(x) if resp0 is None else resp0)
        prob = model.predict_proba(x)
        self.target_pred = prob.argmax(dim=1).to(torch.int32).to(self.device)
        self.target_pred_prob = prob.to(torch.float32).to(self.device)
        tgt_centers = get_emb_centers(emb_t.detach(), self.target_pred.to(emb_t.device), n_label)
        cluster2label = self.align_centers(src_centers, tgt_centers)
        shuffle_idx = [v[1] for v in sorted({idx: i for i, idx in enumerate(cluster2label)}.items())]
        self.num_nodes = emb_t.size(0)
        self.labels = torch.as_tensor(np.asarray(cluster2label), dtype=torch.int64).to(self.device)[self.target_pred.long()]
        self.target_pred_prob = self.target_pred_prob[:, shuffle_idx]             # re-arrange
        if smooth:
            self.smooth_labels, p = self.smooth(target_edge_index, target_edge_attr, smooth_r)
            self.samples = {"data": list(range(emb_t.size(0))), "label": self.smooth_labels, "dist2center": p,
                            "gt": self.gt}
        else:
            self.samples = {"data": list(range(emb_t.size(0))), "label": self.labels,
                            "dist2center": self.target_pred_prob, "gt": self.gt}
        return self.samples

    def smooth(self, edge_index, v, smooth_r):
        """20 steps ``p <- r p + (1 - r) A_hat p`` (reference :327-336), ``A_hat`` from the ``SparseTensor`` branch of the
        reference's ``gcn_norm``: the diagonal SET to 1, the degree the row sums, both sides normalised.  On the device
        the step matrix ``(1 - r) A_hat + r I`` is one CSR and the 20 steps one K-step aggregation call."""
        p = self.target_pred_prob
        n, dev = self.num_nodes, p.device
        edge_index = edge_index.to(dev)
        v = torch.ones(edge_index.size(1), device=dev) if v is None else v.to(dev)
        row, col = edge_index[0], edge_index[1]
        keep = row != col                                            # fill_diag replaces what the diagonal held
        loops = torch.arange(n, device=dev, dtype=row.dtype)
        row, col = torch.cat([row[keep], loops]), torch.cat([col[keep], loops])
        v = torch.cat([v[keep].to(p.dtype), torch.ones(n, dtype=p.dtype, device=dev)])
        # the degree is added in float64 and rounded once: the order of the additions does not reach the float32 result
        deg = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, row, v.double()).to(p.dtype)
        dis = deg.pow(-0.5)
        dis.masked_fill_(dis == float('inf'), 0.)
        val = dis[row] * v * dis[col]
        if not _on_device(p):
            for _ in range(SMOOTH_STEPS):
                p = smooth_r * p + (1 - smooth_r) * torch.zeros_like(p).index_add_(0, row, val[:, None] * p[col])
            return torch.argmax(p, dim=1), p
        from ..graph import CSRGraph
        from ..ops import propagate
        val = (1 - smooth_r) * val
        val[-n:] += smooth_r
        nnz = int(row.numel())

        def csr(a, b):
            order = torch.argsort(a, stable=True)
            ptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
            ptr[1:] = torch.cumsum(torch.bincount(a, minlength=n), 0).to(torch.int32)
            return ptr, b[order].to(torch.int32).contiguous(), val[order].contiguous()

        g = CSRGraph(n, nnz, *csr(row, col), *csr(col, row))
        g._nnz = nnz
        p = propagate(p.contiguous(), g, SMOOTH_STEPS)
        return torch.argmax(p, dim=1), p

    def align_centers(self, src_center, tgt_center):
        """Linear assignment of the target clusters to the source centres, on the host (reference :354-358)."""
        cost = self.Dist.get_dist(tgt_center, src_center, cross=True)
        cost = cost.data.cpu().numpy()
        _, col_ind = linear_sum_assignment(cost)
        return col_ind


def smoothing_graph(edge_index, num_nodes, smooth_r, device):
    """The CSR of one smoothing step, ``(1 - r) A_hat + r I`` with ``A_hat`` as :meth:`GMMClustering.smooth` builds it
    (unit edge weights), for ``ops.propagate``: built once, so that the steps inside an epoch need no sort."""
    from ..graph import CSRGraph
    n, dev = num_nodes, device
    edge_index = edge_index.to(dev)
    row, col = edge_index[0], edge_index[1]
    keep = row != col
    loops = torch.arange(n, device=dev, dtype=row.dtype)
    row, col = torch.cat([row[keep], loops]), torch.cat([col[keep], loops])
    v = torch.ones(row.numel(), dtype=torch.float32, device=dev)
    deg = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, row, v.double()).to(torch.float32)
    dis = deg.pow(-0.5)
    dis.masked_fill_(dis == float('inf'), 0.)
    val = (1 - smooth_r) * (dis[row] * v * dis[col])
    val[-n:] += smooth_r
    nnz = int(row.numel())

    def csr(a, b):
        order = torch.argsort(a, stable=True)
        ptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        ptr[1:] = torch.cumsum(torch.bincount(a, minlength=n), 0).to(torch.int32)
        return ptr, b[order].to(torch.int32).contiguous(), val[order].contiguous()

    g = CSRGraph(n, nnz, *csr(row, col), *csr(col, row))
    g._nnz = nnz
    return g


class DeviceGMMLabels(object):
    """The steps of :meth:`GMMClustering.forward` for ONE run started from given labels, entirely on the device and
    with no host read, so that an epoch which calls it can be captured: the state reset (a copy from a template), M-step
    and factor from the one-hot start, ``max_iter`` blind EM iterations (the freeze rule leaves a finished run
    untouched), the ``predict_proba`` E-step, the per-label sums of both domains, the assignment solver and the relabel
    kernel; with ``smooth_graph`` the 20 smoothing steps and the argmax of their result.  Where the fit is ill-defined
    (``failed``: a covariance without a Cholesky factor or a non-finite assignment cost) the labels are the start's.
    Every buffer is allocated once, on the first call; ``state`` is what the trainer's log reads."""

    def __init__(self, num_class, max_iter=100, tol=1e-3, reg_covar=1e-6, smooth_graph=None):
        self.K, self.max_iter, self.tol, self.reg_covar = int(num_class), int(max_iter), float(tol), float(reg_covar)
        self.smooth_graph = smooth_graph
        self._shape = None

    def _allocate(self, n, d, dev):
        from .. import ops
        K = self.K
        ops.gmm_check_limits(d, K, 1)
        f32 = dict(dtype=torch.float32, device=dev)
        self._template = ops.gmm_state(1, dev)
        self.state = ops.gmm_state(1, dev)
        self.resp = torch.empty(1, n, K, **f32)
        self.par = (torch.empty(1, K, **f32), torch.empty(1, K, d, **f32), torch.empty(1, K, d, d, **f32))
        self.fac = (torch.empty(1, K, d, d, **f32), torch.empty(1, K, dtype=torch.float64, device=dev))
        self.src = (torch.empty(K, d, **f32), torch.empty(K, **f32))
        self.tgt = (torch.empty(K, d, **f32), torch.empty(K, **f32))
        self.perm = (torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev))
        self.pred = torch.empty(n, dtype=torch.int64, device=dev)
        self.out = (torch.empty(n, K, **f32), torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, K, **f32))
        self._shape = (n, d, dev)

    def __call__(self, z_s, y_s, z_t, start):
        """``(onehot [N, K] fp32, labels [N] int64)`` for the target embeddings ``z_t`` from the labels ``start [N]``
        (int64); ``y_s [Ns]`` int64 are the source's true labels."""
        from .. import ops
        x, zs = z_t.detach().to(torch.float32), z_s.detach().to(torch.float32)
        n, d = x.shape
        if self._shape != (n, d, x.device):
            self._allocate(n, d, x.device)
        st, resp, par, fac = self.state, self.resp, self.par, self.fac
        st.copy_(self._template)
        resp.zero_()
        resp[0].scatter_(1, start[:, None], 1.0)                     # the one-hot start
        ops.gmm_mstep(x, resp, self.reg_covar, st, out=par)
        ops.gmm_factor(par[2], st, out=fac)
        for _ in range(self.max_iter):                               # blind: a finished run is left untouched
            ops.gmm_estep(x, par[0], par[1], fac[0], fac[1], self.tol, st, out=resp)
            ops.gmm_mstep(x, resp, self.reg_covar, st, out=par)
            ops.gmm_factor(par[2], st, out=fac)
        ops.gmm_estep(x, par[0], par[1], fac[0], fac[1], out=resp)  # predict_proba: no state, nothing frozen or closed
        ops.gmm_relabel(resp[0], out=(None, self.pred, self.out[2]))
        ops.gmm_label_sums(zs, y_s, self.K, out=self.src)
        ops.gmm_label_sums(x, self.pred, self.K, out=self.tgt)
        ops.lsa_cos(self.tgt[0], self.src[0], st, out=self.perm)
        prob, labels, hot = ops.gmm_relabel(resp[0], self.perm[0], self.perm[1], start, st, out=self.out)
        if self.smooth_graph is not None:
            p = ops.propagate(prob, self.smooth_graph, SMOOTH_STEPS)
            ops.gmm_relabel(p, fallback=start, state=st, out=(None, labels, hot))
        return hot, labels


class Clustering(object):
    """Spherical k-means from given centres with a final alignment to them (reference :361-580).  A sweep on the device
    is one launch of the k-means step kernel and the small centre update; ``max_len`` (the reference's chunk length, there
    to bound a ``[K, len, d]`` temporary) is accepted and not used.  ``verbose`` prints the per-sweep distance."""

    def __init__(self, eps, device, max_len=1000, dist_type='cos', verbose=False):
        self.eps = eps
        self.device = device
        self.Dist = DIST(dist_type)
        self.samples = {}
        self.path2label = {}
        self.center_change = None
        self.stop = False
        self.max_len = max_len
        self.verbose = verbose

    def set_init_centers(self, init_centers):
        self.centers = init_centers
        self.init_centers = init_centers
        self.num_classes = self.centers.size(0)

    def clustering_stop(self, centers):
        if centers is None:
            self.stop = False
        else:
            dist = self.Dist.get_dist(centers, self.centers)
            dist = torch.mean(dist, dim=0)
            if self.verbose:
                print('dist %.4f' % dist.item())
            self.stop = dist.item() < self.eps

    def _metric(self):
        from .. import ops
        return ops.KMEANS_COS if self.Dist.dist_type == 'cos' else ops.KMEANS_EUC_NORMALISED

    def assign_fake_labels(self, feats):
        labels, dists, _, _ = _assign(feats, self.centers, self._metric())
        return dists, labels

    def align_centers(self):
        cost = self.Dist.get_dist(self.centers, self.init_centers, cross=True)
        cost = cost.data.cpu().numpy()
        _, col_ind = linear_sum_assignment(cost)
        return col_ind

    def collect_samples(self, feat, label):
        self.samples['gt'] = label
        self.samples['feature'] = feat
        self.samples['data'] = list(range(feat.size(0)))

    def feature_clustering(self, feat, label):
        centers = None
        self.stop = False
        self.collect_samples(feat, label)
        feature = self.samples['feature'].detach()
        while True:
            self.clustering_stop(centers)
            if centers is not None:
                self.centers = centers
            if self.stop:
                break
            _, _, sums, count = _assign(feature, self.centers, self._metric(), want_dist=False)
            mask = (count.unsqueeze(1) > 0).to(sums.dtype)
            centers = mask * sums + (1 - mask) * self.init_centers             # an empty cluster falls back to its start
        dist2center, labels = self.assign_fake_labels(feature)
        self.samples['label'] = labels
        self.samples['dist2center'] = dist2center
        cluster2label = self.align_centers()
        self.centers = self.centers[cluster2label, :]
        self.samples['label'] = torch.as_tensor(np.asarray(cluster2label), dtype=torch.int64,
                                                device=labels.device)[labels]
        self.center_change = torch.mean(self.Dist.get_dist(self.centers, self.init_centers))
        del self.samples['feature']
