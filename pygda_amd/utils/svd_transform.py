"""``svd_transform`` (pygda/utils/svd_transform.py:8-75): the dataset pre-transform SpecReg relies
on.  Attaches ``data.eival`` (sqrt of the explained variance) and ``data.eivec`` ([k, N] principal
directions) of the dense combinatorial Laplacian ``D - A``; k = 100 below 1000 nodes, else 1000.
Host-side, one-off per dataset, same estimator and seed as the reference (sklearn
``TruncatedSVD(n_iter=20, random_state=42)``); the files ``<processed_paths>eival.pt / eivec.pt``
are written as there.

``svd_transform(..., device=)`` runs the same estimator without the dense ``[N, N]`` array: the randomized range
finder's products are applications of the sparse operator to ``[N, k + 10]`` panels, every orthonormalisation is a
CholeskyQR (Gram matrix on the device, its ``(k + 10)^2`` factorisation in float64 on the host), and the final small
SVD is that of the triangular factor of ``L^T Q`` (csrc/gda_svd.hip, DESIGN "svd_transform on the device")."""
import numpy as np
import torch


def laplacian_dense(edge_index, num_nodes):
    """PyG ``get_laplacian(edge_index, normalization=None)`` scattered into a dense matrix the way
    svd_transform.py:59-64 does: self loops dropped, ``-1`` per edge (last writer wins for
    duplicates), degree on the diagonal."""
    row, col = edge_index[0].cpu().numpy(), edge_index[1].cpu().numpy()
    keep = row != col
    row, col = row[keep], col[keep]
    adj = np.zeros((num_nodes, num_nodes), dtype=np.float32)
    adj[row, col] = -1.0
    deg = np.bincount(row, minlength=num_nodes).astype(np.float32)
    adj[np.arange(num_nodes), np.arange(num_nodes)] = deg
    return adj


def svd_transform(data, processed_paths=None, device=None):
    """``device=None``: the host path below, sklearn on the dense Laplacian.  With a device: the same estimator from
    the sparse Laplacian on that device (:func:`svd_transform_device`); ``data.eival`` / ``data.eivec`` then live there."""
    if device is not None:
        return svd_transform_device(data, processed_paths, device)
    from sklearn.decomposition import TruncatedSVD
    num_node = data.y.shape[0]
    adj = laplacian_dense(data.edge_index, num_node)
    pca = TruncatedSVD(n_components=100 if num_node < 1000 else 1000, n_iter=20, random_state=42)
    pca.fit(adj)
    data.eival = torch.tensor(pca.explained_variance_ ** 0.5, dtype=torch.float32)
    data.eivec = torch.tensor(pca.components_, dtype=torch.float32)
    if processed_paths is not None:
        torch.save(data.eival, processed_paths + 'eival.pt')
        torch.save(data.eivec, processed_paths + 'eivec.pt')
    return data


N_ITER = 20                # TruncatedSVD(n_iter=20)
OVERSAMPLES = 10           # randomized_svd's n_oversamples
SEED = 42                  # random_state=42
Q0_CHUNK_ROWS = 4096       # rows of the Gaussian start panel drawn per host chunk
CHOL_RATIO = 1e-3          # smallest / largest diagonal entry of a Cholesky factor below which it is not trusted
CHOL_SHIFT = 1e-4          # relative diagonal shift of the first pass when the plain factorisation is not trusted


def n_components(num_node):
    return 100 if num_node < 1000 else 1000


def draw_q0(num_node, width, chunk_rows=Q0_CHUNK_ROWS):
    """``RandomState(42).normal(size=(N, width))`` cast to float32, in row chunks: the legacy generator fills row-major
    and keeps its spare Gaussian between calls, so the chunks are the reference's stream with bounded host memory."""
    rs = np.random.RandomState(SEED)
    for r0 in range(0, num_node, chunk_rows):
        rows = min(chunk_rows, num_node - r0)
        yield r0, rs.normal(size=(rows, width)).astype(np.float32)


def _breakdown(what):
    from .. import _lib
    return _lib.GdaError(f"svd_transform: the factorisation broke down ({what}): the Laplacian's numerical rank is "
                         "below k + 10; use the host path (device=None) or a graph with fewer isolated nodes")


def cholesky_factor(G, first_pass):
    """Upper ``R`` with ``R^T R = G`` (float64, host) and whether a shift was needed.  A factor whose diagonal spans
    more than 1 / CHOL_RATIO is not trusted: on the first pass of an orthonormalisation ``G`` is then shifted (the next
    passes repair the result), on a later pass the panel has lost rank."""
    if not bool(torch.isfinite(G).all()):
        raise _breakdown("a non-finite Gram matrix")

    def trusted(M):
        Lf, info = torch.linalg.cholesky_ex(M)
        d = Lf.diagonal()
        return Lf, int(info) == 0 and bool(torch.isfinite(d).all()) and float(d.min()) > CHOL_RATIO * float(d.max())

    Lf, ok = trusted(G)
    if ok:
        return Lf.T, False
    if not first_pass:
        raise _breakdown("a Gram matrix without a trusted Cholesky factor")
    top = float(G.diagonal().max())
    if not top > 0.0:
        raise _breakdown("a zero panel")
    Lf, info = torch.linalg.cholesky_ex(G + CHOL_SHIFT * top * torch.eye(G.size(0), dtype=G.dtype))
    if int(info) != 0:
        raise _breakdown("a Gram matrix that is not positive definite")
    return Lf.T, True


def _orthonormalise(Y, T, passes=2):
    """CholeskyQR of the panel ``Y`` (``T`` is a spare panel): ``(Q, spare, R)`` with ``Y = Q R``, ``R`` float64 on the
    host.  ``passes=2`` is CholeskyQR2 (orthonormal to fp32 rounding); ``passes=1`` leaves an error of cond(Y)^2 eps,
    enough for a power iteration, whose normaliser only has to keep the span.  Three passes whenever the first one
    needed a shift."""
    from .. import ops
    w = Y.size(1)
    R_total = torch.eye(w, dtype=torch.float64)
    p = 0
    while p < passes:
        G = ops.svd_gram(Y).cpu().double()
        R, shifted = cholesky_factor(G, p == 0)
        if shifted:
            passes = 3
        Rinv = torch.linalg.solve_triangular(R, torch.eye(w, dtype=torch.float64), upper=True)
        ops.svd_panel_matmul(Y, Rinv.float().to(Y.device), T)
        Y, T = T, Y
        R_total = R @ R_total
        p += 1
    return Y, T, R_total


def svd_transform_device(data, processed_paths, device):
    from .. import ops
    device = torch.device(device)
    num_node = int(data.y.shape[0])
    k = n_components(num_node)
    w = k + OVERSAMPLES
    if num_node < w:
        raise ValueError(f"svd_transform(device=...) needs at least k + {OVERSAMPLES} = {w} nodes, got {num_node}: "
                         "use the host path (device=None)")
    op = ops.SvdLaplacian(data.edge_index.to(device), num_node)
    Q, T = ops.svd_panel(num_node, w, device), ops.svd_panel(num_node, w, device)
    for r0, block in draw_q0(num_node, w):
        Q[r0:r0 + block.shape[0]].copy_(torch.from_numpy(block))
    # randomized_range_finder: 20 x (Q <- norm(L Q); Q <- norm(L^T Q)), then Q <- qr(L Q); the normaliser is free
    for it in range(2 * N_ITER + 1):
        op.apply(Q, transposed=bool(it % 2), out=T)
        Q, T, _ = _orthonormalise(T, Q, passes=1 if it < 2 * N_ITER else 2)
    # B = Q^T L = Z^T with Z = L^T Q = P R: B = R^T P^T = Vr S (P Ur)^T, so Vt = (P Ur)^T from the SVD of R alone
    op.apply(Q, transposed=True, out=T)
    P, T, R = _orthonormalise(T, Q)
    Ur, S, _ = torch.linalg.svd(R)
    if not bool(torch.isfinite(Ur).all()):
        raise _breakdown("a non-finite small SVD")
    V = ops.svd_panel(num_node, k, device)
    ops.svd_panel_matmul(P, Ur[:, :k].float().contiguous().to(device), V)
    # svd_flip(u_based_decision=False): the entry of largest magnitude of every row of Vt positive, first index on ties
    top = V.abs().argmax(dim=0, keepdim=True)
    sign = torch.sign(V.gather(0, top))
    sign = torch.where(sign == 0, torch.ones_like(sign), sign)
    V.mul_(sign)
    # explained_variance_ = var(L Vt^T, axis=0), ddof = 0, from the column moments of the product (never written)
    m = op.moments(V)
    mean = m[0] / num_node
    var = (m[1] / num_node - mean * mean).clamp_min(0.0)
    eival = var.sqrt().to(torch.float32)
    eivec = V.t().contiguous()
    if not (bool(torch.isfinite(eival).all()) and bool(torch.isfinite(eivec).all())):
        raise _breakdown("non-finite bases")
    data.eival, data.eivec = eival, eivec
    if processed_paths is not None:
        torch.save(data.eival.cpu(), processed_paths + 'eival.pt')
        torch.save(data.eivec.cpu(), processed_paths + 'eivec.pt')
    return data
