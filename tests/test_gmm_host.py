"""CPU: the surface of ``pygda.nn.GMMClustering`` / ``pygda.nn.gmm_clustering``, the argument validation of the gda_gmm_*
and gda_kmeans_* entry points (status codes come back before anything touches a device), the torch restatement of the EM
loop against sklearn in float64 from the same start, and the yardsticks of tests/test_gpu_gmm.py: the test mixtures,
sklearn's fits of them in float64 and float32, and the tolerance rule.

Tolerances.  None is taken from the code under test.  For every compared quantity the yardstick is the deviation of
sklearn in float32 from sklearn in float64 on the SAME input and start; float32 results (the device, the float32 CPU
path) may deviate from sklearn float64 by four times that (the kernels add over slabs and MFMA lanes in an order numpy
does not use), with an absolute floor of 1e-6.  Measured yardsticks on the four inputs (absolute): means 2.5e-7 .. 2.5e-6,
covariances 3.2e-7 .. 4.2e-6, probabilities 4.3e-7 .. 3.7e-4 (the 33-column input has rows between two components), lower
bound 6.4e-7 .. 9.3e-6 -- the constants are computed from the fits, by ``tolerances``, not copied.  The float64 CPU path is held to 1e-9: it is the same arithmetic as sklearn's up to
the order of a few sums.
"""
import ctypes
import functools
import os
import re
import warnings

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment
from sklearn.mixture import GaussianMixture

from pygda_amd import _build, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SIZE, WORKSPACE, UNSUPPORTED, ALIAS = -1, -2, -3, -4, -5
TOL, REG = 1e-3, 1e-6                                   # sklearn's defaults

# (N, d, K): (centre spread in sigma, seed).  Seeds chosen so that sklearn itself is unambiguous on the input: float32 and
# float64 stop at the same iteration with the same labels, and the stopping change is far from tol on both sides
# (asserted by test_inputs_are_not_borderline).  They converge in 6, 20, 8 and 4 iterations.
CASES = {(257, 3, 2): (3.0, 3), (1000, 33, 7): (5.0, 26), (640, 64, 5): (4.0, 1), (1500, 128, 6): (4.0, 7)}


@functools.lru_cache(maxsize=None)
def mixture(N, d, K, spread, seed, noise=0.3):
    """``(x [N, d], true labels, resp0 [N, K])`` in float64: K anisotropic Gaussians whose centres lie ``spread`` sigma
    apart, and the one-hot true labels with a fraction ``noise`` of the rows reassigned at random."""
    rng = np.random.RandomState(seed)
    cen = rng.normal(size=(K, d)) * spread / np.sqrt(2 * d)
    lab = rng.randint(0, K, N)
    A = [np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d) for _ in range(K)]
    x = np.stack([cen[l] + A[l] @ rng.normal(size=d) for l in lab])
    noisy = lab.copy()
    m = rng.rand(N) < noise
    noisy[m] = rng.randint(0, K, m.sum())
    return x, lab, np.eye(K)[noisy]


def case_input(case):
    return mixture(*case, *CASES[case])


def start_params(x, resp0, reg=REG):
    """``(weights, means, precisions)`` of sklearn's initial M-step from ``resp0``, in float64."""
    nk = resp0.sum(0) + 10 * np.finfo(np.float64).eps
    means = resp0.T @ x / nk[:, None]
    prec = []
    for k in range(resp0.shape[1]):
        diff = x - means[k]
        prec.append(np.linalg.inv((resp0[:, k] * diff.T) @ diff / nk[k] + reg * np.eye(x.shape[1])))
    return nk / nk.sum(), means, np.array(prec)


@functools.lru_cache(maxsize=None)
def sklearn_fit(case, dtype):
    """sklearn's fit of the case from ``resp0`` in ``dtype`` ('float64' / 'float32'): the fitted estimator."""
    x, _, r0 = case_input(case)
    w, mu, pr = start_params(x, r0)
    dt = np.dtype(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return GaussianMixture(case[2], n_init=1, tol=TOL, reg_covar=REG, weights_init=w.astype(dt),
                               means_init=mu.astype(dt), precisions_init=pr.astype(dt)).fit(x.astype(dt))


def floor4(dev):
    return max(4.0 * float(dev), 1e-6)


@functools.lru_cache(maxsize=None)
def tolerances(case):
    """The yardsticks (sklearn float32 against sklearn float64 on this input) times four, floored at 1e-6."""
    x = case_input(case)[0]
    a, b = sklearn_fit(case, "float64"), sklearn_fit(case, "float32")
    return {"means": floor4(np.abs(a.means_ - b.means_).max()),
            "covariances": floor4(np.abs(a.covariances_ - b.covariances_).max()),
            "proba": floor4(np.abs(a.predict_proba(x) - b.predict_proba(x.astype(np.float32))).max()),
            "lower_bound": floor4(abs(a.lower_bound_ - float(b.lower_bound_)))}


def check_fit_against_sklearn(case, model, proba, tol=None):
    """``model`` (a FittedMixture) and its ``proba`` on the case's rows against sklearn float64."""
    x = case_input(case)[0]
    ref = sklearn_fit(case, "float64")
    t = tolerances(case) if tol is None else dict.fromkeys(("means", "covariances", "proba", "lower_bound"), tol)
    got = {"means": model.means_, "covariances": model.covariances_, "proba": proba}
    figures = {k: float(np.abs(v.detach().cpu().double().numpy() - (ref.predict_proba(x) if k == "proba"
                                                                    else getattr(ref, k + "_"))).max())
               for k, v in got.items()}
    figures["lower_bound"] = abs(model.lower_bound_ - ref.lower_bound_)
    print(case, "n_iter", model.n_iter_, ref.n_iter_, {k: (figures[k], t[k]) for k in figures})
    assert model.n_iter_ == ref.n_iter_ and model.converged_ == ref.converged_            # conditions, not measurements
    assert np.array_equal(proba.argmax(1).cpu().numpy(), ref.predict(x))                    # labels equal on every row
    for k in figures:
        assert figures[k] <= t[k], (k, figures[k], t[k])


# ---------------------------------------------------------------------------------------------------- surface --
def test_surface_and_limits():
    from pygda.nn import GMMClustering
    import pygda.nn.gmm_clustering as M
    import pygda_amd.nn.gmm_clustering as A
    assert M is A and M.GMMClustering is GMMClustering
    for name in ("Clustering", "DIST", "onehot", "get_emb_centers", "gcn_norm"):
        assert hasattr(M, name), name
    assert "gda_gmm.hip" in _build.SOURCES
    header = open(os.path.join(ROOT, "include", "gda_hip.h")).read()
    lim = {k: int(v) for k, v in re.findall(r"#define (GDA_GMM_MAX_\w+) (\d+)", header)}
    assert lim == {"GDA_GMM_MAX_DIM": ops.GMM_MAX_DIM, "GDA_GMM_MAX_COMPONENTS": ops.GMM_MAX_COMPONENTS,
                   "GDA_GMM_MAX_RUNS": ops.GMM_MAX_RUNS} and lim["GDA_GMM_MAX_DIM"] == 128
    assert ctypes.sizeof(ctypes.c_double) * 2 + 4 * 4 == 32                                  # gda_gmm_state
    with pytest.raises(_lib.GdaError, match="128 columns"):
        ops.gmm_check_limits(129, 3, 1)
    with pytest.raises(_lib.GdaError):
        ops.gmm_check_limits(8, 33, 1)
    with pytest.raises(_lib.GdaError):
        ops.gmm_check_limits(8, 3, 9)
    with pytest.raises(NotImplementedError):
        M.gcn_norm(object())


# ------------------------------------------------------------------------------------------------ ABI refusals --
def P(addr):
    return ctypes.c_void_p(addr)


X, RESP, W, MU, COV, PREC, LD, ST, WS, CEN, LAB, SUMS, CNT = (P(0x1000 * k) for k in range(1, 14))
BIG = 1 << 40


def mstep(x=X, ldx=130, n=100, d=128, k=6, r=5, resp=RESP, w=W, mu=MU, cov=COV, st=ST, ws=WS, ws_bytes=BIG):
    return _lib.lib().gda_gmm_mstep_f32(x, ldx, n, d, k, r, resp, 1e-6, w, mu, cov, st, ws, ws_bytes, None)


def factor(cov=COV, d=128, k=6, r=5, prec=PREC, ld=LD, st=ST):
    return _lib.lib().gda_gmm_factor_f32(cov, d, k, r, prec, ld, st, None)


def estep(x=X, ldx=130, n=100, d=128, k=6, r=5, w=W, mu=MU, prec=PREC, ld=LD, resp=RESP, st=ST, ws=WS, ws_bytes=BIG):
    return _lib.lib().gda_gmm_estep_f32(x, ldx, n, d, k, r, w, mu, prec, ld, resp, 1e-3, st, ws, ws_bytes, None)


def kmeans(x=X, ldx=130, n=100, d=128, k=6, cen=CEN, metric=0, lab=LAB, dist=None, sums=SUMS, cnt=CNT, ws=WS,
           ws_bytes=BIG):
    return _lib.lib().gda_kmeans_step_f32(x, ldx, n, d, k, cen, metric, lab, dist, sums, cnt, ws, ws_bytes, None)


def test_mstep_validates_its_arguments():
    for missing in ("x", "resp", "w", "mu", "cov"):
        assert mstep(**{missing: None}) == NULL, missing
    for bad in ("n", "d", "k", "r"):
        assert mstep(**{bad: -1}) == SIZE and mstep(**{bad: 0}) == SIZE, bad
    assert mstep(ldx=127) == SIZE and mstep(n=1 << 31) == SIZE
    assert mstep(d=129, ldx=129) == UNSUPPORTED and mstep(k=33) == UNSUPPORTED and mstep(r=9) == UNSUPPORTED
    need = _lib.lib().gda_gmm_mstep_workspace_bytes(100, 128, 6, 5)
    # one slab of 128 rows: [5, 1, 6, 129] sums, [5, 6] nk, 5 * 6 * 3 tiles of 64 x 64
    assert need == 5 * 6 * 129 * 4 + 8 + 5 * 6 * 4 + 8 + 5 * 6 * 3 * 64 * 64 * 4
    assert mstep(ws=None, ws_bytes=0) == WORKSPACE and mstep(ws_bytes=need - 1) == WORKSPACE
    assert mstep(ws=P(0x6004), ws_bytes=need) == UNSUPPORTED
    L = _lib.lib()
    assert L.gda_gmm_mstep_workspace_bytes(0, 8, 2, 1) == 0 and L.gda_gmm_mstep_workspace_bytes(10, 129, 2, 1) == 0
    # 7410 x 128, 6 components: 2048 / (3 tiles * 6 * 8 runs) = 14 slabs of 544 rows, whatever the number of runs
    assert L.gda_gmm_mstep_workspace_bytes(7410, 128, 6, 5) == 5 * 14 * 6 * 129 * 4 + 5 * 6 * 4 + 8 \
        + 5 * 6 * 14 * 3 * 64 * 64 * 4
    assert L.gda_gmm_mstep_workspace_bytes(7410, 128, 6, 1) == 14 * 6 * 129 * 4 + 6 * 4 + 8 + 6 * 14 * 3 * 64 * 64 * 4


def test_factor_validates_its_arguments():
    for missing in ("cov", "prec", "ld", "st"):
        assert factor(**{missing: None}) == NULL, missing
    for bad in ("d", "k", "r"):
        assert factor(**{bad: -1}) == SIZE and factor(**{bad: 0}) == SIZE, bad
    assert factor(d=129) == UNSUPPORTED and factor(k=33) == UNSUPPORTED and factor(r=9) == UNSUPPORTED
    assert factor(prec=COV) == ALIAS


def test_estep_validates_its_arguments():
    for missing in ("x", "w", "mu", "prec", "ld", "resp"):
        assert estep(**{missing: None}) == NULL, missing
    for bad in ("n", "d", "k", "r"):
        assert estep(**{bad: -1}) == SIZE and estep(**{bad: 0}) == SIZE, bad
    assert estep(ldx=127) == SIZE
    assert estep(d=129, ldx=129) == UNSUPPORTED and estep(k=33) == UNSUPPORTED and estep(r=9) == UNSUPPORTED
    need = _lib.lib().gda_gmm_estep_workspace_bytes(100, 5)
    assert need == 5 * 2 * 8                                                    # two blocks of 64 rows per run, float64
    assert estep(ws=None, ws_bytes=0) == WORKSPACE and estep(ws_bytes=need - 1) == WORKSPACE
    assert estep(ws=P(0x6008), ws_bytes=need) == UNSUPPORTED
    assert _lib.lib().gda_gmm_estep_workspace_bytes(0, 5) == 0 and _lib.lib().gda_gmm_estep_workspace_bytes(5, 9) == 0


def test_kmeans_step_validates_its_arguments():
    for missing in ("x", "cen", "lab", "sums", "cnt"):
        assert kmeans(**{missing: None}) == NULL, missing
    for bad in ("n", "d", "k"):
        assert kmeans(**{bad: -1}) == SIZE and kmeans(**{bad: 0}) == SIZE, bad
    assert kmeans(ldx=127) == SIZE
    assert kmeans(d=129, ldx=129) == UNSUPPORTED and kmeans(k=33) == UNSUPPORTED
    assert kmeans(metric=3) == UNSUPPORTED and kmeans(metric=-1) == UNSUPPORTED
    need = _lib.lib().gda_kmeans_step_workspace_bytes(100, 128, 6)
    assert need == 2 * 6 * 129 * 4                                              # two blocks of 64 rows
    assert kmeans(ws=None, ws_bytes=0) == WORKSPACE and kmeans(ws_bytes=need - 1) == WORKSPACE
    assert kmeans(ws=P(0x6004), ws_bytes=need) == UNSUPPORTED


# ------------------------------------------------------------------------------------ the CPU path against sklearn --
@pytest.mark.parametrize("case", list(CASES))
def test_inputs_are_not_borderline(case):
    """An input fault, not a code fault, if this fails: sklearn itself must be unambiguous on the input."""
    x = case_input(case)[0]
    a, b = sklearn_fit(case, "float64"), sklearn_fit(case, "float32")
    assert a.converged_ and b.converged_ and a.n_iter_ == b.n_iter_ and 4 <= a.n_iter_ <= 24
    assert np.array_equal(a.predict(x), b.predict(x.astype(np.float32)))
    change = np.abs(np.diff([-np.inf] + list(a.lower_bounds_)))
    assert change[-1] < TOL / 4 and change[-2] > 4 * TOL, change[-2:]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_cpu_em_matches_sklearn_from_the_same_start(case, dtype):
    from pygda.nn import GMMClustering
    x, _, r0 = case_input(case)
    xt = torch.tensor(x, dtype=dtype)
    c = GMMClustering(case[2], "cpu")
    model = c.fit_em(xt, torch.tensor(r0, dtype=dtype))
    assert c.gmm is model and model.means_.dtype == dtype
    for name in ("weights_", "means_", "covariances_", "precisions_cholesky_", "lower_bound_", "n_iter_", "converged_",
                 "predict", "predict_proba"):
        assert hasattr(model, name), name
    proba = model.predict_proba(xt)
    assert torch.equal(model.predict(xt), proba.argmax(1))
    check_fit_against_sklearn(case, model, proba, tol=1e-9 if dtype == torch.float64 else None)
    ref = sklearn_fit(case, "float64")
    np.testing.assert_allclose(model.weights_.double().numpy(), ref.weights_, atol=1e-6)
    np.testing.assert_allclose(model.precisions_cholesky_.double().numpy(), ref.precisions_cholesky_,
                               atol=1e-9 if dtype == torch.float64 else 4 * max(
                                   1e-6, np.abs(sklearn_fit(case, "float32").precisions_cholesky_
                                                - ref.precisions_cholesky_).max()))


def test_restarts_keep_the_largest_lower_bound():
    from pygda.nn import GMMClustering
    case = (257, 3, 2)
    x, lab, r0 = case_input(case)
    rng = np.random.RandomState(0)
    bad = np.eye(2)[rng.randint(0, 2, len(x))]                                  # a start without information
    xt = torch.tensor(x)
    c = GMMClustering(2, "cpu")
    both = c.fit_em(xt, torch.tensor(np.stack([bad, r0])))
    alone = [c.fit_em(xt, torch.tensor(r)) for r in (bad, r0)]
    best = max(alone, key=lambda m: m.lower_bound_)
    assert both.lower_bound_ == best.lower_bound_ and torch.equal(both.means_, best.means_)


def test_non_positive_pivot_raises_sklearns_error():
    from pygda.nn import GMMClustering
    x = torch.tensor([[1.0, 2.0], [1.0, 2.0], [0.0, 0.5], [3.0, -1.0], [2.0, 2.0], [-1.0, 0.0]], dtype=torch.float64)
    r0 = torch.zeros(6, 2, dtype=torch.float64)
    r0[:2, 0] = 1                                                               # two identical rows are a whole component
    r0[2:, 1] = 1
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        GMMClustering(2, "cpu", reg_covar=0.0).fit_em(x, r0)


# ---------------------------------------------------------------------------------------------------- forward --
def separated(n=240, d=8, K=4, seed=5):
    rng = np.random.RandomState(seed)
    cen = rng.normal(size=(K, d)) * 6
    lab = np.arange(n) % K
    return cen, lab, cen[lab] + rng.normal(size=(n, d))


def quirky_graph(n, seed=0):
    """Duplicate edges, a self loop, an isolated last node; weights in (0.5, 1.5)."""
    rng = np.random.RandomState(seed)
    s, d = rng.randint(0, n - 1, 4 * n), rng.randint(0, n - 1, 4 * n)
    s, d = np.concatenate([s, s[:7], [3]]), np.concatenate([d, d[:7], [3]])
    return torch.tensor(np.stack([s, d])), torch.tensor(rng.uniform(0.5, 1.5, len(s)), dtype=torch.float32)


def smooth_reference(edge_index, v, p, r, n, steps=20):
    """Dense float64 restatement of reference :327-336: diagonal SET to 1, degree = row sums, both sides normalised."""
    A = np.zeros((n, n))
    np.add.at(A, (edge_index[0].numpy(), edge_index[1].numpy()), v.double().numpy())
    np.fill_diagonal(A, 1.0)
    dis = A.sum(1) ** -0.5
    A = dis[:, None] * A * dis[None, :]
    p = p.double().numpy()
    for _ in range(steps):
        p = r * p + (1 - r) * (A @ p)
    return p


def test_forward_dict_labels_and_alignment():
    import pygda.nn.gmm_clustering as M
    cen, lab, x = separated()
    n, K = len(x), len(cen)
    perm = np.array([2, 0, 3, 1])
    src = torch.tensor(cen[perm], dtype=torch.float32)                          # source class c sits at cluster perm[c]
    emb = torch.tensor(x, dtype=torch.float32)
    y = torch.tensor(lab)
    c = M.GMMClustering(K, "cpu", seed=3)
    out = c.forward(src, emb, y, None, None, False, 0.5)
    assert set(out) == {"data", "label", "dist2center", "gt"} and out["data"] == list(range(n)) and out["gt"] is y
    assert out["label"].dtype == torch.int64 and out["label"].shape == (n,)
    assert out["dist2center"].dtype == torch.float32 and out["dist2center"].shape == (n, K)
    assert c.target_pred.dtype == torch.int32 and c.num_nodes == n and c.samples is out
    assert torch.equal(out["dist2center"].argmax(1), out["label"])
    want = np.argsort(perm)[lab]                                                # the source class of every row
    assert np.array_equal(out["label"].numpy(), want)
    # shuffle_idx is the inverse of the assignment: column j of the re-arranged probabilities is cluster i with c2l[i] = j
    tgt = M.get_emb_centers(emb, c.target_pred, K)
    c2l = c.align_centers(src, tgt)
    raw = c.gmm.predict_proba(emb)
    assert torch.equal(out["dist2center"][:, c2l], raw)
    # seeded: the same draw twice
    again = M.GMMClustering(K, "cpu", seed=3).forward(src, emb, y, None, None, False, 0.5)
    assert torch.equal(again["dist2center"], out["dist2center"])


def test_forward_with_smoothing_and_smooth_against_dense_float64():
    import pygda.nn.gmm_clustering as M
    cen, lab, x = separated()
    n, K = len(x), len(cen)
    ei, v = quirky_graph(n)
    emb = torch.tensor(x, dtype=torch.float32)
    c = M.GMMClustering(K, "cpu", seed=1)
    out = c.forward(torch.tensor(cen, dtype=torch.float32), emb, torch.tensor(lab), ei, v, True, 0.7)
    assert torch.equal(out["label"], c.smooth_labels) and torch.equal(out["label"], out["dist2center"].argmax(1))
    rng = np.random.RandomState(2)
    c.target_pred_prob = torch.tensor(rng.dirichlet(np.ones(K), n), dtype=torch.float32)     # soft rows: smoothing acts
    labels, p = c.smooth(ei, v, 0.7)
    want = smooth_reference(ei, v, c.target_pred_prob, 0.7, n)
    # 20 steps of a convex combination of float32 rows: below 20 * 2^-23 of the largest entry (1)
    assert np.abs(p.double().numpy() - want).max() < 20 * 2.0 ** -23
    assert np.array_equal(labels.numpy(), want.argmax(1))
    assert np.abs(want[-1] - c.target_pred_prob[-1].double().numpy()).max() < 1e-12      # the isolated node keeps its row


def test_helpers_follow_the_reference():
    import pygda.nn.gmm_clustering as M
    emb = torch.tensor([[1.0, 0.0], [3.0, 1.0], [0.0, 2.0]])
    lab = torch.tensor([1, 1, 0])
    sums = M.get_emb_centers(emb, lab, 2)
    assert torch.equal(sums, torch.tensor([[0.0, 2.0], [4.0, 1.0]]))           # sums, not means
    assert torch.equal(M.onehot(lab, 3), torch.eye(3)[lab])
    A, B = torch.tensor([[1.0, 0.0], [0.0, 2.0]]), torch.tensor([[0.0, 3.0], [0.0, 5.0]])
    cos, euc = M.DIST("cos"), M.DIST("euc")
    assert torch.allclose(cos.get_dist(A, B), torch.tensor([0.5, 0.0]))
    assert torch.allclose(cos.get_dist(A, B, cross=True), torch.tensor([[0.5, 0.5], [0.0, 0.0]]))
    assert euc.get_dist(A, B).dim() == 0 and torch.allclose(euc.get_dist(A, B), torch.tensor(2.0 ** 0.5))   # ONE norm
    assert torch.allclose(euc.get_dist(A, B, cross=True), torch.tensor([[2.0 ** 0.5] * 2, [0.0, 0.0]]), atol=1e-6)
    # align_centers against scipy on a designed cost: the greedy choice (row 0 -> column 0) is not the optimum
    g = M.GMMClustering(3, "cpu")
    src = torch.tensor([[1.0, 0.0, 0.0], [0.9, 0.1, 0.0], [0.0, 0.0, 1.0]])
    tgt = torch.tensor([[1.0, 0.05, 0.0], [1.0, 0.0, 0.0], [0.1, 0.0, 1.0]])
    cost = cos.get_dist(tgt, src, cross=True).numpy()
    assert np.array_equal(g.align_centers(src, tgt), linear_sum_assignment(cost)[1])
    assert list(g.align_centers(src, tgt)) == [1, 0, 2]


# ------------------------------------------------------------------------------------------------- Clustering --
def kmeans_reference(feat, init, dist, eps):
    """A straight torch restatement of the reference's sweep loop (no chunking): labels, distances, centres, change."""
    centers, new = init, None
    K = init.size(0)
    while True:
        if new is not None:
            stop = torch.mean(dist.get_dist(new, centers), dim=0).item() < eps
            centers = new
            if stop:
                break
        lab = dist.get_dist(feat, centers, cross=True).min(1)[1]
        hot = torch.eye(K, dtype=feat.dtype)[lab]
        mask = (hot.sum(0)[:, None] > 0).to(feat.dtype)
        new = mask * (hot.T @ feat) + (1 - mask) * init
    d2c = dist.get_dist(feat, centers, cross=True)
    lab = d2c.min(1)[1]
    c2l = linear_sum_assignment(dist.get_dist(centers, init, cross=True).numpy())[1]
    centers = centers[c2l]
    return torch.as_tensor(c2l)[lab], d2c, centers, torch.mean(dist.get_dist(centers, init))


def clustering_inputs(empty):
    rng = np.random.RandomState(11)
    cen = rng.normal(size=(4, 6)) * 3
    feat = torch.tensor(cen[np.arange(150) % 3] + rng.normal(size=(150, 6)), dtype=torch.float32)
    init = torch.tensor(cen + 0.5 * rng.normal(size=cen.shape), dtype=torch.float32)
    if empty:
        init[3] = -feat.mean(0) * 5                                             # opposite to every row: nobody picks it
    else:
        feat = torch.cat([feat, torch.tensor(cen[3] + rng.normal(size=(50, 6)), dtype=torch.float32)])
    return feat, init


@pytest.mark.parametrize("dist_type", ["cos", "euc"])
@pytest.mark.parametrize("empty", [False, True])
def test_feature_clustering_against_a_torch_restatement(dist_type, empty, capsys):
    import pygda.nn.gmm_clustering as M
    feat, init = clustering_inputs(empty)
    eps = 1e-6 if dist_type == "cos" else 1e-3
    c = M.Clustering(eps, "cpu", max_len=64, dist_type=dist_type)
    c.set_init_centers(init)
    gt = torch.zeros(len(feat), dtype=torch.int64)
    c.feature_clustering(feat, gt)
    lab, d2c, centers, change = kmeans_reference(feat, init, M.DIST(dist_type), eps)
    assert capsys.readouterr().out == ""                                        # the per-sweep print is behind `verbose`
    assert set(c.samples) == {"gt", "data", "label", "dist2center"} and c.samples["gt"] is gt
    assert torch.equal(c.samples["label"], lab)
    assert torch.allclose(c.samples["dist2center"], d2c, atol=1e-6) and torch.allclose(c.centers, centers, atol=1e-4)
    assert torch.allclose(c.center_change, change, atol=1e-6) and c.stop
    if empty:
        assert 3 not in set(c.samples["label"].tolist()) and torch.equal(c.centers[3], init[3])


# ------------------------------------------------------------------------------------- the reference's own results --
# tests/golden/gmm_clustering.npz: the reference's gmm_clustering.py run on the PyG stub (tests/golden/make_golden_gmm.py).
@pytest.mark.parametrize("dist_type", ["cos", "euc"])
@pytest.mark.parametrize("empty", [False, True])
def test_feature_clustering_against_the_reference_golden(dist_type, empty):
    import pygda.nn.gmm_clustering as M
    from tests.conftest import load_golden, sub
    want = sub(load_golden("gmm_clustering"), f"clustering/{dist_type}/{int(empty)}/")
    feat, init = clustering_inputs(empty)
    c = M.Clustering(1e-6 if dist_type == "cos" else 1e-3, "cpu", max_len=64, dist_type=dist_type)
    c.set_init_centers(init)
    c.feature_clustering(feat, torch.zeros(len(feat), dtype=torch.int64))
    assert np.array_equal(c.samples["label"].numpy(), want["label"])                        # labels exactly
    # the same float32 expressions; only the reference's chunks of 64 rows order the centre sums differently
    assert np.abs(c.samples["dist2center"].numpy() - want["dist2center"]).max() <= 1e-6
    # a centre is a sum of at most 200 float32 rows, added in another order
    assert np.abs(c.centers.numpy() - want["centers"]).max() <= 200 * 2.0 ** -24 * np.abs(want["centers"]).max()
    assert abs(float(c.center_change) - float(want["center_change"])) <= 1e-6


def test_forward_against_the_reference_golden():
    """The reference draws its starts from numpy's global state and this project from its own generator; on separated
    embeddings both reach the same mixture, so labels are pinned exactly.  The probabilities are saturated there (the
    float32-against-float64 yardstick is 0): the floor of the rule, 1e-6, applies; the kept lower bounds are those of two
    float32 EM runs that stop within tol of the optimum, so they agree within tol."""
    import pygda.nn.gmm_clustering as M
    from tests.conftest import load_golden, sub
    want = sub(load_golden("gmm_clustering"), "gmm/")
    cen, lab, x = separated()
    src = torch.tensor(cen[want["perm"]], dtype=torch.float32)
    c = M.GMMClustering(len(cen), "cpu", seed=0)
    out = c.forward(src, torch.tensor(x, dtype=torch.float32), torch.tensor(lab), None, None, False, 0.5)
    assert np.array_equal(out["label"].numpy(), want["label"])
    assert np.abs(out["dist2center"].numpy() - want["dist2center"]).max() <= 1e-6
    assert abs(c.gmm.lower_bound_ - float(want["lower_bound"])) <= TOL
