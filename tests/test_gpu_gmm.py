"""GPU: the mixture and k-means kernels of csrc/gda_gmm.hip, single steps against float64 and the full EM loop against
sklearn float64 (inputs, fits and the tolerance rule come from tests/test_gmm_host.py).

Tolerances of the single-step tests follow the same rule as the fits: the yardstick is sklearn's OWN routine for that
step in float32 against float64 on the test's input (``_estimate_gaussian_parameters``, ``_compute_precision_cholesky``,
``predict_proba`` / ``score`` of an estimator carrying the parameters), the kernel gets four times that, floored at 1e-6.
Measured yardsticks over the shape grid: weights <= 3.0e-7, means <= 2.5e-7, covariances <= 1.7e-6, probabilities
<= 1.2e-5, mean log-likelihood <= 1.2e-5 (the value itself is near -200 at 128 columns); the kernels deviate by at most
4.9e-8, 1.6e-7, 1.8e-6, 3.9e-6 and 7.1e-7.  Each test computes its own constants from its input and prints them with the
figures.
"""
import functools

import numpy as np
import pytest
import torch
from scipy.linalg import solve_triangular
from sklearn.mixture import GaussianMixture
from sklearn.mixture import _gaussian_mixture as skm

from tests.test_gmm_host import (CASES, REG, TOL, case_input, check_fit_against_sklearn, clustering_inputs, floor4,
                                 quirky_graph, separated, sklearn_fit)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every N of {1, 63, 64, 65, 257, 1000}, d of {1, 3, 32, 33, 64, 65, 127, 128}, K of {1, 2, 7, 32}, R of {1, 5}
GRID = [(1, 1, 1, 1), (63, 3, 2, 1), (64, 32, 7, 5), (65, 33, 2, 1), (257, 64, 7, 1), (257, 65, 1, 5), (1000, 127, 2, 1),
        (1000, 128, 32, 5)]


def panel(x):
    """``x`` on the device as a column view of a wider block whose padding is NaN."""
    n, d = x.shape
    block = torch.full((n, d + 5), float("nan"), dtype=torch.float32, device=DEV)
    block[:, :d] = torch.as_tensor(x, dtype=torch.float32)
    return block[:, :d]


@functools.lru_cache(maxsize=None)
def soft_case(N, d, K, R):
    """Overlapping clusters (centres one sigma apart) and SOFT responsibilities, no row saturated: ``x [N, d]``,
    ``resp [R, N, K]`` (rows sum to 1), and well-conditioned parameters for the E-step, all float64."""
    rng = np.random.RandomState(N * 131 + d * 7 + K + R)
    cen = rng.normal(size=(K, d)) / np.sqrt(2 * d)
    x = cen[rng.randint(0, K, N)] + rng.normal(size=(N, d))
    resp = rng.dirichlet(np.full(K, 2.0), size=(R, N))
    means = cen[None] + 0.1 * rng.normal(size=(R, K, d))
    cov = np.empty((R, K, d, d))
    for r in range(R):
        for k in range(K):
            A = rng.normal(size=(d, 2 * d + 3))
            cov[r, k] = A @ A.T / (2 * d + 3) + 0.1 * np.eye(d)
    weights = rng.dirichlet(np.full(K, 5.0), size=R)
    return x, resp, weights, means, cov


def T(a):
    return torch.as_tensor(a, dtype=torch.float32).to(DEV)


def N64(t):
    return t.detach().cpu().double().numpy()


def estimator(weights, means, cov, dtype):
    g = GaussianMixture(len(weights))
    g.weights_, g.means_, g.covariances_ = weights.astype(dtype), means.astype(dtype), cov.astype(dtype)
    g.precisions_cholesky_ = skm._compute_precision_cholesky(g.covariances_, "full")
    return g


# ------------------------------------------------------------------------------------------------------ M-step --
@pytest.mark.parametrize("shape", GRID)
def test_mstep_against_float64(shape):
    from pygda_amd import ops
    N, d, K, R = shape
    x, resp = soft_case(*shape)[:2]
    w, mu, cov = ops.gmm_mstep(panel(x), T(resp), REG)
    torch.cuda.synchronize()
    assert torch.equal(cov, cov.transpose(2, 3))                                # symmetric bit for bit
    for r in range(R):
        nk, m64, c64 = skm._estimate_gaussian_parameters(x, resp[r], REG, "full")
        nk32, m32, c32 = skm._estimate_gaussian_parameters(x.astype(np.float32), resp[r].astype(np.float32), REG, "full")
        fig = (np.abs(N64(w[r]) - nk / nk.sum()).max(), np.abs(N64(mu[r]) - m64).max(), np.abs(N64(cov[r]) - c64).max())
        tol = (floor4(np.abs(nk32 / nk32.sum() - nk / nk.sum()).max()), floor4(np.abs(m32 - m64).max()),
               floor4(np.abs(c32 - c64).max()))
        print(shape, r, "weights/means/covariances", fig, tol)
        assert all(f <= t for f, t in zip(fig, tol)), (fig, tol)


def test_mstep_component_without_responsibility():
    from pygda_amd import ops
    x, resp = soft_case(257, 33, 7, 1)[:2]
    resp = resp.copy()
    resp[0, :, 3] = 0.0
    w, mu, cov = ops.gmm_mstep(panel(x), T(resp), REG)
    nk, m64, c64 = skm._estimate_gaussian_parameters(x, resp[0], REG, "full")
    assert bool(torch.isfinite(cov).all()) and bool(torch.isfinite(mu).all())
    # nk = 10 eps: the mean is 0 / (10 eps) = 0, the covariance reg_covar on the diagonal -- sklearn's result
    assert torch.equal(mu[0, 3], torch.zeros(33, device=DEV)) and np.allclose(m64[3], 0)
    assert np.abs(N64(cov[0, 3]) - c64[3]).max() <= 1e-6 and abs(float(w[0, 3]) - nk[3] / nk.sum()) <= 1e-6


# ------------------------------------------------------------------------------------------------------ factor --
@pytest.mark.parametrize("shape", GRID)
def test_factor_against_float64(shape):
    from pygda_amd import ops
    N, d, K, R = shape
    cov = soft_case(*shape)[4]
    cov32 = cov.astype(np.float32)
    state = ops.gmm_state(R, DEV)
    prec, logdet = ops.gmm_factor(T(cov32), state)
    flags = ops.gmm_state_fields(state)[1].cpu()
    assert int(flags[:, 2].sum()) == 0
    for r in range(R):
        for k in range(K):
            L = np.linalg.cholesky(cov32[r, k].astype(np.float64))            # of the fp32 input, exactly
            want = solve_triangular(L, np.eye(d), lower=True).T
            y32 = skm._compute_precision_cholesky(cov32[r, k][None], "full")[0]
            fig = np.abs(N64(prec[r, k]) - want).max()
            tol = floor4(np.abs(y32 - want).max())
            ld = abs(float(logdet[r, k]) - np.log(np.diag(want)).sum())
            ld_tol = floor4(abs(float(np.log(np.diag(y32)).sum(dtype=np.float32)) - np.log(np.diag(want)).sum()))
            assert fig <= tol and ld <= max(ld_tol, 4 * 2.0 ** -24 * max(1.0, abs(np.log(np.diag(want)).sum()))), \
                (shape, r, k, fig, tol, ld, ld_tol)
            assert bool((prec[r, k].tril(-1) == 0).all())


def test_factor_flags_an_indefinite_covariance_and_returns():
    """A status path: the flag is set, the call returns normally, the other runs are factored."""
    from pygda_amd import ops
    cov = soft_case(64, 32, 7, 5)[4].astype(np.float32).copy()
    cov[2, 4] = -cov[2, 4]                                                      # run 2, component 4: negative definite
    cov[3, 0, 5, 5] = float("nan")                                              # run 3: a pivot that is not finite
    state = ops.gmm_state(5, DEV)
    prec = torch.full((5, 7, 32, 32), 7.0, device=DEV)
    logdet = torch.full((5, 7), 7.0, dtype=torch.float64, device=DEV)
    ops.gmm_factor(T(cov), state, out=(prec, logdet))
    torch.cuda.synchronize()
    flags = ops.gmm_state_fields(state)[1].cpu()
    assert flags[:, 2].tolist() == [0, 0, 1, 1, 0]
    assert bool((prec[2, 4] == 7.0).all()) and float(logdet[2, 4]) == 7.0       # nothing stored for that component
    want = solve_triangular(np.linalg.cholesky(cov[0, 1].astype(np.float64)), np.eye(32), lower=True).T
    assert np.abs(N64(prec[0, 1]) - want).max() < 1e-4
    # the failed run is now frozen: an M-step leaves its arrays alone
    x, resp = soft_case(64, 32, 7, 5)[:2]
    out = (torch.full((5, 7), 3.0, device=DEV), torch.full((5, 7, 32), 3.0, device=DEV),
           torch.full((5, 7, 32, 32), 3.0, device=DEV))
    ops.gmm_mstep(panel(x), T(resp), REG, state, out=out)
    assert bool((out[1][2] == 3.0).all()) and bool((out[2][3] == 3.0).all()) and not bool((out[1][0] == 3.0).any())


# ------------------------------------------------------------------------------------------------------ E-step --
@pytest.mark.parametrize("shape", GRID)
def test_estep_against_float64(shape):
    from pygda_amd import ops
    N, d, K, R = shape
    x, _, weights, means, cov = soft_case(*shape)
    x32 = x.astype(np.float32)
    prec = np.stack([np.stack([solve_triangular(np.linalg.cholesky(cov[r, k]), np.eye(d), lower=True).T
                               for k in range(K)]) for r in range(R)])
    logdet = np.log(np.diagonal(prec, axis1=2, axis2=3)).sum(-1)
    state = ops.gmm_state(R, DEV)
    resp = ops.gmm_estep(panel(x), T(weights), T(means), T(prec), torch.as_tensor(logdet, device=DEV), TOL, state)
    bounds, flags = (t.cpu() for t in ops.gmm_state_fields(state))
    assert flags[:, 0].tolist() == [1] * R and flags[:, 1].tolist() == [0] * R and bool(torch.isinf(bounds[:, 1]).all())
    for r in range(R):
        a, b = estimator(weights[r], means[r], cov[r], np.float64), estimator(weights[r], means[r], cov[r], np.float32)
        # rows sum to 1 within rounding: the entries are float32 roundings of float64 values that sum to 1 (2^-25 in all), and
        # the float32 sum taken here adds at most (K - 1) 2^-24.  Four times that.
        assert float((resp[r].sum(1) - 1).abs().max()) <= 4 * K * 2.0 ** -24
        fig = (np.abs(N64(resp[r]) - a.predict_proba(x)).max(), abs(float(bounds[r, 0]) - a.score(x)))
        tol = (floor4(np.abs(b.predict_proba(x32) - a.predict_proba(x)).max()), floor4(abs(b.score(x32) - a.score(x))))
        print(shape, r, "probabilities/lower bound", fig, tol)
        assert fig[0] <= tol[0] and fig[1] <= tol[1], (fig, tol)


def test_estep_row_far_from_every_component():
    from pygda_amd import ops
    x, _, weights, means, cov = soft_case(65, 33, 2, 1)
    x = x.copy()
    x[7] = 3000.0                                                               # every log-probability underflows exp
    prec = np.stack([solve_triangular(np.linalg.cholesky(cov[0, k]), np.eye(33), lower=True).T for k in range(2)])[None]
    logdet = np.log(np.diagonal(prec, axis1=2, axis2=3)).sum(-1)
    resp = ops.gmm_estep(panel(x), T(weights), T(means), T(prec), torch.as_tensor(logdet, device=DEV))
    assert bool(torch.isfinite(resp).all()) and abs(float(resp[0, 7].sum()) - 1) < 1e-6
    want = estimator(weights[0], means[0], cov[0], np.float64).predict_proba(x)
    assert int(resp[0, 7].argmax()) == int(want[7].argmax())


# ----------------------------------------------------------------------------------------------------- full EM --
@functools.lru_cache(maxsize=None)
def device_fit(case, check_every=8):
    from pygda.nn import GMMClustering
    x, _, r0 = case_input(case)
    c = GMMClustering(case[2], DEV, check_every=check_every)
    xp = panel(x)
    return c.fit_em(xp, T(r0)), xp


@pytest.mark.parametrize("case", list(CASES))
def test_em_against_sklearn_float64(case):
    model, xp = device_fit(case)
    check_fit_against_sklearn(case, model, model.predict_proba(xp))
    ref = sklearn_fit(case, "float64")
    assert np.abs(N64(model.weights_) - ref.weights_).max() <= 1e-6


def bits(model):
    return [getattr(model, k) for k in ("weights_", "means_", "covariances_", "precisions_cholesky_")]


def same_bits(a, b):
    return (all(torch.equal(p, q) for p, q in zip(bits(a), bits(b))) and a.lower_bound_ == b.lower_bound_
            and a.n_iter_ == b.n_iter_ and a.converged_ == b.converged_)


def test_em_does_not_depend_on_check_every_and_repeats_bit_for_bit():
    case = (640, 64, 5)
    base = device_fit(case)[0]
    for every in (1, 7, 100):
        assert same_bits(device_fit(case, every)[0], base), every
    device_fit.cache_clear()
    assert same_bits(device_fit(case)[0], base)                                # two identical calls


def test_runs_of_a_batch_equal_the_runs_alone():
    """Five starts that converge at different iterations: each run of the batch is bit-identical to that run alone."""
    from pygda.nn import GMMClustering
    from pygda_amd import ops
    case = (257, 3, 2)
    x, lab, _ = case_input(case)
    rng = np.random.RandomState(4)
    starts = []
    for noise in (0.0, 0.2, 0.4, 0.6, 0.8):
        noisy = lab.copy()
        m = rng.rand(len(lab)) < noise
        noisy[m] = rng.randint(0, 2, m.sum())
        starts.append(np.eye(2)[noisy])
    xp = panel(x)
    c = GMMClustering(2, DEV)

    def run(resp0):                                                            # the loop of _fit_device, every run kept
        state = ops.gmm_state(resp0.size(0), DEV)
        resp = resp0.clone()
        par = ops.gmm_mstep(xp, resp, REG, state)
        fac = ops.gmm_factor(par[2], state)
        for _ in range(40):
            ops.gmm_estep(xp, par[0], par[1], fac[0], fac[1], TOL, state, out=resp)
            ops.gmm_mstep(xp, resp, REG, state, out=par)
            ops.gmm_factor(par[2], state, out=fac)
        return par, fac, state

    par, fac, state = run(T(np.stack(starts)))
    iters = ops.gmm_state_fields(state)[1][:, 0].tolist()
    assert len(set(iters)) > 1 and max(iters) < 40, iters                       # they stop at different iterations
    for r, s in enumerate(starts):
        p1, f1, s1 = run(T(s[None]))
        assert torch.equal(state[r], s1[0]), r
        for a, b in zip(par + fac, p1 + f1):
            assert torch.equal(a[r], b[0]), r
    best = c.fit_em(xp, T(np.stack(starts)))
    k = int(np.argmax(ops.gmm_state_fields(state)[0][:, 0].cpu().numpy()))
    assert torch.equal(best.means_, par[1][k]) and best.n_iter_ == iters[k]


def test_non_positive_pivot_raises_on_the_device():
    from pygda.nn import GMMClustering
    x = torch.tensor([[1.0, 2.0], [1.0, 2.0], [0.0, 0.5], [3.0, -1.0], [2.0, 2.0], [-1.0, 0.0]], device=DEV)
    r0 = torch.zeros(6, 2, device=DEV)
    r0[:2, 0] = 1
    r0[2:, 1] = 1
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        GMMClustering(2, DEV, reg_covar=0.0).fit_em(x, r0)


def test_limits_raise_before_device_work():
    from pygda.nn import GMMClustering
    from pygda_amd import _lib
    with pytest.raises(_lib.GdaError, match="128 columns"):
        GMMClustering(2, DEV).fit_em(torch.zeros(10, 129, device=DEV), torch.full((10, 2), 0.5, device=DEV))


# ------------------------------------------------------------------------------------------------- kmeans_step --
@pytest.mark.parametrize("shape", [(1, 1, 1), (65, 3, 2), (257, 33, 7), (1000, 128, 32)])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_kmeans_step_against_float64(shape, metric):
    from pygda_amd import ops
    N, d, K = shape
    rng = np.random.RandomState(N + d + K)
    x = (rng.normal(size=(N, d)) + 3.0).astype(np.float32)                      # a common direction: see the last centre
    cen = (rng.normal(size=(K, d)) + 3.0).astype(np.float32)
    if K > 2:
        cen[K - 1] = -40 * np.abs(cen[K - 1]) - 40                              # far away AND opposite: nobody picks it
    if N > 1 and K > 1:
        cen[1] = cen[0]                                                         # a designed exact tie on every row
    labels, dist, sums, counts = ops.kmeans_step(panel(x), T(cen), metric)
    x64, c64 = x.astype(np.float64), cen.astype(np.float64)
    if metric == 1:
        want = ((x64[:, None] - c64[None]) ** 2).sum(2)
        tol = 4 * d * 2.0 ** -24 * want                                         # d positive terms added in order
    else:
        xn = x64 / np.maximum(np.linalg.norm(x64, axis=1), 1e-12)[:, None]
        cn = c64 / np.maximum(np.linalg.norm(c64, axis=1), 1e-12)[:, None]
        want = 0.5 * (1 - xn @ cn.T) if metric == 0 else np.sqrt(((xn[:, None] - cn[None]) ** 2).sum(2))
        # unit rows: d products whose magnitudes sum to at most 1 (a distance of at most 2), plus the two normalisations
        tol = np.full_like(want, 4 * (d + 4) * 2.0 ** -24 * (1.0 if metric == 0 else 2.0))
    assert (np.abs(N64(dist) - want) <= tol).all(), np.abs(N64(dist) - want).max()
    got = labels.cpu().numpy()
    if K > 1 and N > 1:
        assert not (got == 1).any()                                             # the tie goes to the lower index
    if K > 2:
        assert not (got == K - 1).any() and float(counts[K - 1]) == 0 and bool((sums[K - 1] == 0).all())
        tie_free = want.copy()
        tie_free[:, 1] = np.inf                                                 # column 1 never wins: it repeats column 0
        order = np.argsort(tie_free, axis=1)
        rows = np.arange(N)
        first, second = order[:, 0], order[:, 1]                                # rows whose float64 winner is not a near tie
        clear = tie_free[rows, second] - tie_free[rows, first] > tol[rows, first] + tol[rows, second]
        assert clear.mean() > 0.9 and np.array_equal(got[clear], first[clear])
    else:
        assert not got.any()
    hot = np.eye(K)[got]
    assert np.array_equal(N64(counts), hot.sum(0))
    assert np.abs(N64(sums) - hot.T @ x64).max() <= 4 * 2.0 ** -24 * np.abs(x64).sum(0).max()


# --------------------------------------------------------------------------------- forward and feature_clustering --
@pytest.mark.parametrize("smooth", [False, True])
def test_forward_on_the_device_against_the_cpu_path(smooth):
    import pygda.nn.gmm_clustering as M
    cen, lab, x = separated(n=257)
    n, K = len(x), len(cen)
    rng = np.random.RandomState(8)
    resp0 = np.stack([np.eye(K)[np.where(rng.rand(n) < 0.3, rng.randint(0, K, n), lab)] for _ in range(2)])
    ei, v = quirky_graph(n)
    src = torch.tensor(cen[[2, 0, 3, 1]], dtype=torch.float32)
    emb = torch.tensor(x, dtype=torch.float32)
    y = torch.tensor(lab)
    cpu = M.GMMClustering(K, "cpu").forward(src, emb, y, ei, v, smooth, 0.6, resp0=torch.tensor(resp0, dtype=torch.float32))
    g = M.GMMClustering(K, DEV)
    dev = g.forward(src.to(DEV), emb.to(DEV), y.to(DEV), ei.to(DEV), v.to(DEV), smooth, 0.6, resp0=T(resp0))
    assert dev["label"].is_cuda and dev["dist2center"].is_cuda and dev["dist2center"].dtype == torch.float32
    assert torch.equal(dev["label"].cpu(), cpu["label"])
    # Both are float32 runs of the same loop, each within the rule's bound of float64.  On separated data the
    # probabilities are saturated, the float32-against-float64 yardstick is 0 and the floor of 1e-6 applies to each; the
    # 20 smoothing steps are convex combinations of entries below 1 and add at most 20 * 2^-23 of rounding on each side.
    bound = 2 * (1e-6 + (20 * 2.0 ** -23 if smooth else 0.0))
    figure = float((dev["dist2center"].cpu() - cpu["dist2center"]).abs().max())
    print("forward, smooth", smooth, figure, bound)
    assert figure <= bound
    assert g.gmm.n_iter_ >= 1 and torch.equal(dev["label"], g.smooth_labels if smooth else g.labels)


@pytest.mark.parametrize("dist_type", ["cos", "euc"])
@pytest.mark.parametrize("empty", [False, True])
def test_feature_clustering_on_the_device_against_the_cpu_path(dist_type, empty):
    import pygda.nn.gmm_clustering as M
    feat, init = clustering_inputs(empty)
    eps = 1e-6 if dist_type == "cos" else 1e-3
    gt = torch.zeros(len(feat), dtype=torch.int64)
    cpu = M.Clustering(eps, "cpu", dist_type=dist_type)
    cpu.set_init_centers(init)
    cpu.feature_clustering(feat, gt)
    dev = M.Clustering(eps, DEV, dist_type=dist_type)
    dev.set_init_centers(init.to(DEV))
    dev.feature_clustering(feat.to(DEV), gt.to(DEV))
    assert torch.equal(dev.samples["label"].cpu(), cpu.samples["label"])
    assert torch.allclose(dev.samples["dist2center"].cpu(), cpu.samples["dist2center"], atol=2e-6)
    assert torch.allclose(dev.centers.cpu(), cpu.centers, atol=1e-4)
    assert abs(float(dev.center_change) - float(cpu.center_change)) <= 2e-6
