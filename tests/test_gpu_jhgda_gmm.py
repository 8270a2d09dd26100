"""GPU: JHGDA's mixture pseudo-labels (``pseudo='gmm'``).  The assignment solver against scipy, the cosine cost against
``DIST('cos')`` in float64, the per-label sums and the relabel kernel against float64, and the trainer on the planted
pair of tests/test_jhgda_gmm_host.py against the CPU float64 fit: equal iteration counts, flags and pseudo-labels, the
rest bounded by four times the CPU float32 fit's own deviation from float64; the freeze rule, determinism, the fallback,
no library product and no host read on the path, and the untouched ``pseudo='classifier'`` fit against the record of the
commit before this option existed (tests/golden/jhgda_planted_classifier.json)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

import pygda_amd
from pygda_amd import ops
from pygda_amd.nn.gmm_clustering import DIST
from tests.test_jhgda_gmm_host import C, GMM, HID, IN_DIM, KW, cpu_fit, fit, labels_of, planted_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.join(os.path.dirname(__file__), "golden")


def state():
    return ops.gmm_state(1, DEV)


def failed(st):
    return int(ops.gmm_state_fields(st)[1][0, 2])


def is_perm(c2l, shuf, K):
    return sorted(c2l.tolist()) == list(range(K)) and all(c2l[shuf[j]] == j for j in range(K))


# ---------------------------------------------------------------------------------------------- the solver alone --
def second_best_gap(cost):
    """The optimum's lead over the best assignment that avoids one of its pairs (inf for a single pair)."""
    row, col = linear_sum_assignment(cost)
    best, gap = cost[row, col].sum(), np.inf
    big = np.abs(cost).sum() + 1.0
    for i, j in zip(row, col):
        if len(row) == 1:
            break
        c = cost.copy()
        c[i, j] = big
        r2, c2 = linear_sum_assignment(c)
        gap = min(gap, c[r2, c2].sum() - best)
    return gap


@pytest.mark.parametrize("K", [1, 2, 3, 5, 31, 32])
def test_solver_equals_scipy_on_costs_with_a_unique_optimum(K):
    cost = np.random.RandomState(100 + K).uniform(size=(K, K))
    assert second_best_gap(cost) > 1e-6                                  # a condition on the seed, checked on the CPU
    _, col = linear_sum_assignment(cost)
    st = state()
    c2l, shuf = ops.lsa_cost(torch.tensor(cost, device=DEV), st)
    c2l, shuf = c2l.cpu().numpy(), shuf.cpu().numpy()
    assert np.array_equal(c2l, col) and np.array_equal(shuf, np.argsort(col)) and failed(st) == 0
    assert cost[np.arange(K), c2l].sum() == cost[np.arange(K), col].sum()


@pytest.mark.parametrize("name", ["integers", "all_equal"])
def test_solver_on_ties_gives_a_permutation_with_scipys_objective(name):
    K = 9
    cost = (np.random.RandomState(4).randint(0, 4, size=(K, K)).astype(np.float64) if name == "integers"
            else np.full((K, K), 0.25))
    row, col = linear_sum_assignment(cost)
    c2l, shuf = (v.cpu().numpy() for v in ops.lsa_cost(torch.tensor(cost, device=DEV), state()))
    assert is_perm(c2l, shuf, K)
    assert cost[np.arange(K), c2l].sum() == cost[row, col].sum()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_solver_non_finite_cost_gives_the_identity_and_failed(bad):
    cost = np.random.RandomState(5).uniform(size=(6, 6))
    cost[2, 3] = bad
    st = state()
    c2l, shuf = ops.lsa_cost(torch.tensor(cost, device=DEV), st)
    torch.cuda.synchronize()
    assert c2l.tolist() == list(range(6)) and shuf.tolist() == list(range(6)) and failed(st) == 1
    c2l, shuf = ops.lsa_cost(torch.tensor(cost, device=DEV))            # no state: the identity all the same
    assert c2l.tolist() == list(range(6))


@pytest.mark.parametrize("K,d", [(1, 1), (2, 3), (7, 33), (32, 128)])
def test_lsa_cos_against_dist_cos_float64_and_scipy(K, d):
    rng = np.random.RandomState(K * 7 + d)
    tgt = rng.normal(size=(K, d)).astype(np.float32) * rng.uniform(0.1, 30, size=(K, 1)).astype(np.float32)
    src = rng.normal(size=(K, d)).astype(np.float32) * rng.uniform(0.1, 30, size=(K, 1)).astype(np.float32)
    tgt[K // 2] = 0                                                      # an empty cluster: cost 0.5 to every centre
    cost = DIST("cos").get_dist(torch.tensor(tgt).double(), torch.tensor(src).double(), cross=True).numpy()
    assert np.allclose(cost[K // 2], 0.5, atol=0, rtol=0)
    assert second_best_gap(cost) > 1e-6
    _, col = linear_sum_assignment(cost)
    st = state()
    c2l, shuf = ops.lsa_cos(torch.tensor(tgt, device=DEV), torch.tensor(src, device=DEV), st)
    assert np.array_equal(c2l.cpu().numpy(), col) and np.array_equal(shuf.cpu().numpy(), np.argsort(col))
    assert failed(st) == 0
    src[0, 0] = np.inf                                                   # a non-finite centre: identity, failed, no error
    c2l, _ = ops.lsa_cos(torch.tensor(tgt, device=DEV), torch.tensor(src, device=DEV), st)
    assert c2l.tolist() == list(range(K)) and failed(st) == 1


# ------------------------------------------------------------------------------ per-label sums and the relabelling --
SHAPES = [(1, 1, 1), (63, 2, 33), (64, 7, 128), (65, 32, 1), (1000, 7, 33), (1000, 32, 128), (1000, 2, 1)]


@pytest.mark.parametrize("N,K,d", SHAPES)
def test_label_sums_against_float64(N, K, d):
    rng = np.random.RandomState(N + 31 * K + d)
    x = rng.normal(size=(N, d)).astype(np.float32) * 3 + 1
    lab = rng.randint(0, max(K - 2, 1), size=N)                          # the last classes stay empty (K > 2)
    block = torch.full((N, d + 3), float("nan"), device=DEV)             # a panel: the padding is never read
    block[:, :d] = torch.tensor(x)
    labels = torch.tensor(lab, device=DEV)
    sums, counts = ops.gmm_label_sums(block[:, :d], labels, K)
    again = ops.gmm_label_sums(block[:, :d], labels, K)
    assert torch.equal(sums, again[0]) and torch.equal(counts, again[1])
    hot = np.eye(K)[lab]
    ref = hot.T @ x.astype(np.float64)
    yard = np.abs(torch.zeros(K, d).index_add_(0, torch.tensor(lab), torch.tensor(x)).double().numpy() - ref).max()
    err = np.abs(sums.double().cpu().numpy() - ref).max()
    print(N, K, d, "sums", err, "float32 yardstick", yard)
    assert err <= max(4 * yard, 1e-6)
    assert np.array_equal(counts.cpu().numpy(), hot.sum(0))
    if K > 2:
        assert float(sums[K - 1].abs().max()) == 0 and float(counts[K - 1]) == 0


@pytest.mark.parametrize("N,K,d", SHAPES)
def test_relabel_exact(N, K, d):
    rng = np.random.RandomState(N + K)
    resp = rng.dirichlet(np.ones(K), size=N).astype(np.float32)
    if N > 3 and K > 1:
        resp[1, :] = resp[1, 0]                                          # a full tie: the lowest index
        resp[2, K - 1] = resp[2].max()                                   # a two-way tie
    perm = rng.permutation(K)
    c2l = torch.tensor(perm, dtype=torch.int32, device=DEV)
    shuf = torch.tensor(np.argsort(perm), dtype=torch.int32, device=DEV)
    fb = torch.tensor(rng.randint(0, K, size=N), device=DEV)
    r = torch.tensor(resp, device=DEV)
    arg = resp.argmax(1)                                                 # numpy: the first of equal maxima
    for st, fail, want in ((None, 0, perm[arg]), (state(), 0, perm[arg]), (state(), 1, fb.cpu().numpy())):
        if fail:
            ops.gmm_state_fields(st)[1][0, 2] = 1
        prob, labels, hot = ops.gmm_relabel(r, c2l, shuf, fb, st)
        assert np.array_equal(labels.cpu().numpy(), want)
        assert np.array_equal(hot.cpu().numpy(), np.eye(K, dtype=np.float32)[want])
        assert np.array_equal(prob.cpu().numpy(), resp[:, np.argsort(perm)])
    prob, labels, hot = ops.gmm_relabel(r)                               # the argmax of given probabilities alone
    assert prob is None and np.array_equal(labels.cpu().numpy(), arg)
    assert np.array_equal(hot.cpu().numpy(), np.eye(K, dtype=np.float32)[arg])
    again = ops.gmm_relabel(r, c2l, shuf, fb)
    assert all(torch.equal(a, b) for a, b in zip(again, ops.gmm_relabel(r, c2l, shuf, fb)))


# ----------------------------------------------------------------------------------------------------- the trainer --
def gpu_fit(**kw):
    return fit(DEV, torch.float32, **kw)


def final(m):
    dtype = m.jhgda.cls_model[0].weight.dtype
    s, t = (pygda_amd.data.Data(x=d.x.to(dtype), edge_index=d.edge_index, y=d.y) for d in planted_pair())
    sd = {k: v.detach().double().cpu().numpy() for k, v in m.jhgda.state_dict().items()}
    return sd, m.predict(s)[0].double().cpu().numpy(), m.predict(t)[0].double().cpu().numpy()


def deviation(a, b):
    """(loss without its label_matching term, parameters, logits): the largest absolute differences of two fits."""
    (ma, la), (mb, lb) = a, b
    loss = max(abs((x[0] - 0.1 * p) - (y[0] - 0.1 * q)) for x, p, y, q in zip(la, ma.lm_log, lb, mb.lm_log))
    (sa, *ga), (sb, *gb) = final(ma), final(mb)
    return (loss, max(np.abs(sa[k] - sb[k]).max() for k in sa), max(np.abs(x - y).max() for x, y in zip(ga, gb)))


@pytest.mark.parametrize("kw", [{}, dict(hid=33), dict(gmm_smooth_r=0.5)], ids=["hid8", "hid33", "smooth"])
def test_fit_against_the_cpu_float64_fit(kw):
    """Measured on the MI355X (loss, parameters, logits; device against float64, then the CPU float32 yardstick):
    see DESIGN 4.27."""
    kw = dict(GMM, **kw)
    m64, log64, seen64 = cpu_fit(torch.float64, **kw)
    m32, log32, _ = cpu_fit(torch.float32, **kw)
    m, log, seen = gpu_fit(use_hip_graph=False, **kw)
    print(kw, "gmm_log", m.gmm_log, "float64", m64.gmm_log)
    assert [e[:3] for e in m.gmm_log] == [e[:3] for e in m64.gmm_log]
    assert len(seen) == 3
    for a, b in zip(labels_of(seen), labels_of(seen64)):
        assert np.array_equal(a, b)
    for e, e32, e64 in zip(m.gmm_log, m32.gmm_log, m64.gmm_log):       # the lower bound: the same rule as below
        assert abs(e[3] - e64[3]) <= max(4 * abs(e32[3] - e64[3]), 1e-3 * max(1.0, abs(e64[3]))), (e, e32, e64)
    yard = deviation((m32, log32), (m64, log64))
    got = deviation((m, log), (m64, log64))
    print(kw, "device - float64", got, "float32 - float64", yard)
    # label_matching is an argmax count without a gradient (tests/test_jhgda_host.py::check_fit): one flipped row per
    # level and domain at the most
    assert max(abs(a - b) for a, b in zip(m.lm_log, m64.lm_log)) <= 1.0 + 1e-6
    for g, y, floor in zip(got, yard, (1e-4, 1e-4, 1e-3)):
        assert g <= max(4 * y, floor), (got, yard)


def same_fit(a, b):
    (ma, la), (mb, lb) = a, b
    return la == lb and ma.gmm_log == mb.gmm_log and ma.lm_log == mb.lm_log and all(
        torch.equal(x, y) for x, y in zip(ma.jhgda.state_dict().values(), mb.jhgda.state_dict().values()))


def test_freeze_rule_more_iterations_than_needed_change_no_bit():
    m, log, _ = gpu_fit(**GMM)
    most = max(e[0] for e in m.gmm_log)
    assert 2 <= most <= 90 and all(e[1] == 1 for e in m.gmm_log)
    m2, log2, _ = gpu_fit(gmm_max_iter=most + 2, **GMM)
    assert same_fit((m, log), (m2, log2))


def test_two_fits_and_eager_against_captured_bit_identical():
    runs = []
    for graph in (False, False, True):
        m, log, _ = gpu_fit(epochs=8, use_hip_graph=graph, epochs_per_graph=4, gmm_max_iter=30, **GMM)
        assert len(m.gmm_log) == 8 and all(e[2] == 0 for e in m.gmm_log)
        runs.append((m, log))
    assert same_fit(runs[0], runs[1]) and same_fit(runs[0], runs[2])


@pytest.mark.parametrize("graph", [False, True])
def test_singular_covariance_falls_back_to_the_classifier_fit_bit_for_bit(graph):
    """The duplicated target rows of the host test: ``k_factor`` meets a non-positive pivot, sets ``failed`` and every
    later kernel leaves the run alone -- a status, not a fault."""
    kw = dict(duplicated=True, epochs=4, use_hip_graph=graph, epochs_per_graph=4)
    mg, logg, _ = gpu_fit(pseudo="gmm", gmm_reg_covar=0.0, gmm_max_iter=10, **kw)
    mc, logc, _ = gpu_fit(**kw)
    assert [e[2] for e in mg.gmm_log] == [1] * 4 and mc.gmm_log == []
    assert logg == logc and mg.lm_log == mc.lm_log
    assert all(torch.equal(x, y) for x, y in zip(mg.jhgda.state_dict().values(), mc.jhgda.state_dict().values()))


def test_no_blas_product_and_no_host_read_on_the_gmm_path(monkeypatch):
    """A captured fit succeeds: a ``.cpu()`` or ``.item()`` inside an epoch would end the capture with an error."""
    calls = []

    def spy(name, fn):
        def wrapped(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapped

    for owner, attr in ((torch, "mm"), (torch, "matmul"), (torch.Tensor, "mm"), (torch.Tensor, "__matmul__"),
                        (F, "linear")):
        monkeypatch.setattr(owner, attr, spy(attr, getattr(owner, attr)))
    s, t = planted_pair()
    m = pygda_amd.models.JHGDA(IN_DIM, HID, C, device=DEV, epoch=4, use_hip_graph=True, epochs_per_graph=4,
                               gmm_smooth_r=0.5, gmm_max_iter=10, **KW, **GMM)
    torch.manual_seed(0)
    m.fit(s, t)
    m.predict(t)
    torch.cuda.synchronize()
    assert calls == [], sorted(set(calls))
    assert len(m.gmm_log) == 4


def test_classifier_fit_is_what_it_was_before_the_option_existed():
    """Losses, label_matching sums and the parameters' float64 sums of the planted pair's 3-epoch fit, recorded on
    the MI355X from the commit before ``pseudo`` was added."""
    rec = json.load(open(os.path.join(HERE, "jhgda_planted_classifier.json")))
    m, log, _ = gpu_fit()
    assert [float(l).hex() for l, _ in log] == rec["losses"]
    assert [float(v).hex() for v in m.lm_log] == rec["lm"]
    sums = {k: float(v.double().sum()).hex() for k, v in m.jhgda.state_dict().items()}
    assert sums == rec["param_sums"]
