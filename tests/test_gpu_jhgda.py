"""JHGDA on the MI355X: the proximity kernel (edge-list and dense branches) and the pooling-row kernel against float64
at widths that are not tile multiples, the fit against the reference's recorded float32 fit bounded by its float64
run, determinism (two fits, eager against captured), no BLAS product on the path, and the memory of a full-size epoch
and of the proximity op alone at the ACMv9 -> DBLPv7 stand-in shapes."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import ops
from pygda_amd.data import Data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.join(os.path.dirname(__file__), "golden")


def _assign(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(n, k, generator=g) * 4, dim=1).to(DEV)


def _edges(n, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, 3 * n), generator=g)
    ei = torch.cat([ei, ei[:, :5], torch.tensor([[0, 1], [0, 2]])], 1)       # duplicates, a self loop, directed edges
    return ei.to(DEV)


def _prox64(A, S):
    S = S.double().detach().requires_grad_(True)
    n = S.size(0)
    if A.shape[0] < A.shape[1]:
        a = torch.zeros(n, n, dtype=torch.float64, device=DEV).index_put_(
            (A[0], A[1]), torch.ones(A.size(1), dtype=torch.float64, device=DEV), accumulate=True)
        a.requires_grad_(False)
    else:
        a = A.double().detach().requires_grad_(True)
    p = torch.min(S @ S.T, torch.ones(1, dtype=torch.float64, device=DEV))
    loss = torch.sum(-a * torch.log(p + 1e-7) - (1 - a) * torch.log(1 - p + 1e-7)) / (n * n)
    grads = torch.autograd.grad(loss, [S] + ([a] if a.requires_grad else []))
    return loss.item(), grads


@pytest.mark.parametrize("n", [300, 1201, 9360])
@pytest.mark.parametrize("k", [60, 257, 1872])
def test_prox_edge_list_against_float64(n, k):
    S = _assign(n, k, n + k).requires_grad_(True)
    ei = _edges(n, n)
    loss = ops.jhgda_prox(ei, S)
    (dS,) = torch.autograd.grad(loss, S)
    ref, (ref_dS,) = _prox64(ei, S)
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref) + 1e-7
    err = (dS.double() - ref_dS).abs().max().item()
    assert err <= 1e-4 * ref_dS.abs().max().item() + 1e-9, err


@pytest.mark.parametrize("n,k", [(60, 12), (257, 52), (1872, 374)])
def test_prox_dense_against_float64(n, k):
    S = _assign(n, k, 3 * n).requires_grad_(True)
    A = torch.rand(n, n, generator=torch.Generator().manual_seed(n)).to(DEV) * 2        # not symmetric
    A.requires_grad_(True)
    loss = ops.jhgda_prox(A, S)
    dS, dA = torch.autograd.grad(2.5 * loss, (S, A))
    ref, (ref_dS, ref_dA) = _prox64(A, S)
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref) + 1e-7
    assert (dS.double() - 2.5 * ref_dS).abs().max().item() <= 1e-4 * 2.5 * ref_dS.abs().max().item()
    assert (dA.double() - 2.5 * ref_dA).abs().max().item() <= 1e-4 * 2.5 * ref_dA.abs().max().item()


def test_prox_one_hot_assignment_and_two_runs_bit_identical():
    idx = torch.randint(0, 13, (500,), generator=torch.Generator().manual_seed(1)).to(DEV)
    S = torch.eye(13, device=DEV)[idx]                               # P entries exactly 0 or 1 (min's tie)
    ei = _edges(500, 4)
    a = ops.jhgda_prox(ei, S)
    ref, _ = _prox64(ei, S)
    assert abs(a.item() - ref) <= 1e-5 * abs(ref)
    S2 = _assign(1201, 257, 9).requires_grad_(True)
    r1 = torch.autograd.grad(ops.jhgda_prox(ei[:, ei[0] < 500], S2[:500]), S2)[0]
    r2 = torch.autograd.grad(ops.jhgda_prox(ei[:, ei[0] < 500], S2[:500]), S2)[0]
    assert torch.equal(r1, r2)


@pytest.mark.parametrize("n,k", [(300, 60), (1201, 257), (9360, 1872), (7, 2)])
def test_pool_rows_against_float64(n, k):
    X = torch.randn(n, k, generator=torch.Generator().manual_seed(k)).to(DEV).requires_grad_(True)
    w = torch.randn(n, k, generator=torch.Generator().manual_seed(k + 1)).to(DEV)
    S, ce = ops.jhgda_pool_rows(X)
    gX = torch.autograd.grad((S * w).sum() + 0.7 * ce, X)[0]
    X64 = X.detach().double().requires_grad_(True)
    S64 = torch.softmax(torch.relu(X64), dim=1)
    ce64 = torch.mean(torch.sum(-S64 * torch.log(S64 + 1e-7), dim=1))
    g64 = torch.autograd.grad((S64 * w.double()).sum() + 0.7 * ce64, X64)[0]
    assert (S.double() - S64).abs().max().item() < 1e-6
    assert abs(ce.item() - ce64.item()) < 1e-5 * abs(ce64.item()) + 1e-7
    assert (gX.double() - g64).abs().max().item() < 1e-5 * g64.abs().max().item() + 1e-7


def _pair(name):
    f = np.load(os.path.join(HERE, name))
    s = Data(x=torch.from_numpy(f["src_x"]), edge_index=torch.from_numpy(f["src_ei"]), y=torch.from_numpy(f["src_y"]))
    t = Data(x=torch.from_numpy(f["tgt_x"]), edge_index=torch.from_numpy(f["tgt_ei"]), y=torch.from_numpy(f["tgt_y"]))
    return f, s, t


def _fit(name, extra, epochs=3, **kw):
    f, s, t = _pair(name)
    m = pygda_amd.models.JHGDA(16, 16, 3, num_layers=3, lr=4e-3, device=DEV, epoch=epochs, verbose=0, **extra, **kw)
    log = []
    m.epoch_hook = lambda e, loss, acc, secs: log.append((loss, acc))
    torch.manual_seed(int(f["init_seed"]))
    m.fit(s, t)
    return f, s, t, m, log


@pytest.mark.parametrize("name,extra", [("jhgda_fit3.npz", {}),
                                        ("jhgda_fit3_sparse_share.npz", dict(sparse=True, share=True))])
@pytest.mark.parametrize("graph", [False, True])
def test_fit3_against_the_reference_bounded_by_its_float64_run(name, extra, graph):
    from tests.test_jhgda_host import check_fit
    f, s, t, m, log = _fit(name, extra, use_hip_graph=graph, epochs_per_graph=3)
    check_fit(f, log, m.lm_log, m.jhgda.state_dict(), m.predict(s)[0].cpu().numpy(), m.predict(t)[0].cpu().numpy(),
              s.x.size(0), tol_loss=1e-4, tol_param=1e-4, tol_logit=1e-3)


def test_prox_loss_alone_when_s_takes_no_gradient():
    S = _assign(1201, 257, 3)
    ei = _edges(1201, 3)
    a = ops.jhgda_prox(ei, S)                                   # no gradient wanted: no strip, no GEMM
    b = ops.jhgda_prox(ei, S.clone().requires_grad_(True))
    assert torch.equal(a.detach(), b.detach())
    A = torch.rand(300, 300, generator=torch.Generator().manual_seed(2)).to(DEV)
    S2 = _assign(300, 60, 4)
    assert torch.equal(ops.jhgda_prox(A, S2).detach(), ops.jhgda_prox(A, S2.clone().requires_grad_(True)).detach())


def test_label_matching_count_without_the_nxk_matrix():
    from pygda_amd.nn import JHGDABase
    net = JHGDABase(16, 16, 3, device=DEV, pool_ratio=0.2, num_s=300, num_t=260).to(DEV)
    g = torch.Generator().manual_seed(6)
    lab = torch.randint(0, 3, (1201,), generator=g).to(DEV)
    Y = torch.eye(3, device=DEV)[lab]
    S = _assign(1201, 57, 8)
    Yp = torch.softmax(torch.randint(0, 2, (57, 3), generator=g).float(), 1).to(DEV)      # many exact ties
    want = 1 - (torch.argmax(Y.cpu() @ Yp.cpu().T, 1) == torch.argmax(S.cpu(), 1)).sum() / 1201.0
    assert net.label_matching(S, Y, Yp, one_hot=True).item() == pytest.approx(want.item(), abs=1e-7)
    assert net.label_matching(S, Y, Yp).item() == pytest.approx(want.item(), abs=1e-7)


def test_two_fits_and_eager_against_captured_bit_identical():
    runs = []
    for graph in (False, False, True):
        _, s, t, m, log = _fit("jhgda_fit3.npz", {}, epochs=8, use_hip_graph=graph)
        runs.append((log, [v.clone() for v in m.jhgda.state_dict().values()]))
    for log, sd in runs[1:]:
        assert log == runs[0][0]
        assert all(torch.equal(a, b) for a, b in zip(sd, runs[0][1]))


def test_no_blas_product_on_the_jhgda_path(monkeypatch):
    f, s, t = _pair("jhgda_fit3.npz")
    m = pygda_amd.models.JHGDA(16, 16, 3, device=DEV, epoch=2, verbose=0)
    calls = []

    def spy(name, fn):
        def wrapped(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapped

    for owner, attr in ((torch, "mm"), (torch, "matmul"), (torch.Tensor, "mm"), (torch.Tensor, "__matmul__"),
                        (F, "linear")):
        monkeypatch.setattr(owner, attr, spy(attr, getattr(owner, attr)))
    torch.manual_seed(0)
    m.fit(s, t)
    m.predict(t)
    torch.cuda.synchronize()
    assert calls == [], sorted(set(calls))


def _cfg(ns, es, nt, et, seed=7):
    from bench import make_cfg_a
    return make_cfg_a(seed=seed, ns=ns, es=es, nt=nt, et=et)


def test_one_full_size_epoch_at_acm_dblp_shapes():
    src, tgt = (Data(x=d.x.to(DEV), edge_index=d.edge_index.to(DEV), y=d.y.to(DEV))
                for d in _cfg(9360, 15556, 5484, 8117))
    m = pygda_amd.models.JHGDA(src.x.size(1), 128, int(src.y.max()) + 1, device=DEV, epoch=1, verbose=0)
    log, grow = [], []
    m.epoch_hook = lambda e, loss, acc, secs: log.append(loss)
    inner = m._device_fit

    def measured(s, t, graphs):
        # the epoch itself, model and inputs already built; every cached workspace is dropped first, so the GEMMs' and
        # the proximity kernel's scratch are counted with the activations, gradients and Adam state
        pygda_amd._lib._ws_cache.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        inner(s, t, graphs)
        torch.cuda.synchronize()
        grow.append(torch.cuda.max_memory_allocated() - base)

    m._device_fit = measured
    torch.manual_seed(0)
    m.fit(src, tgt)                                             # warm: workspaces, graphs, the allocator's pools
    m.fit(src, tgt)
    assert len(log) == 2 and all(np.isfinite(v) for v in log)
    assert grow[1] < 3 * 9360 * 9360 * 4, f"the epoch allocated {grow[1] / 2**20:.1f} MiB"


def test_prox_alone_at_full_size_grows_memory_below_4nk():
    n, k = 9360, 1872
    S = _assign(n, k, 0).requires_grad_(True)
    ei = _edges(n, 1)
    edges = ops.JhgdaEdges(ei, n)
    loss = ops.jhgda_prox(ei, S, edges)                         # warm: the workspace
    torch.autograd.grad(loss, S)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = ops.jhgda_prox(ei, S, edges)
    (dS,) = torch.autograd.grad(loss, S)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    assert torch.isfinite(loss) and torch.isfinite(dS).all()
    ws = pygda_amd._lib.lib().gda_jhgda_prox_workspace_bytes(n, k)
    assert grow + ws < 4 * n * k * 4, f"grew {grow / 2**20:.1f} MiB beside a {ws / 2**20:.1f} MiB workspace"
