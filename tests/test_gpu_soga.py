"""SOGA on the MI355X: the kernels of csrc/gda_soga.hip against float64 -- the label-smoothed cross-entropy with its
gradient and hit count, the adaptation term with its four parts and ``dlogits`` on random tables and on tables built
for the hard cases (a hub that is a negative of every row, an unreferenced node, repeated negatives, positive ==
centre, a node that is the centre of several rows) -- each held against torch-float32's own distance to float64 on the
same inputs; two runs bit-identical; the 3 + 3-epoch fits against the fixtures recorded from the reference's own
soga.py with the host test's check; eager and captured fits bit-identical; one pretraining and one adaptation epoch at
the ACMv9 -> DBLPv7 stand-in shapes; no BLAS product on the path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import ops
from tests.test_gpu_acdne import _close
from tests.test_soga_host import FIXTURES, check_fit_against_fixture, fixture, run_fit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAMS = (0.7, 1.3)


def close(gpu, f32, f64, name, slack=2e-6):
    """``_close`` of tests/test_gpu_acdne.py, the figures printed first."""
    a, b, c = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64) for v in (gpu, f32, f64))
    print(f"{name}: |gpu - f64| = {np.abs(a - c).max():.3e}, |fp32 torch - f64| = {np.abs(b - c).max():.3e}")
    _close(gpu, f32, f64, name, slack)


@pytest.mark.parametrize("n", [1, 63, 1001])
@pytest.mark.parametrize("c", [2, 3, 7, 33, 64])
def test_smooth_ce_against_float64(n, c):
    g = torch.Generator().manual_seed(n * 100 + c)
    z = 2.0 * torch.randn(n, c, generator=g, dtype=torch.float64)
    z[torch.arange(n), z.argmax(1)] += 0.01                         # the arg-max is not a float32 near-tie
    y = torch.randint(0, c, (n,), generator=g)
    y[: n // 2] = z.argmax(1)[: n // 2]                             # half of the rows are hits

    def host(dtype):
        x = z.to(dtype).requires_grad_(True)
        loss = ops.soga_smooth_ce(x, y, 0.1)
        return loss.detach(), torch.autograd.grad(loss, x)[0]

    (l64, g64), (l32, g32) = host(torch.float64), host(torch.float32)
    zd, yd = z.float().to(DEV).requires_grad_(True), y.to(DEV)
    loss = ops.soga_smooth_ce(zd, yd, 0.1)
    stats = ops.ce_stats_for(zd, yd)
    (gd,) = torch.autograd.grad(loss, zd)
    close(loss, l32, l64, "loss")
    close(gd, g32, g64, "dlogits")
    assert stats is not None and abs(stats[0].item() - loss.item()) <= 1e-6 * max(abs(loss.item()), 1)
    assert int(stats[1].item()) == int((z.argmax(1) == y).sum())
    loss2 = ops.soga_smooth_ce(zd, yd, 0.1)
    assert torch.equal(loss, loss2) and torch.equal(gd, torch.autograd.grad(loss2, zd)[0])


def _random_tables(n, m, k, v, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, n, (m, 1), generator=g), torch.randint(0, n, (m, 1), generator=g),
             torch.randint(0, n, (m, k), generator=g)) for _ in range(v)]


def _hard_tables(n, m, k, v, seed):
    """Node 0 a negative of EVERY row of every view (a reverse list of v * m entries: several segments); node 1 in no
    role; a repeated negative in every row with k >= 3; positive == centre in every third row; node 2 the centre of
    every fifth row."""
    tables = _random_tables(n, m, k, v, seed)
    spare = min(3, n - 1)
    for cen, pos, neg in tables:
        for t in (cen, pos, neg):
            t[t == 1] = spare
        neg[:, 0] = 0
        if k >= 3:
            neg[:, 2] = neg[:, 1]
        if n > 2:
            cen[::5] = 2
        pos[::3] = cen[::3]
    return tables


def _check_adapt(n, c, tables, seed, segment=None):
    g = torch.Generator().manual_seed(seed)
    z = 2.0 * torch.randn(n, c, generator=g, dtype=torch.float64)
    lams = LAMS

    def host(dtype):
        x = z.to(dtype).requires_grad_(True)
        loss, parts = ops.soga_adapt(x, ops.soga_plan(tables, n), *lams)
        return loss.detach(), parts, torch.autograd.grad(loss, x)[0]

    (l64, p64, g64), (l32, p32, g32) = host(torch.float64), host(torch.float32)
    plan = ops.soga_plan(tables, n, DEV, segment=segment)
    zd = z.float().to(DEV).requires_grad_(True)
    loss, parts = ops.soga_adapt(zd, plan, *lams)
    (gd,) = torch.autograd.grad(loss, zd)
    assert torch.isfinite(parts).all() and torch.isfinite(gd).all() and loss.item() == parts[0].item()
    close(loss, l32, l64, "loss")
    close(parts, p32, p64, "parts")
    close(gd, g32, g64, "dlogits")
    loss2, parts2 = ops.soga_adapt(zd, plan, *lams)
    assert torch.equal(parts, parts2) and torch.equal(gd, torch.autograd.grad(loss2, zd)[0])
    return plan, gd


SHAPES = [(1, 2, 1), (63, 3, 5), (260, 7, 5), (1001, 33, 8), (4099, 64, 5)]


@pytest.mark.parametrize("v", [1, 2])
@pytest.mark.parametrize("n,c,k", SHAPES)
def test_adapt_against_float64_on_random_tables(n, c, k, v):
    _check_adapt(n, c, _random_tables(n, n, k, v, n + v), 7 * n + c)


@pytest.mark.parametrize("v", [1, 2])
@pytest.mark.parametrize("n,c,k", SHAPES[1:])
def test_adapt_against_float64_on_the_hard_cases(n, c, k, v):
    tables = _hard_tables(n, n, k, v, n + 10 * v)
    plan, gd = _check_adapt(n, c, tables, 3 * n + c)
    node_seg = plan.node_seg.cpu().numpy()
    assert node_seg[1] - node_seg[0] >= max(v * n // plan.segment, 1)          # the hub crosses the segment length
    if n >= 260:
        assert node_seg[1] - node_seg[0] >= 4
    assert node_seg[2] == node_seg[1]                                         # node 1 is referenced by nothing
    # the segment length changes the order of the hub's sum, never what is summed
    _, gd16 = _check_adapt(n, c, tables, 3 * n + c, segment=16)
    assert float((gd16 - gd).abs().max()) <= 1e-5 * float(gd.abs().max())


def test_adapt_checks_its_arguments():
    from pygda_amd import _lib
    plan = ops.soga_plan(_random_tables(50, 50, 3, 2, 1), 50, DEV)
    with pytest.raises(_lib.GdaError, match="64 classes"):
        ops.soga_adapt(torch.zeros(50, 65, device=DEV), plan)
    with pytest.raises(_lib.GdaError, match="64 classes"):
        ops.soga_smooth_ce(torch.zeros(50, 65, device=DEV), torch.zeros(50, dtype=torch.int64, device=DEV))
    with pytest.raises(_lib.GdaError, match="plan lives on"):
        ops.soga_adapt(torch.zeros(50, 3), plan)
    plan.nrev -= 2 * 50                                                       # as if built for K - 1
    with pytest.raises(_lib.GdaError, match="gda_soga_adapt_f32"):
        ops.soga_adapt(torch.zeros(50, 3, device=DEV), plan)


@pytest.mark.parametrize("name", FIXTURES)
def test_fit3_against_the_reference_bounded_by_its_float64_run(name):
    f, s, t = fixture(name)
    _, got = run_fit(f, s, t, DEV)
    check_fit_against_fixture(got, f)


def test_eager_and_captured_fits_are_bit_identical():
    f, s, t = fixture("soga_fit3_gin.npz")

    def run(graph):
        _, got = run_fit(f, s, t, DEV, epochs=7, use_hip_graph=graph, epochs_per_graph=3)
        return got

    eager, captured, again = run(False), run(True), run(True)
    assert len(eager["src_losses"]) == 7 and len(eager["tgt_losses"]) == 7
    for k in eager:
        if k != "tables":
            assert np.array_equal(eager[k], captured[k]), k
            assert np.array_equal(captured[k], again[k]), k


@pytest.mark.parametrize("gnn", ["gcn", "gat"])
def test_one_epoch_of_each_phase_at_the_acm_dblp_shapes(gnn):
    from bench import make_cfg_a
    src, tgt = make_cfg_a()
    m = pygda_amd.models.SOGA(src.x.size(1), 128, 5, gnn=gnn, device=DEV, epoch=1, verbose=0, record=True)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    import random
    random.seed(0)
    np.random.seed(0)
    m.fit(src, tgt)
    logits, _ = m.predict(tgt)
    assert len(log) == 2 and all(np.isfinite(v) for v in log) and np.isfinite(m.parts_log).all()
    assert logits.shape == (5484, 5) and torch.isfinite(logits).all()


def test_no_blas_product_on_the_soga_path(monkeypatch):
    f, s, t = fixture("soga_fit3_gcn.npz")
    calls = []

    def spy(name, fn):
        def wrapped(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapped

    for owner, attr in ((torch, "mm"), (torch, "matmul"), (torch.Tensor, "mm"), (torch.Tensor, "__matmul__"),
                        (F, "linear")):
        monkeypatch.setattr(owner, attr, spy(attr, getattr(owner, attr)))
    m, _ = run_fit(f, s, t, DEV, epochs=5)
    m.predict(t)
    torch.cuda.synchronize()
    assert calls == [], sorted(set(calls))
