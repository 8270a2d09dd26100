"""PairAlign on the MI355X: the kernels of csrc/gda_pairalign.hip against float64 -- the class-pair outer-product sums
over the edges, the class-segmented softmax sums, the class-coefficient cross-entropy each way (with a coefficient vector
changed in place under one captured graph) and the in-place refresh of the re-weighted CSR values --, and the fixture
fits on the device: against the reference's record, captured against eager, and twice from one seed.

Every comparison with float64 uses the rule of test_gpu_asn.py / test_gpu_dgda.py:
|gpu - f64| <= 8 |fp32 torch - f64| + slack max|f64|, the fp32 and float64 values from a plain torch composition of the
reference's lines on the same inputs.  For the fits the fp32 value is the reference's own record (pairalign_fit.npz) and
the float64 value the project's host path run in double, which tests/test_pairalign_host.py pins to that record first
(pa.py's ``.float()`` casts do not allow a float64 rerun of the reference itself).

Starting slacks: 2e-6 for the statistic kernels (float64 accumulation of fp32 inputs; test_gpu_dgda.py's figure for an
fp32-product-class result), 1e-6 / 1e-5 for the loss and its gradient (the bounds of test_softmax_nll_vs_torch), 1e-5 for
the fits' losses and 1e-4 for their parameters, predictions and weights (test_gpu_dgda.py's).  The refreshed CSR values
are held to 4e-7 relative: they and the rebuilt ones are the same product of three factors rounded in two orders, at most
six fp32 roundings apart (6 x 2^-24 = 3.6e-7).

Observed on the MI355X (largest |gpu - f64| / max|f64| of a group, and the largest share of its limit); no slack was
widened:
- edge statistics, 47 cases: 2.2e-15 (the fp32 torch composition is at 1e-7: the 8 x term alone is five orders above);
- softmax sums, 60 cases: 2.2e-7, 0.08 of the limit (the fp32 ``expf`` of the rows, then float64 sums);
- loss 3.4e-7 (0.03 of the limit), gradient 1.8e-6 (0.07), 10 cases each;
- GS fit: losses 2.9e-7 (0.03), ``ew`` 9.2e-7, ``lw`` 3.3e-7, ``edge_weight`` 9.0e-7 (0.01), both predicts 3.4e-6 (0.03),
  final parameters 3.8e-6 (0.04); GCN fit: losses 6.9e-8, predicts 6.6e-7, parameters 1.2e-6 (0.01), weights 3e-11;
- refreshed against rebuilt CSR values: within the 4e-7 bound in all 12 cases, layer outputs and gradients within 1e-5 of
  the largest entry; captured fits equal eager ones bit for bit at 2 epochs per replay, at dropout 0.3 as well."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pygda_amd import ops
from pygda_amd.nn.reweight_gnn import GCN_reweight, GS_reweight, _ReweightedGraphCache
from tests.conftest import load_golden
from tests.test_pairalign_host import FITS, run_fit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIMIT = ops.PA_MAX_CLASSES


def _close(gpu, f32, f64, name, slack):
    """|gpu - f64| <= 8 |fp32 torch - f64| + slack max|f64|."""
    gpu, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                     for v in (gpu, f32, f64))
    e_gpu, e_ref = (np.abs(gpu - f64).max(), np.abs(f32 - f64).max()) if f64.size else (0.0, 0.0)
    scale = max(np.abs(f64).max(), 1e-30) if f64.size else 1.0
    lim = 8 * e_ref + slack * scale
    print(f"[pairalign] {name}: gpu {e_gpu:.3e} fp32-torch {e_ref:.3e} rel {e_gpu / scale:.3e} limit {lim:.3e}")
    assert e_gpu <= lim, f"{name}: |gpu - f64| = {e_gpu:.3e} > {lim:.3e} (fp32 torch {e_ref:.3e})"


# -------------------------------------------------------------------------------------- (a) edge-pair statistics --
def _edge_ref(z, ei, cls, K, dtype):
    """calc_edge_rw_pseudo's sums: the per-edge outer products, added up per ordered class pair."""
    n, c = z.shape
    zd = z.to(dtype)
    ci = torch.zeros(n, dtype=torch.int64, device=z.device) if cls is None else cls
    outer = torch.einsum("bi,bj->bij", zd[ei[0]], zd[ei[1]]).reshape(-1, c * c)
    S = torch.zeros(K * K, c * c, dtype=dtype, device=z.device).index_add_(0, ci[ei[0]] * K + ci[ei[1]], outer)
    return S.view(K, K, c, c).permute(0, 2, 1, 3)


def _check_edge_stats(z, ei, cls, K, name):
    n = z.size(0)
    plan = ops.PaEdgePlan(ei, n, cls, K)
    got = ops.pa_edge_stats(z, plan)
    assert got.dtype == torch.float64 and got.shape == (K, z.size(1), K, z.size(1))
    _close(got, _edge_ref(z, ei, cls, K, torch.float32), _edge_ref(z, ei, cls, K, torch.float64), name, 2e-6)
    assert torch.equal(got, ops.pa_edge_stats(z, plan))                      # fixed partials, fixed order
    assert plan.seg.size(0) <= n + ei.size(1) // ops.PA_SEGMENT              # nothing of edge extent
    return got


@pytest.mark.parametrize("n,c,k", [(n, c, k) for n in (1, 2, 63, 65, 257) for c in (1, 2, 5, 7, LIMIT)
                                   for k in sorted({1, c})])
def test_edge_stats_against_float64(n, c, k):
    g = torch.Generator().manual_seed(1000 * n + 10 * c + k)
    ei = torch.randint(0, n, (2, 4 * n), generator=g).to(DEV)                # duplicates and self loops occur
    z = (torch.randn(n, c, generator=g) * 2).to(DEV)
    cls = None if k == 1 else torch.randint(0, k, (n,), generator=g).to(DEV)
    _check_edge_stats(z, ei, cls, k, f"edge stats n={n} c={c} k={k}")


def test_edge_stats_special_graphs():
    g = torch.Generator().manual_seed(5)
    c = k = 5
    n = 400
    z = torch.randn(n, c, generator=g).to(DEV)
    cls = torch.randint(0, k, (n,), generator=g)
    cls[cls == 3] = 2                                                        # a class with no node
    cls = cls.to(DEV)
    none = torch.zeros(2, 0, dtype=torch.int64, device=DEV)
    got = _check_edge_stats(z, none, cls, k, "no edges")
    assert float(got.abs().max()) == 0.0
    hub = torch.stack([torch.zeros(300, dtype=torch.int64), torch.randint(0, n, (300,), generator=g)])
    rest = torch.randint(0, n, (2, 900), generator=g)
    dup = torch.tensor([[7, 7, 7, 9, 9], [8, 8, 8, 9, 9]])                   # a triple edge and a double self loop
    ei = torch.cat([hub, rest, dup], 1).to(DEV)
    plan = ops.PaEdgePlan(ei, n, cls, k)
    assert int((plan.seg[:, 0] == 0).sum()) >= 5                             # the hub row is cut into segments
    got = _check_edge_stats(z, ei, cls, k, "hub row, empty class, duplicates")
    assert float(got[3].abs().max()) == 0.0 and float(got[:, :, 3].abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.PaEdgePlan(ei, n, cls + 1, k)
    with pytest.raises(Exception):
        ops.pa_edge_stats(torch.zeros(n, LIMIT + 1, device=DEV), ops.PaEdgePlan(ei, n, None, 1))


# -------------------------------------------------------------------------------------------- (b) softmax sums --
def _soft_ref(z, cls, K, dtype):
    p = torch.softmax(z.to(dtype), dim=1)
    ci = torch.zeros(z.size(0), dtype=torch.int64, device=z.device) if cls is None else cls
    return torch.zeros(K, z.size(1), dtype=dtype, device=z.device).index_add_(0, ci, p)


@pytest.mark.parametrize("n,c", [(n, c) for n in (1, 2, 63, 65, 257, 5000) for c in (1, 2, 5, 7, LIMIT)])
def test_softmax_sums_against_float64(n, c):
    g = torch.Generator().manual_seed(77 * n + c)
    z0 = (torch.randn(n, c, generator=g) * 3).to(DEV)
    z1 = (torch.randn(n + 3, c, generator=g) * 3).to(DEV)
    z0[0] = 80.0 * (torch.arange(c, device=DEV) % 2 * 2 - 1)                 # rows of +-80 stay finite
    z1[-1] = -80.0
    cls = torch.randint(0, c, (n,), generator=g).to(DEV)
    plan = ops.PaSoftPlan(n, cls, c, n + 3, None, 1, DEV)
    p0, p1 = ops.pa_softmax_sums(z0, z1, plan)
    assert p0.shape == (c, c) and p1.shape == (1, c) and bool(torch.isfinite(p0).all() and torch.isfinite(p1).all())
    _close(p0, _soft_ref(z0, cls, c, torch.float32), _soft_ref(z0, cls, c, torch.float64), f"softmax sums src n={n} c={c}", 2e-6)
    _close(p1, _soft_ref(z1, None, 1, torch.float32), _soft_ref(z1, None, 1, torch.float64), f"softmax sums tgt n={n} c={c}", 2e-6)
    q0, q1 = ops.pa_softmax_sums(z0, z1, plan)
    assert torch.equal(p0, q0) and torch.equal(p1, q1)


# --------------------------------------------------------------------------------------- (c) coefficient loss --
def _ce_ref(x, y, coef, sel, dtype):
    x = x.detach().to(dtype).requires_grad_(True)
    xs, ys = (x, y) if sel is None else (x[sel], y[sel])
    loss = torch.mean(coef.to(dtype)[ys] * F.cross_entropy(xs, ys, reduction="none"))
    (g,) = torch.autograd.grad(loss * 2.5, x)
    return loss.detach(), g


@pytest.mark.parametrize("n,c", [(1, 2), (257, 5), (5000, 5), (5000, LIMIT), (65, 1)])
@pytest.mark.parametrize("masked", [False, True])
def test_coefficient_ce_against_float64(n, c, masked):
    g = torch.Generator().manual_seed(13 * n + c)
    x = (torch.randn(n, c, generator=g) * 3).to(DEV).requires_grad_()
    y = torch.randint(0, c, (n,), generator=g).to(DEV)
    coef = (torch.rand(c, generator=g) * 3).to(DEV)
    sel = None
    if masked:
        keep = torch.rand(n, generator=g) < 0.6
        keep[0] = True
        if c > 2:
            keep &= (y != 1).cpu()                                           # a class absent from the mask
            keep[int(torch.nonzero((y != 1).cpu())[0])] = True
        sel = torch.nonzero(keep).view(-1).to(DEV)
        coef[1 % c] = float("inf") if c > 2 else coef[1 % c]                 # ... whose coefficient is never read
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    loss = ops.pa_ce(x, y, coef, sel, stats)
    (gx,) = torch.autograd.grad(loss * 2.5, x)
    safe = torch.where(torch.isinf(coef), torch.zeros_like(coef), coef)
    l32, g32 = _ce_ref(x, y, safe, sel, torch.float32)
    l64, g64 = _ce_ref(x, y, safe, sel, torch.float64)
    _close(loss, l32, l64, f"ce loss n={n} c={c} masked={masked}", 1e-6)
    _close(gx, g32, g64, f"ce grad n={n} c={c} masked={masked}", 1e-5)
    assert float(stats[0]) == float(loss.detach()) and float(stats[1]) == float((x.argmax(dim=1) == y).sum())   # over ALL rows
    if masked:
        out = torch.ones(n, dtype=torch.bool, device=DEV)
        out[sel] = False
        assert float(gx[out].abs().max()) == 0.0 if bool(out.any()) else True
    assert torch.equal(ops.pa_ce(x, y, coef, sel), loss)


def test_coefficient_ce_reads_coef_at_replay_time():
    g = torch.Generator().manual_seed(3)
    n, c = 300, 5
    x = torch.randn(n, c, generator=g).to(DEV).requires_grad_()
    y = torch.randint(0, c, (n,), generator=g).to(DEV)
    sel = torch.nonzero(torch.rand(n, generator=g) < 0.5).view(-1).to(DEV)
    coef = torch.ones(c, device=DEV)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)

    def step():
        loss = ops.pa_ce(x, y, coef, sel, stats)
        return loss, torch.autograd.grad(loss, x)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        loss, gx = step()
    graph.replay()
    l1, g1 = loss.clone(), gx.clone()
    new = torch.tensor([2.0, 0.5, 4.0, 1.0, 8.0], device=DEV)
    coef.copy_(new)                                                          # in place: the captured graph is not touched
    graph.replay()
    l2, g2 = loss.clone(), gx.clone()
    e1, ge1 = step()
    assert torch.equal(l2, e1) and torch.equal(g2, ge1) and not torch.equal(l1, l2)
    coef.fill_(1.0)
    graph.replay()
    assert torch.equal(loss, l1) and torch.equal(gx, g1)


# -------------------------------------------------------------------------------------------- (d) value refresh --
@pytest.mark.parametrize("kind,aggr", [("GS", "mean"), ("GS", "add"), ("GCN", "mean"), ("GCN", "add")])
@pytest.mark.parametrize("lmda", [0.0, 0.3, 1.0])
def test_refresh_against_the_rebuilt_csr(kind, aggr, lmda):
    g = torch.Generator().manual_seed(17)
    n, c, d = 300, 5, 8
    ei = torch.cat([torch.randint(0, n, (2, 1500), generator=g), torch.tensor([[4, 4, 9], [6, 6, 9]])], 1)
    ei = ei[:, (ei[0] != 11) & (ei[1] != 11)].to(DEV)                       # an isolated node
    cls = torch.randint(0, c, (n,), generator=g).to(DEV)
    rw = (torch.rand(c, c, generator=g) * 2 + 0.1).to(DEV)
    torch.manual_seed(5)
    layer = (GS_reweight(d, d, aggr) if kind == "GS" else GCN_reweight(d, d, aggr)).to(DEV)
    flags = layer.graph_flags()
    pg = ops.PaGraph(ei, n, None, lmda, *flags)
    ops.pa_refresh(pg, cls, rw)
    w = rw.view(-1)[cls[ei[0]] * c + cls[ei[1]]]
    ref = _ReweightedGraphCache().get(ei, w, lmda, n, *flags)
    nnz = ref.nnz
    for a, b, name in ((pg.graph.val, ref.val, "val"), (pg.graph.t_val, ref.t_val, "t_val")):
        assert torch.allclose(a[:nnz], b[:nnz], rtol=4e-7, atol=0), name
    assert torch.equal(pg.graph.colidx[:nnz], ref.colidx[:nnz]) and torch.equal(pg.graph.t_colidx[:nnz], ref.t_colidx[:nnz])
    x = torch.randn(n, d, generator=g).to(DEV)
    outs = []
    for run in (lambda xi: layer.forward_on(xi, pg.graph), lambda xi: layer(xi, ei, w, lmda)):
        xi = x.clone().requires_grad_()
        out = run(xi)
        grads = torch.autograd.grad((out * out).sum(), [xi, *layer.parameters()])
        outs.append((out.detach(), *grads))
    # values six fp32 roundings apart (3.6e-7), outputs linear in them: 1e-5 of the largest entry leaves a factor 30
    for a, b in zip(*outs):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-12
    if lmda in (0.0, 1.0):                                                    # unit weights give the base values back
        ops.pa_refresh(pg, cls, torch.ones_like(rw))
        assert torch.equal(pg.graph.val[:nnz], pg.base[:nnz]) and torch.equal(pg.graph.t_val[:nnz], pg.t_base[:nnz])


# ------------------------------------------------------------------------------------------------------- the fits --
@pytest.fixture(scope="module")
def G():
    return load_golden("pairalign_fit")


@pytest.fixture(scope="module")
def host64(G):
    """The project's host path in double on the fixture, once per configuration."""
    return {tag: run_fit(G, tag, "cpu", torch.float64) for tag in FITS}


def _fit_figures(m, s, t, log):
    state = m.gnn.state_dict()
    return dict(losses=[l for l, *_ in log], ew=np.stack([e for _, _, e, _, _ in log]),
                lw=np.stack([l for _, _, _, l, _ in log]), edge_weight=np.stack([w for *_, w in log]),
                src_logits=m.predict(s)[0], tgt_logits=m.predict(t)[0],
                **{"final/" + k: v for k, v in state.items() if v.is_floating_point()})


@pytest.mark.parametrize("tag", ["GS", "GCN"])
def test_device_fit_against_the_record(G, host64, tag):
    m, s, t, log = run_fit(G, tag, DEV)
    got = _fit_figures(m, s, t, log)
    f64 = _fit_figures(*host64[tag])
    for k, v in got.items():
        _close(v, G[f"{tag}/{k}"], f64[k], f"{tag} fit {k}", 1e-5 if k == "losses" else 1e-4)
    # an arg-max on a near-tie may fall the other way under another summation order: at most one row of the 50 / 40
    accs = np.array([a for _, a, *_ in log])
    assert np.abs(accs - G[f"{tag}/accs"]).max() <= 1.0 / s.x.size(0) + 1e-12
    assert int((t.y_hat.cpu() != torch.from_numpy(G[f"{tag}/y_hat"])).sum()) <= 1
    assert len(m.solves) == sum(sum(m._fires(e)) for e in range(m.epoch))


def _bits(m, s, t, log):
    return ([(l, a) for l, a, *_ in log], [v.clone() for v in m.gnn.state_dict().values()], s.edge_weight.clone(),
            np.array(s.lw), np.array(s.ew), t.y_hat.clone(), m.predict(t)[0].clone())


def _same(a, b):
    assert a[0] == b[0]
    for u, v in zip(a[1], b[1]):
        assert torch.equal(u, v)
    assert torch.equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert torch.equal(a[5], b[5]) and torch.equal(a[6], b[6])


def test_fit_with_dropout_draws_from_the_project_stream(G):
    """Dropout above 0: parity with the reference is in distribution only, but the masks come from the project's
    Philox stream, so a fit is a function of (seed, step counter) and a captured fit replays the eager one's masks."""
    runs = []
    for graphed in (False, True):
        ops.dropout_state.counter(torch.device(DEV)).zero_()
        runs.append(_bits(*run_fit(G, "GS", DEV, dropout=0.3, use_hip_graph=graphed, epochs_per_graph=2)))
    assert all(np.isfinite(l) for l, _ in runs[0][0])
    assert runs[0][0][-1][0] < runs[0][0][0][0]                              # it still trains
    assert runs[0][0] == runs[1][0]
    for u, v in zip(runs[0][1], runs[1][1]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("tag", ["GS", "GCN"])
def test_captured_fit_is_bit_equal_to_eager_and_repeatable(G, tag):
    eager = _bits(*run_fit(G, tag, DEV, use_hip_graph=False))
    captured = _bits(*run_fit(G, tag, DEV, use_hip_graph=True, epochs_per_graph=2))
    again = _bits(*run_fit(G, tag, DEV, use_hip_graph=True, epochs_per_graph=2))
    _same(eager, captured)
    _same(captured, again)
