"""GTrans on the MI355X: the kernels of csrc/gda_gtrans.hip against float64 -- the norm with its fold, keep mask and
degrees, the aggregation on the refreshed CSRs, the gradient to the features and (SDDMM and chain) to the flip weights on
a graph with a duplicate edge, an explicit self loop, a one-way edge, an isolated node, zero-weight edges, a row whose
edges are all dropped, pre-fold values on both sides of 1 and exactly 1 and, at 300 nodes, a row of 271 entries in either
CSR; the loss with a zero row and both margins; the projection against the outputs recorded from the reference -- each
held against torch-float32's own distance to float64 on the same inputs (the host fallbacks are the yardsticks); two runs
bit-identical; the fits against the fixtures recorded from the reference's own gtrans.py with the host test's check;
eager and captured fits bit-identical; one iteration at the ACMv9 -> DBLPv7 stand-in shapes."""
import os

import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import ops
from tests.test_gpu_acdne import _close
from tests.test_gtrans_host import (FIXTURES, HERE, PROJECT_BOUND, check_fit_against_fixture, fixture, plan_inputs,
                                    run_fit)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(gpu, f32, f64, name, slack=2e-6):
    """``_close`` of tests/test_gpu_acdne.py, the figures printed first."""
    a, b, c = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64) for v in (gpu, f32, f64))
    print(f"{name}: |gpu - f64| = {np.abs(a - c).max():.3e}, |fp32 torch - f64| = {np.abs(b - c).max():.3e}")
    _close(gpu, f32, f64, name, slack)


_PLANS = {}


def plans(n):
    """The crafted graph on ``n`` nodes once: the host plan, its device twin and the shared inputs (left unchanged)."""
    if n not in _PLANS:
        plan, ei, mei, w_edges, p, keep = plan_inputs(n, 40 + n, hub=n >= 300)
        _PLANS[n] = (plan, ops.wgcn_plan(ei, n, mei, device=DEV), w_edges, p, keep)
    return _PLANS[n]


@pytest.mark.parametrize("n", [1, 67, 300])
@pytest.mark.parametrize("d", [4, 20, 128, 256])
def test_norm_aggregation_and_both_gradients_against_float64(n, d):
    hp, dp, w_edges, p, keep = plans(n)
    if n >= 300:
        assert int((hp.rowptr[1:] - hp.rowptr[:-1]).max()) > 256 and int((hp.t_rowptr[1:] - hp.t_rowptr[:-1]).max()) > 256
    g = torch.Generator().manual_seed(n * 1000 + d)
    h, G = torch.randn(n, d, generator=g, dtype=torch.float64), torch.randn(n, d, generator=g, dtype=torch.float64)
    bias = torch.randn(d, generator=g, dtype=torch.float64)

    def run(plan, dtype, dev):
        hh = h.to(dev, dtype).requires_grad_(True)
        pp = p.to(dev, dtype).requires_grad_(True) if plan.m else None
        kk = keep.to(dev).float() if dev != "cpu" else keep
        val, w = ops.wgcn_norm(plan, plan.entry_weights(w_edges.to(dev, dtype)), pp, keep=kk)
        y = ops.weighted_propagate(hh, plan, val, bias.to(dev, dtype))
        grads = torch.autograd.grad((y * G.to(dev, dtype)).sum(), [hh] + ([pp] if plan.m else []))
        return [y.detach(), w.detach(), val.detach().clone()] + list(grads)

    r64, r32 = run(hp, torch.float64, "cpu"), run(hp, torch.float32, "cpu")
    rd, rd2 = run(dp, torch.float32, DEV), run(dp, torch.float32, DEV)
    for name, a, b, c, c2 in zip(("y", "w", "val", "dL/dh", "dL/dp"), r64, r32, rd, rd2):
        assert torch.isfinite(c).all(), name
        close(c, b, a, f"{name}[n={n}, d={d}]")
        assert torch.equal(c, c2), name                                             # two runs: the same bits
    tv = torch.empty_like(dp.graphs[0].t_val)
    tv.copy_(dp.graphs[0].val[dp.t_to_fwd.long()])
    assert torch.equal(tv, dp.graphs[0].t_val)                                      # the by-source twin, through t_to_fwd


def test_keep_bits_are_the_dropout_stream_indexed_by_the_listed_edge():
    """Every bit against the numpy Philox of tests/test_gpu_parity.py: key (seed, (step << 20) ^ site), element index
    ``epos`` -- the edge's position in the coalesced list, not the entry's in the CSR --, no rescaling."""
    from tests.test_gpu_parity import _philox_keep
    hp, dp, w_edges, p, keep = plans(300)
    w_prev = dp.entry_weights(w_edges.float().to(DEV))
    ops.dropout_state.next_step(torch.device(DEV))
    site = ops.dropout_state.site
    val, _ = ops.wgcn_norm(dp, w_prev, None, p_drop=0.05, view=0)
    val = val.clone()
    step = int(ops.dropout_state.counter(torch.device(DEV)).item())
    want = _philox_keep(ops.dropout_state.seed, step, site + 1, hp.ec, 0.05)         # one bit per listed edge
    assert 0 < int((~want).sum()) < hp.ec // 8
    ops.dropout_state.site = site                                                   # the same step and site: the same bits
    assert torch.equal(ops.wgcn_norm(dp, w_prev, None, p_drop=0.05, view=0)[0], val)
    r64 = ops.wgcn_norm(hp, hp.entry_weights(w_edges), None, keep=want)[0]
    r32 = ops.wgcn_norm(hp, hp.entry_weights(w_edges.float()), None, keep=want)[0]
    close(val, r32, r64, "val under the stream's keep bits")
    listed = (hp.epos >= 0) & (hp.erow != hp.col) & (r64 != 0)
    kept_entry = torch.ones(hp.nnz, dtype=torch.bool)
    kept_entry[hp.epos >= 0] = want[hp.epos[hp.epos >= 0]]
    full = ops.wgcn_norm(hp, hp.entry_weights(w_edges), None)[0]
    live = (hp.epos >= 0) & (hp.erow != hp.col) & (full != 0)
    assert torch.equal((val.cpu() == 0)[live], ~kept_entry[live])                   # exactly the stream's dropped edges
    assert (val.cpu()[hp.erow == hp.col] > 0).all()                                 # a self loop always carries weight


@pytest.mark.parametrize("n", [1, 63, 1001])
@pytest.mark.parametrize("d", [1, 16, 129])
@pytest.mark.parametrize("margin", [-1, 0.3])
def test_loss_against_float64(n, d, margin):
    g = torch.Generator().manual_seed(n * 1000 + d)
    o = [torch.randn(n, d, generator=g, dtype=torch.float64) for _ in range(3)]
    zero = n // 2
    for t in o:
        t[zero] = 0                                                                 # one all-zero row

    def run(dtype, dev):
        leaves = [t.to(dev, dtype).requires_grad_(True) for t in o]
        loss, parts = ops.gtrans_loss(*leaves, margin)
        return [loss.detach(), parts] + list(torch.autograd.grad(loss, leaves))

    r64, r32, rd, rd2 = run(torch.float64, "cpu"), run(torch.float32, "cpu"), run(torch.float32, DEV), run(torch.float32, DEV)
    for name, a, b, c, c2 in zip(("loss", "parts", "g1", "g2", "g3"), r64, r32, rd, rd2):
        assert torch.isfinite(c).all(), name                                        # the zero row: no NaN
        close(c, b, a, f"{name}[n={n}, d={d}, margin={margin}]")
        assert torch.equal(c, c2), name
    for gz in rd[2:]:
        assert (gz[zero] == 0).all()


@pytest.mark.parametrize("case", ["one", "below", "above", "mid", "mid_below", "big"])
def test_project_against_the_reference(case):
    f = np.load(os.path.join(HERE, "gtrans_perturb.npz"))
    v, budget = torch.from_numpy(f[f"project/{case}/in"]), int(f[f"project/{case}/budget"])
    assert v.numel() in (1, 50, 1000, 40000)
    out = ops.gtrans_project(v.clone().to(DEV), budget).double().cpu().numpy()
    e32, e64 = np.abs(out - f[f"project/{case}/out32"]).max(), np.abs(out - f[f"project/{case}/out64"]).max()
    print(f"{case} (m = {v.numel()}): against the reference's float32 {e32:.3e}, float64 {e64:.3e} (bound {PROJECT_BOUND:.3e})")
    assert e32 <= PROJECT_BOUND and e64 <= PROJECT_BOUND
    assert np.array_equal(out, ops.gtrans_project(v.clone().to(DEV), budget).double().cpu().numpy())
    if case == "big":                                                               # 40,000 entries below the budget
        low = ops.gtrans_project(v.clone().to(DEV), 10 ** 6).cpu()
        assert torch.equal(low, v.clamp(1e-7, 1 - 1e-7))
        neg = v.clone()
        neg[::3] = -0.5                                                             # the clamp that follows the Adam step
        got = ops.gtrans_project(neg.clone().to(DEV), 10 ** 6).cpu()
        assert torch.equal(got, neg.clamp(min=1e-7).clamp(1e-7, 1 - 1e-7))


@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_fit_matches_the_reference(name):
    f, s, t = fixture(name)
    m, got = run_fit(f, s, t, DEV, replay=True)
    assert len(got["src_losses"]) == 12 and got["steps"].shape == (12 + 20, 3)
    check_fit_against_fixture(got, f)


@pytest.mark.parametrize("stepped", [False, True])
def test_eager_and_captured_fits_are_bit_identical(stepped):
    f, s, t = fixture(FIXTURES[1])
    kw = dict(replay=True, step_structure=stepped, epochs_per_graph=2)
    _, eager = run_fit(f, s, t, DEV, use_hip_graph=False, **kw)
    _, captured = run_fit(f, s, t, DEV, use_hip_graph=True, **kw)
    for k in eager:
        assert np.array_equal(eager[k], captured[k]), k
    if stepped:
        assert (eager["p_iter"][-1] > 1e-6).sum() > 0 and np.isfinite(eager["logits"]).all()
        k = int(f["n_perturbations"])
        assert np.clip(eager["p_iter"], 0, 1).sum(1).max() <= k + 1e-5 * eager["p_iter"].shape[1]


@pytest.mark.parametrize("margin", [-1, 0.3])
def test_loss_gradient_to_the_flip_weights_against_float64(margin):
    """``test_time_loss`` as the trainer composes it -- both views' norms, a two-layer bottleneck on each of the three
    passes, the loss -- on the 300-node graph (rows of 271 entries in either CSR: the SpMM's chunked rows on the refreshed
    values, the second view on the first one's split; the duplicate edge's group of two): the loss and its gradients to
    the flip weights and to the features against the float64 composition of the host fallbacks, by ``_close``."""
    hp, dp, w_edges, p, keep = plans(300)
    n, d = 300, 20
    assert dp.graphs[0].split(False).n_long > 0 and dp.graphs[0].split(True).n_long > 0
    assert dp.graphs[1].split(False) is dp.graphs[0].split(False)
    g = torch.Generator().manual_seed(9)
    h0 = torch.randn(n, d, generator=g, dtype=torch.float64)
    W, b0, b1 = (torch.randn(*s_, generator=g, dtype=torch.float64) / 4 for s_ in ((d, d), (d,), (d,)))
    perm = torch.randperm(n, generator=g)

    def run(plan, dtype, dev):
        hh = h0.to(dev, dtype).requires_grad_(True)
        pp = p.to(dev, dtype).requires_grad_(True)
        w_prev = plan.entry_weights(w_edges.to(dev, dtype))
        Wd, b0d, b1d = (t.to(dev, dtype) for t in (W, b0, b1))
        v1, _ = ops.wgcn_norm(plan, w_prev, pp, keep=keep.to(dev).to(dtype) if dev != "cpu" else keep, view=0)
        v2, _ = ops.wgcn_norm(plan, w_prev, pp, view=1)
        lin = (lambda x: ops.linear_nt(x, Wd)) if dev != "cpu" else (lambda x: x @ Wd.t())
        outs = []
        for x, val, view in ((hh, v1, 0), (hh, v2, 1), (hh[perm.to(dev)], v2, 1)):
            y = torch.relu(ops.weighted_propagate(x, plan, val, b0d, view))
            outs.append(ops.weighted_propagate(lin(y), plan, val, b1d, view))
        loss, parts = ops.gtrans_loss(*outs, margin)
        return [loss.detach(), parts] + list(torch.autograd.grad(loss, [pp, hh]))

    r64, r32 = run(hp, torch.float64, "cpu"), run(hp, torch.float32, "cpu")
    rd, rd2 = run(dp, torch.float32, DEV), run(dp, torch.float32, DEV)
    for name, a, b, c, c2 in zip(("loss", "parts", "dL/dp", "dL/dh0"), r64, r32, rd, rd2):
        close(c, b, a, f"{name}[margin={margin}]")
        assert torch.equal(c, c2), name
    pairs = [hp.gidx[hp.gptr[u]:hp.gptr[u + 1]] for u in range(hp.mu) if hp.gptr[u + 1] - hp.gptr[u] == 2]
    assert pairs and all(torch.equal(rd[2].cpu()[k[0]], rd[2].cpu()[k[1]]) for k in pairs)   # a duplicate edge's two weights
    assert float(r64[2].abs().max()) > 0
    with pytest.raises(pygda_amd._lib.GdaError, match="refreshed"):                  # a view refreshed before its backward
        pp = p.float().to(DEV).requires_grad_(True)
        w_prev = dp.entry_weights(w_edges.float().to(DEV))
        v, _ = ops.wgcn_norm(dp, w_prev, pp, view=0)
        y = ops.weighted_propagate(h0.float().to(DEV).requires_grad_(True), dp, v, None, 0)
        ops.wgcn_norm(dp, w_prev, pp, view=0)
        y.sum().backward()


def test_one_iteration_at_the_acm_dblp_shapes():
    from bench import make_cfg_a
    src, tgt = make_cfg_a()
    m = pygda_amd.models.GTrans(src.x.size(1), 128, 5, device=DEV, epoch=5, verbose=0, record=True, step_structure=True)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    np.random.seed(0)
    m.fit(src, tgt)
    logits, _ = m.predict(tgt)
    assert len(log) == 5 + 1 and all(np.isfinite(v) for v in log) and np.isfinite(m.parts_log).all()
    assert len(m.parts_log) == 5 + 20 and logits.shape == (5484, 5) and torch.isfinite(logits).all()
