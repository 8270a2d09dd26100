"""ACDNE on the MI355X: the kernels of csrc/gda_acdne.hip against float64 (process_graph at the fixture's size and at
N = 9,360, step 3; the proximity loss and the heads at several batch sizes, an odd one among them), two runs
bit-identical, the 3-epoch fit against the reference's fixture with the bound taken from the float64 restatement,
eager and captured fits bit-identical, one full-size epoch at the DBLPv7 -> Citationv1 shapes, and no BLAS product on
the path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import ops
from pygda_amd.data import Data
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(in_dim=24, hid_dim=16, num_classes=3, n_emb=12, pair_weight=0.1, step=3, dropout=0.0, lr=0.01,
          weight_decay=0.001, batch_size=40)


def _close(gpu, f32, f64, name, slack=2e-6):
    """|gpu - f64| <= 8 |fp32 torch - f64| + slack max|f64|."""
    gpu, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                     for v in (gpu, f32, f64))
    e_gpu, e_ref = np.abs(gpu - f64).max(), np.abs(f32 - f64).max()
    lim = 8 * e_ref + slack * max(np.abs(f64).max(), 1e-30)
    assert e_gpu <= lim, f"{name}: |gpu - f64| = {e_gpu:.3e} > {lim:.3e} (fp32 torch {e_ref:.3e})"


def _torch_process_graph(ei, x, n, step, dtype):
    """process_graph's lines in torch (dense, on the device) at ``dtype``: the test's own yardstick."""
    adj = torch.zeros(n, n, dtype=dtype, device=DEV)
    adj.index_put_((ei[0].to(DEV), ei[1].to(DEV)), torch.ones(ei.size(1), dtype=dtype, device=DEV), accumulate=True)

    def scale(w):
        return (1.0 / (w.sum(1) + 1e-12))[:, None] * w

    g = scale(adj)
    a_k, a = g, g.clone()
    for k in range(2, step + 1):
        a_k = a_k @ g
        a = a + a_k / k
    a.fill_diagonal_(0)
    a = scale(a)
    col = a.sum(0)
    col[col == 0] = 1
    ppmi = torch.log(n * a / col[None, :] + 1e-12)
    ppmi = torch.nan_to_num(ppmi, nan=0.0).clamp_min(0)
    return ppmi, scale(ppmi) @ x.to(DEV, dtype)


def _random_graph(n, e, f, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei = torch.cat([ei, ei.flip(0), ei[:, :3]], 1)
    ei = ei[:, ei[0] != ei[1]]
    x = (torch.rand(n, f, generator=g) < 0.02).float()
    return ei, x


@pytest.mark.parametrize("n,e,f,step", [(160, 360, 24, 1), (160, 360, 24, 2), (160, 360, 24, 3), (1001, 2500, 300, 3),
                                        (9360, 15556, 512, 3)])
def test_process_graph_against_float64(n, e, f, step):
    ei, x = _random_graph(n, e, f, n + step)
    a, xn = ops.acdne_process_graph(ei.to(DEV), x.to(DEV), n, step)
    a64, xn64 = _torch_process_graph(ei, x, n, step, torch.float64)
    a32, xn32 = _torch_process_graph(ei, x, n, step, torch.float32)
    _close(a, a32, a64, "A_ppmi", 1e-5)
    _close(xn, xn32, xn64, "X_nei", 1e-5)
    a2, xn2 = ops.acdne_process_graph(ei.to(DEV), x.to(DEV), n, step)
    assert torch.equal(a, a2) and torch.equal(xn, xn2)
    del a64, a32, a, a2
    torch.cuda.empty_cache()


def test_process_graph_matches_the_reference_fixture():
    gr = load_golden("acdne_graph")
    for step in (1, 2, 3):
        a, x = ops.acdne_process_graph(torch.tensor(gr["src_ei"]).to(DEV), torch.tensor(gr["src_x"]).to(DEV), 160, step)
        np.testing.assert_allclose(a.cpu().numpy(), gr[f"ppmi32_s{step}"], atol=2e-5)
        np.testing.assert_allclose(x.cpu().numpy(), gr[f"xnei32_s{step}"], atol=2e-6)
        assert not a[7].any() and not a[:, 7].any()


def _step_inputs(h, e, c, seed, ns=300, nt=250):
    g = torch.Generator().manual_seed(seed)
    ps = (torch.rand(ns, ns, generator=g) * (torch.rand(ns, ns, generator=g) < 0.3)).float()
    pt = (torch.rand(nt, nt, generator=g) * (torch.rand(nt, nt, generator=g) < 0.3)).float()
    pidx = torch.cat([torch.randperm(ns, generator=g)[:h], torch.randperm(nt, generator=g)[:h]])
    rows = torch.cat([torch.randperm(ns, generator=g)[:h], torch.randperm(nt, generator=g)[:h] + ns])
    z = torch.randn(2 * h, e, generator=g)
    y = torch.randint(0, c, (ns,), generator=g)
    params = [torch.randn(c, e, generator=g) * 0.3, torch.randn(c, generator=g) * 0.1,
              torch.randn(128, e, generator=g) * 0.2, torch.randn(128, generator=g) * 0.1,
              torch.randn(128, 128, generator=g) * 0.1, torch.randn(128, generator=g) * 0.1,
              torch.randn(2, 128, generator=g) * 0.1, torch.randn(2, generator=g) * 0.1]
    return ps, pt, pidx, rows, z, y, params


def _losses64(ps, pt, pidx, rows, z, y, params, alpha, pw):
    """The step's loss and gradients in float64 by autograd (GradReverse as a hook)."""
    h = z.size(0) // 2
    z = z.double().requires_grad_(True)
    P = [p.double().requires_grad_(True) for p in params]
    emb = torch.relu(z)
    net = 0.0
    for d, M in enumerate((ps, pt)):
        ix = pidx[d * h:(d + 1) * h]
        a = M.double()[ix][:, ix].clone()
        a.fill_diagonal_(0)
        a = (1.0 / (a.sum(1) + 1e-12))[:, None] * a
        e_ = emb[d * h:(d + 1) * h]
        r = (e_ * e_).sum(1, keepdim=True)
        net = net + ((a * (r - 2 * e_ @ e_.T + r.T)).sum(1)).mean()
    clf = F.cross_entropy(F.linear(emb, P[0], P[1])[:h], y[rows[:h]])
    er = emb * 1.0
    er.register_hook(lambda g: -alpha * g)
    d = F.linear(F.relu(F.linear(F.relu(F.linear(er, P[2], P[3])), P[4], P[5])), P[6], P[7])
    dom = F.cross_entropy(d, torch.cat([torch.zeros(h), torch.ones(h)]).long())
    total = clf + dom + pw * net
    grads = torch.autograd.grad(total, [z] + P)
    return total.detach(), grads


@pytest.mark.parametrize("h,e,c", [(20, 12, 3), (37, 128, 5), (50, 128, 5), (128, 64, 7)])
def test_prox_and_heads_against_float64(h, e, c):
    ps, pt, pidx, rows, z, y, params = _step_inputs(h, e, c, h * 31 + c)
    alpha, pw = 0.7, 0.1
    total64, g64 = _losses64(ps, pt, pidx, rows, z, y, params, alpha, pw)
    d = [t.to(DEV) for t in (ps, pt, pidx, rows, z, y)]
    dp = [p.to(DEV) for p in params]
    al = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)

    def run():
        prox, gprox = ops.acdne_prox(d[0], d[1], d[2], d[4], h, pw)
        return prox, gprox, ops.acdne_heads(d[4], gprox, dp, d[5], d[3], al, prox, pw, loss_acc=acc)

    prox, gprox, (loss, dz, grads) = run()
    np.testing.assert_allclose(loss.item(), total64.item(), rtol=2e-5)
    assert acc.item() == loss.item()
    for name, a, b in zip(["dz", "Wc", "bc", "W1", "b1", "W2", "b2", "W3", "b3"], [dz] + list(grads), g64):
        b = b.cpu().numpy()
        err = np.abs(a.cpu().double().numpy() - b).max()
        assert err <= 2e-5 * max(np.abs(b).max(), 1e-3), f"{name}: {err:.3e}"
    prox2, gprox2, (loss2, dz2, grads2) = run()
    assert torch.equal(prox, prox2) and torch.equal(gprox, gprox2) and torch.equal(loss, loss2)
    assert torch.equal(dz, dz2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


def _pair_dev(g):
    return (Data(x=torch.tensor(g["src_x"]), edge_index=torch.tensor(g["src_ei"]), y=torch.tensor(g["src_y"])),
            Data(x=torch.tensor(g["tgt_x"]), edge_index=torch.tensor(g["tgt_ei"]), y=torch.tensor(g["tgt_y"])))


def _fit(graph, steps_per_graph=4):
    g = load_golden("acdne_fit3")
    s, t = _pair_dev(g)
    log = []
    m = pygda_amd.models.ACDNE(device=DEV, epoch=3, verbose=0, use_hip_graph=graph, steps_per_graph=steps_per_graph,
                               **KW)
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    torch.manual_seed(411)
    np.random.seed(412)
    m.fit(s, t)
    out = dict(losses=np.array([l for l, _ in log]), accs=np.array([a for _, a in log]),
               tgt_prob=m.predict(t)[0].cpu().numpy(), src_prob=m.predict(s, train=True)[0].cpu().numpy())
    out.update({"final/" + k: v.cpu().numpy() for k, v in m.acdne.state_dict().items()})
    return out


def test_fit3_against_the_reference_bounded_by_the_float64_restatement():
    g = load_golden("acdne_fit3")
    hip = _fit(True)
    for k in ["losses", "tgt_prob", "src_prob"] + [k for k in g if k.startswith("final/")]:
        f64, ref32 = g["f64/" + k].astype(np.float64), g[k].astype(np.float64)
        floor = 1e-6 * max(np.abs(f64).max(), 1.0)             # stated floor: fp32 rounding of a unit-sized value
        err = np.abs(hip[k] - f64).max()
        assert err <= 2 * np.abs(ref32 - f64).max() + floor, f"{k}: {err:.3e}"
    np.testing.assert_array_equal(hip["accs"], g["accs"])


def test_eager_and_captured_fits_are_bit_identical():
    a, b = _fit(True, 4), _fit(False)
    c = _fit(True, 3)                                        # 8 steps: two replays of 3 and two eager steps
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], c[k]), k


def test_one_full_size_epoch_at_dblp_citation_shapes():
    from bench import make_cfg_a
    src, tgt = make_cfg_a(seed=7, ns=5484, es=8117, nt=8935, et=15098)
    m = pygda_amd.models.ACDNE(src.x.size(1), 128, 5, dropout=0.5, weight_decay=1e-3, lr=1e-3, device=DEV, epoch=1,
                               verbose=0)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    np.random.seed(0)
    m.fit(src, tgt)
    assert len(log) == 1 and np.isfinite(log[0]) and log[0] > 0
    prob, _ = m.predict(tgt)
    assert prob.shape == (8935, 5) and torch.isfinite(prob).all()
    assert torch.allclose(prob.sum(1), torch.ones(8935, device=DEV), atol=1e-5)
    assert m.ppmi_t.shape == (8935, 8935) and torch.isfinite(m.whole_xs_xt_stt_nei).all()


def test_no_blas_product_on_the_acdne_path(monkeypatch):
    from bench import make_cfg_a
    src, tgt = make_cfg_a(seed=7, ns=1200, es=1800, nt=1000, et=1500)
    m = pygda_amd.models.ACDNE(src.x.size(1), 128, 5, device=DEV, epoch=2, verbose=0)
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
    m.fit(src, tgt)
    m.predict(tgt)
    torch.cuda.synchronize()
    assert calls == [], sorted(set(calls))
