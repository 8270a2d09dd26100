"""CWGCN on the MI355X: the loss kernels (csrc/gda_cwgcn.hip) against float64, the trainer against the reference's
fixtures (full batch eager and captured, bit-identical to each other; mini-batch; graph mode), the classifier left
untouched by stage 2, one full-size step of each stage against a float64 restatement, and no BLAS product on the
path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import ops
from pygda_amd.data import Data
from tests.conftest import T, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = [1, 2, 3, 67, 1000, 100003]
DS = [1, 5, 64, 128, 300, 1024]


def _close(gpu, f32, f64, name, slack=2e-6):
    """|gpu - f64| <= 8 |fp32 torch - f64| + slack max|f64| (NaN where float64 has NaN)."""
    gpu, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                     for v in (gpu, f32, f64))
    nan = np.isnan(f64)
    assert np.array_equal(np.isnan(gpu), nan), f"{name}: NaN pattern"
    if nan.all():
        return
    e_gpu, e_ref = np.abs(gpu - f64)[~nan].max(), np.abs(f32 - f64)[~nan].max()
    lim = 8 * e_ref + slack * max(np.abs(f64[~nan]).max(), 1e-30)
    assert e_gpu <= lim, f"{name}: |gpu - f64| = {e_gpu:.3e} > {lim:.3e} (fp32 torch {e_ref:.3e})"


def _strided(n, d, g):
    """[n, d] as a column view of a wider block (row stride d + 3)."""
    return (torch.randn(n, d + 3, generator=g) * 0.7 + 0.3)[:, 1:d + 1].to(DEV)


def _c_loss_torch(z, y):
    d = torch.sum(torch.square(z - F.one_hot(y, z.size(1)).to(z.dtype)), dim=1)
    return torch.mean(1 - torch.exp(torch.div(-d, 100))), torch.exp(torch.div(-d, 10))


def _moments_torch(x, w):
    sw = torch.sum(w)
    w = w.view(-1, 1) * (1 / sw)
    mean = torch.sum(x * w, dim=0)
    var = torch.sum(torch.pow(x - mean, 2) * w, dim=0)
    return mean, torch.pow(var / (1 - torch.sum(torch.pow(w, 2))), 1 / 2)


def _match_torch(x, ms, ss):
    st, mt = torch.std_mean(x, dim=0)
    return torch.sum(torch.square(ms - mt)) + torch.sum(torch.square(ss - st))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_correntropy_loss_against_float64(n, d):
    g = torch.Generator().manual_seed(n * 7 + d)
    z = _strided(n, d, g).requires_grad_(True)
    y = torch.randint(0, d, (n,), generator=g).to(DEV)
    gl = torch.tensor(0.75, device=DEV)
    runs = []
    for _ in range(2):
        z.grad = None
        loss, w = ops.correntropy_loss(z, y)
        loss.backward(gl)
        runs.append((loss.detach().clone(), w.clone(), z.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    ref = {}
    for dt in (torch.float64, torch.float32):
        zz = z.detach().to(dt).requires_grad_(True)
        l_, w_ = _c_loss_torch(zz, y)
        l_.backward(gl.to(dt))
        ref[dt] = (l_.detach(), w_.detach(), zz.grad)
    for i, name in enumerate(("loss", "weight", "grad")):
        _close(runs[0][i], ref[torch.float32][i], ref[torch.float64][i], f"{name} n={n} d={d}")


def test_correntropy_labels_outside_the_logits_are_never_read():
    """A label >= C (what the reference's one_hot cannot encode) matches no column; no address is formed from it."""
    z = torch.randn(50, 4, device=DEV)
    y = torch.randint(0, 4, (50,), device=DEV)
    y[3], y[7] = 4, 10 ** 9
    loss, w = ops.correntropy_loss(z, y)
    d = (z - F.one_hot(y.clamp(max=4), 5)[:, :4].float()).pow(2).sum(1)
    torch.testing.assert_close(w, torch.exp(-d / 10), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_weighted_moments_against_float64(n, d):
    g = torch.Generator().manual_seed(n * 11 + d)
    x = _strided(n, d, g)
    w = (torch.rand(n, generator=g) * 0.9 + 0.1).to(DEV)
    runs = [ops.weighted_moments(x, w) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0)), "two runs differ"      # n = 1: NaN std
    f64 = _moments_torch(x.double(), w.double())
    f32 = _moments_torch(x, w)
    _close(runs[0][0], f32[0], f64[0], f"mean n={n} d={d}")
    if n == 1:
        # one row carries all the weight: 1 - sum w'^2 = 0 and the variance is exactly 0, so std is 0 / 0 -- NaN here.
        # The reference's lines give NaN, inf or a rounding residue depending on whether w (1 / w) rounds to 1
        assert torch.isnan(runs[0][1]).all()
        return
    _close(runs[0][1], f32[1], f64[1], f"std n={n} d={d}", slack=1e-5)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_std_mean_match_against_float64(n, d):
    g = torch.Generator().manual_seed(n * 13 + d)
    x = _strided(n, d, g).requires_grad_(True)
    if n > 1:
        x.data[:, 0] = 0.25                          # a constant column: std_t = 0, torch masks its std gradient
    ms = (torch.randn(d, generator=g) * 0.2).to(DEV)
    ss = (torch.rand(d, generator=g) + 0.5).to(DEV)
    gl = torch.tensor(1.5, device=DEV)
    runs = []
    for _ in range(2):
        x.grad = None
        loss = ops.std_mean_match(x, ms, ss)
        loss.backward(gl)
        runs.append((loss.detach().clone(), x.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0)), "two runs differ"
    ref = {}
    for dt in (torch.float64, torch.float32):
        xx = x.detach().to(dt).requires_grad_(True)
        l_ = _match_torch(xx, ms.to(dt), ss.to(dt))
        l_.backward(gl.to(dt))
        ref[dt] = (l_.detach(), xx.grad)
    _close(runs[0][0], ref[torch.float32][0], ref[torch.float64][0], f"loss n={n} d={d}", slack=1e-5)
    _close(runs[0][1], ref[torch.float32][1], ref[torch.float64][1], f"grad n={n} d={d}", slack=1e-5)


# ------------------------------------------------------------------------------------------ trainer --
def _node_pair(g):
    s = Data(x=T(g["src_x"]), edge_index=T(g["src_ei"]), y=T(g["src_y"]))
    t = Data(x=T(g["tgt_x"]), edge_index=T(g["tgt_ei"]), y=T(g["tgt_y"]))
    return s, t


def _graphs(g, prefix):
    out = []
    for i in range(int(g[f"{prefix}/count"])):
        out.append(Data(x=T(g[f"{prefix}/{i}/x"]), edge_index=T(g[f"{prefix}/{i}/ei"]), y=T(g[f"{prefix}/{i}/y"])))
    return out


def _fit(name, captured):
    g = load_golden(name)
    graph = name.startswith("cwgcn_graph")
    if graph:
        s, t = _graphs(g, "src"), _graphs(g, "tgt")
        kw = dict(in_dim=10, hid_dim=8, num_classes=2, mode='graph', batch_size=int(g["batch_size"]))
        kw["gnn"] = "gcn"
    else:
        s, t = _node_pair(g)
        gnn = name.rsplit("_", 1)[1]
        kw = dict(in_dim=12, hid_dim=8, num_classes=3, gnn="gcn" if gnn == "mb" else gnn,
                  batch_size=int(g["batch_size"]) if "batch_size" in g else 0)
    m = pygda_amd.models.CWGCN(lr=0.01, weight_decay=0.001, device=DEV, epoch=3, verbose=0, use_hip_graph=captured,
                               **kw)
    log, cls_stage1 = [], {}
    m.epoch_hook = lambda e, loss, acc, secs: log.append((loss, acc))
    stage = m._stage

    def stage_rec(loader, optimizer, step, *a):
        if m.stage == 2:
            cls_stage1.update({k: v.detach().clone() for k, v in m.gnn.state_dict().items()})
        return stage(loader, optimizer, step, *a)

    m._stage = stage_rec
    torch.manual_seed(int(g["seed"]))
    m.fit(s, t)
    torch.cuda.synchronize()
    return g, m, log, cls_stage1


NODE_FULL = ["cwgcn_fit3_gcn", "cwgcn_fit3_sage", "cwgcn_fit3_gat", "cwgcn_fit3_gin"]


def _check_golden(g, m, log, cls_stage1, predict=True):
    losses, accs = np.array([l for l, _ in log]), np.array([a for _, a in log])
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(accs, g["accs"], atol=0.035)
    for prefix, sd in (("stage1/", cls_stage1), ("final/", m.gnn.state_dict())):
        for k, v in sd.items():
            np.testing.assert_allclose(v.cpu().numpy(), g[prefix + k], rtol=2e-3, atol=2e-4, err_msg=prefix + k)
    np.testing.assert_allclose(m.src_stats[0].cpu().numpy(), g["mean_s"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(m.src_stats[1].cpu().numpy(), g["std_s"], rtol=2e-3, atol=2e-4)
    np.testing.assert_array_equal(np.array([p.requires_grad for p in m.gnn.parameters()]), g["requires_grad"])
    if predict:
        for side in ("tgt", "src"):
            logits, labels = m.predict(None, source=side == "src", reference_compat=True)
            np.testing.assert_allclose(logits.cpu().numpy(), g[f"{side}_logits"], rtol=2e-3, atol=2e-3)
            np.testing.assert_array_equal(labels.cpu().numpy(), g[f"{side}_labels"])
    for k, v in m.gnn.state_dict().items():        # the classifier is outside the stage-2 loss: bit-identical
        if k.startswith("cls."):
            assert torch.equal(v, cls_stage1[k]), k


@pytest.mark.parametrize("name", NODE_FULL)
def test_full_batch_fit_matches_the_reference_eager_and_captured_bit_identical(name):
    g, me, loge, cls_e = _fit(name, False)
    _check_golden(g, me, loge, cls_e)
    g, mc, logc, cls_c = _fit(name, True)
    assert mc._graphed is None and loge == logc, (loge, logc)
    for (k, a), b in zip(me.gnn.state_dict().items(), mc.gnn.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(me.src_stats[0], mc.src_stats[0]) and torch.equal(me.src_stats[1], mc.src_stats[1])


def test_captured_fit_replays_several_steps_per_launch(monkeypatch):
    """PYGDA_AMD_GRAPH_UNROLL=4 without an epoch hook: the six stage-1 steps run as one 4-step replay and two single
    steps; the last step's source statistics are still the ones stage 2 needs."""
    monkeypatch.setenv("PYGDA_AMD_GRAPH_UNROLL", "4")
    g, me, _, _ = _fit("cwgcn_fit3_gcn", False)
    m = pygda_amd.models.CWGCN(12, 8, 3, lr=0.01, weight_decay=0.001, device=DEV, epoch=3, verbose=0, use_hip_graph=True)
    s, t = _node_pair(g)
    torch.manual_seed(int(g["seed"]))
    m.fit(s, t)
    torch.cuda.synchronize()
    for (k, a), b in zip(me.gnn.state_dict().items(), m.gnn.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(me.src_stats[1], m.src_stats[1])


@pytest.mark.parametrize("name", ["cwgcn_fit3_mb", "cwgcn_graph_fit3_b0", "cwgcn_graph_fit3_b6"])
def test_minibatch_and_graph_mode_fit_match_the_reference(name):
    g, m, log, cls1 = _fit(name, None)
    _check_golden(g, m, log, cls1, predict=name != "cwgcn_graph_fit3_b6")


# ------------------------------------------------------------------------------------------ full size --
def _gcn64(x, ei, w, b, dt):
    """PyG GCNConv in dtype dt: x W^T, self loops, degree over the destination, symmetric weights, + b."""
    n = x.size(0)
    loop = torch.arange(n)
    row, col = torch.cat([ei[0], loop]), torch.cat([ei[1], loop])
    deg = torch.zeros(n, dtype=dt).index_add_(0, col, torch.ones(col.numel(), dtype=dt))
    dis = deg.pow(-0.5)
    h = x @ w.t()
    return torch.zeros(n, h.size(1), dtype=dt).index_add_(0, col, h[row] * (dis[row] * dis[col])[:, None]) + b


def _restate(net, init, data, dt, stage, stats=None):
    P = {k: v.cpu().to(dt).requires_grad_(True) for k, v in init.items()}
    x, ei = data.x.cpu().to(dt), data.edge_index.cpu()
    h0 = torch.relu(_gcn64(x, ei, P["convs.0.lin.weight"], P["convs.0.bias"], dt))
    h1 = _gcn64(h0, ei, P["convs.1.lin.weight"], P["convs.1.bias"], dt)
    if stage == 1:
        z = _gcn64(h1, ei, P["cls.lin.weight"], P["cls.bias"], dt)
        loss, w = _c_loss_torch(z, data.y.cpu())
        extra = _moments_torch(h1.detach(), w.detach())
    else:
        loss = _match_torch(h1, stats[0].cpu().to(dt), stats[1].cpu().to(dt))
        extra = None
    loss.backward()
    return loss.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items()}, extra


def test_one_full_size_step_of_each_stage_against_float64():
    """DBLPv7 -> Citationv1 shapes (5484 / 8935 nodes, 6775 features, hid 128, 5 classes): one stage-1 step (loss,
    every gradient, the weighted source moments) and one stage-2 step (loss, every gradient), from the same weights."""
    from bench import make_cfg_a
    src, tgt = make_cfg_a(seed=7, ns=5484, es=8117, nt=8935, et=15098)
    src, tgt = src.to(DEV), tgt.to(DEV)
    m = pygda_amd.models.CWGCN(src.x.size(1), 128, 5, device=DEV, epoch=1, verbose=0)
    torch.manual_seed(0)
    m.gnn = m.init_model()
    m.gnn.train()
    init = {k: v.detach().clone() for k, v in m.gnn.named_parameters()}
    loss, _, w, xl = m.forward_model(src)
    loss.backward()
    stats = ops.weighted_moments(xl[1], w)
    res = {dt: _restate(m.gnn, init, src, dt, 1) for dt in (torch.float64, torch.float32)}
    _close(loss, res[torch.float32][0], res[torch.float64][0], "stage-1 loss", 1e-6)
    for k, p in m.gnn.named_parameters():
        _close(p.grad, res[torch.float32][1][k], res[torch.float64][1][k], "stage-1 grad " + k, 1e-5)
    _close(stats[0], res[torch.float32][2][0], res[torch.float64][2][0], "mean_s", 1e-5)
    _close(stats[1], res[torch.float32][2][1], res[torch.float64][2][1], "std_s", 1e-5)
    m.gnn.zero_grad(set_to_none=True)
    logits, tl = m.gnn(tgt.x, tgt.edge_index)
    loss2 = ops.std_mean_match(tl[1], *stats)
    loss2.backward()
    res = {dt: _restate(m.gnn, init, tgt, dt, 2, stats) for dt in (torch.float64, torch.float32)}
    _close(loss2, res[torch.float32][0], res[torch.float64][0], "stage-2 loss", 1e-6)
    for k, p in m.gnn.named_parameters():
        if k.startswith("cls."):
            assert p.grad is None, k
            continue
        _close(p.grad, res[torch.float32][1][k], res[torch.float64][1][k], "stage-2 grad " + k, 1e-5)


def test_no_blas_product_on_the_cwgcn_path(monkeypatch):
    from bench import make_cfg_a
    src, tgt = make_cfg_a(seed=7, ns=5484, es=8117, nt=8935, et=15098)
    m = pygda_amd.models.CWGCN(src.x.size(1), 128, 5, device=DEV, epoch=2, verbose=0)
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
    m.predict(None)
    m.predict(None, source=True)
    torch.cuda.synchronize()
    assert calls == [], sorted(set(calls))
