"""SAGDA on the MI355X: the FAConv kernels (csrc/gda_faconv.hip) against float64, the reassociated SAGNN layer at the
cfg-A shapes against a float64 run in the reference's order, the trainer against the reference's fixtures (eager and
captured), one full-size step against a float64 restatement, and the absence of BLAS products on the path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import ops
from pygda_amd.data import Data
from pygda_amd.graph import build_csr
from pygda_amd.nn.sagda_base import SAGNN, faconv_graph
from tests.conftest import T, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGIT_ATOL = 1e-4
REL = 1e-4


def _bound_msg(gpu, f32, f64, name, slack=1e-7):
    """None when max|gpu - f64| <= 4 max|fp32 restatement - f64| + slack max|f64|, else the violation."""
    gpu, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                     for v in (gpu, f32, f64))
    e_gpu, e_ref = np.abs(gpu - f64).max(), np.abs(f32 - f64).max()
    lim = 4 * e_ref + slack * np.abs(f64).max()
    return None if e_gpu <= lim else f"{name}: |gpu - f64| = {e_gpu:.3e} > {lim:.3e} (fp32 restatement {e_ref:.3e})"


def _bound_ok(gpu, f32, f64, name, slack=1e-7):
    msg = _bound_msg(gpu, f32, f64, name, slack)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------ kernel --
def _graph_edges(kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "n1":
        return 1, torch.zeros(2, 0, dtype=torch.int64)
    if kind == "uniform":
        n = 700
        src, dst = torch.randint(0, n, (4000,), generator=g), torch.randint(0, n, (4000,), generator=g)
    elif kind == "powerlaw":            # a destination hub and a source hub of 600+ entries each, over a sparse rest
        n = 2000
        src, dst = torch.randint(0, n, (3000,), generator=g), torch.randint(0, n, (3000,), generator=g)
        others = torch.randperm(n - 2, generator=g)[:650] + 2
        src = torch.cat([src, others, torch.ones(650, dtype=torch.int64)])
        dst = torch.cat([dst, torch.zeros(650, dtype=torch.int64), others])
    elif kind == "loops_dups":
        n = 300
        src, dst = torch.randint(0, n, (1500,), generator=g), torch.randint(0, n, (1500,), generator=g)
        loops = torch.randint(0, n, (40,), generator=g)
        src, dst = torch.cat([src, src[:60], loops]), torch.cat([dst, dst[:60], loops])
    else:                               # isolated: the upper half of the nodes has no edge at all
        n = 400
        src, dst = torch.randint(0, n // 2, (900,), generator=g), torch.randint(0, n // 2, (900,), generator=g)
    perm = torch.randperm(src.numel(), generator=g)
    return n, torch.stack([src[perm], dst[perm]])


def _coo(graph):
    rp = graph.rowptr.cpu().long()
    nnz = int(rp[-1])
    row = torch.repeat_interleave(torch.arange(graph.num_nodes), rp[1:] - rp[:-1])
    return row, graph.colidx[:nnz].cpu().long(), graph.val[:nnz].cpu()


def _restate(h, s, r, row, col, w, eps, bias):
    t = torch.tanh(s[col] + r[row])
    msg = h[col] * (t * w).unsqueeze(1)
    return torch.zeros_like(h).index_add_(0, row, msg) + eps * h + bias


@pytest.mark.parametrize("kind", ["uniform", "powerlaw", "loops_dups", "isolated", "n1"])
@pytest.mark.parametrize("d", [1, 3, 8, 64, 128, 130, 256])
def test_faconv_kernels_against_float64(kind, d):
    n, ei = _graph_edges(kind, 7 + d)
    graph = build_csr(ei.to(DEV), n, None, False, True, True, "col", with_edge_map=True)
    row, col, w = _coo(graph)
    if kind == "powerlaw":
        deg = torch.bincount(row, minlength=n)
        assert deg.max() > 500 and torch.bincount(col, minlength=n).max() > 500
    g = torch.Generator().manual_seed(100 + d)
    h0, s0, r0 = torch.randn(n, d, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    b0, gout = torch.randn(d, generator=g), torch.randn(n, d, generator=g)
    res = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        h, s, r, b = (v.to(dt).clone().requires_grad_(True) for v in (h0, s0, r0, b0))
        out = _restate(h, s, r, row, col, w.to(dt), 0.1, b)
        out.backward(gout.to(dt))
        res[name] = (out, h.grad, s.grad, r.grad, b.grad)

    def run():
        h, s, r, b = (v.to(DEV).requires_grad_(True) for v in (h0, s0, r0, b0))
        out = ops.faconv_aggregate(h, s, r, graph, 0.1, b)
        out.backward(gout.to(DEV))
        return out.detach(), h.grad, s.grad, r.grad, b.grad

    a, a2 = run(), run()
    for name, x, y, f32, f64 in zip(("out", "gh", "gs", "gr", "gb"), a, a2, res["f32"], res["f64"]):
        assert torch.equal(x, y), f"{name}: two runs differ"
        if name != "gb":              # the bias gradient is ops.colsum's (the caller's), not the FAConv kernels'
            _bound_ok(x, f32, f64, name)
    # the packed projection [h | s | r] takes the same kernels through row strides: same bits
    p = torch.cat([h0, s0[:, None], r0[:, None]], 1).to(DEV).requires_grad_(True)
    out = ops.faconv_aggregate_packed(p, d, graph, 0.1, b0.to(DEV))
    out.backward(gout.to(DEV))
    assert torch.equal(out, a[0])
    assert torch.equal(p.grad[:, :d], a[1]) and torch.equal(p.grad[:, d], a[2]) and torch.equal(p.grad[:, d + 1], a[3])


# ------------------------------------------------------------------------------- reassociation --
def _fa_weights(ei, n, dt):
    """gcn_norm of FAConv (remaining self loops, fill 1, destination degree) restated for a loop-free edge list."""
    loops = torch.arange(n)
    row, col = torch.cat([ei[1], loops]), torch.cat([ei[0], loops])
    deg = torch.bincount(row, minlength=n).to(dt)
    dis = deg.pow(-0.5)
    return row, col, dis[col] * dis[row]


def test_sagnn_layer0_reassociation_against_reference_order():
    """SAGNN layer 0 on the cfg-A source (sparse bag-of-words input): output and the gradients of W, b, att_l, att_r
    within 4x of the fp32 REFERENCE-ORDER run's distance from float64 (FAConv over the 6,775-wide rows, then the
    product) -- the reassociation moves the rounding, not the result."""
    from bench import make_cfg_a
    src, _ = make_cfg_a()
    n, F_ = src.x.shape
    torch.manual_seed(5)
    layer = SAGNN(F_, 128, 1.0, 1.0)
    with torch.no_grad():
        layer.bias.uniform_(-0.1, 0.1)
    init = {k: v.detach().clone() for k, v in layer.named_parameters()}
    gout = torch.randn(n, 128, generator=torch.Generator().manual_seed(6))
    s = src.to(DEV)
    layer = layer.to(DEV)
    out = layer(s.x, s.edge_index)
    out.backward(gout.to(DEV))
    got = dict(out=out, W=layer.weight.grad, b=layer.bias.grad, att_l=layer.conv.att_l.weight.grad,
               att_r=layer.conv.att_r.weight.grad)
    ei = src.edge_index
    res = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        dev = DEV
        x = src.x.to(dev, dt)
        W, b, al, ar = (init[k].to(dev, dt).requires_grad_(True) for k in ("weight", "bias", "conv.att_l.weight",
                                                                             "conv.att_r.weight"))
        row, col, w = (v.to(dev) for v in _fa_weights(ei, n, dt))
        sl, sr = x @ al.t(), x @ ar.t()
        coef = torch.tanh(sl[col, 0] + sr[row, 0]) * w
        z = torch.zeros_like(x)
        for c0 in range(0, row.numel(), 4096):               # F-wide messages in chunks of edges
            sel = slice(c0, c0 + 4096)
            z.index_add_(0, row[sel], x[col[sel]] * coef[sel, None])
        z = z + 0.1 * x
        y = z @ W + b
        y.backward(gout.to(dev, dt))
        res[name] = dict(out=y, W=W.grad, b=b.grad, att_l=al.grad, att_r=ar.grad)
        del x, z
    for k in got:
        _bound_ok(got[k], res["f32"][k], res["f64"][k], k, slack=0.0)


# ---------------------------------------------------------------------------------- trainer goldens --
def _pair(g):
    s = Data(x=T(g["src_x"]), edge_index=T(g["src_ei"]), y=T(g["src_y"]))
    t = Data(x=T(g["tgt_x"]), edge_index=T(g["tgt_ei"]), y=T(g["tgt_y"]))
    return s, t


def _no_dropout(module):
    for m in module.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        for d in getattr(m, "dropout_layers", []):
            d.p = 0.0


def _fit_golden(monkeypatch, layers, graphed):
    g = load_golden(f"sagda_fit3_l{layers}")
    s, t = _pair(g)
    m = pygda_amd.models.SAGDA(12, 8, 3, num_layers=layers, ppmi=True, adv_dim=6, lr=0.01, weight_decay=0.003,
                               device=DEV, epoch=3, verbose=0, use_hip_graph=graphed)
    init = m.init_model

    def init_with_reference_ppmi(**kw):
        net = init(**kw)
        _no_dropout(net)
        for li, conv in enumerate(net.ppmi_encoder.conv_layers):
            ei, w = T(g[f"ppmi/target/{li}/edge_index"], DEV), T(g[f"ppmi/target/{li}/weight"], DEV)
            conv.cache_dict["target"] = build_csr(ei, t.num_nodes, w, add_self_loops=False, normalize=False)
        return net

    monkeypatch.setattr(m, "init_model", init_with_reference_ppmi)
    seen = []
    m.epoch_hook = lambda e, loss, acc, secs: seen.append((loss, acc))
    torch.manual_seed(int(g["seed"]))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(s, t)
    return g, m, seen


@pytest.mark.parametrize("layers", [1, 2])
def test_sagda_fit_predict_golden_eager_and_captured(monkeypatch, layers):
    runs = {}
    for graphed in (False, True):
        g, m, seen = _fit_golden(monkeypatch, layers, graphed)
        assert (getattr(m, "_graphed", None) is not None) == graphed, "the captured step did not replay"
        np.testing.assert_allclose([x[0] for x in seen], g["losses"], rtol=REL)
        np.testing.assert_array_equal([x[1] for x in seen], g["accs"])
        logits, labels = m.predict(None)
        slogits, slabels = m.predict(None, source=True)
        for got, lab, key in ((logits, labels, "tgt"), (slogits, slabels, "src")):
            np.testing.assert_allclose(got.cpu().numpy(), g[f"{key}_logits"], rtol=0, atol=LOGIT_ATOL)
            np.testing.assert_array_equal(lab.cpu().numpy(), g[f"{key}_labels"])
            np.testing.assert_array_equal(got.argmax(1).cpu().numpy(), g[f"{key}_logits"].argmax(1))
        runs[graphed] = ([x[0] for x in seen], logits, slogits)
    assert runs[False][0] == runs[True][0]
    assert torch.equal(runs[False][1], runs[True][1]) and torch.equal(runs[False][2], runs[True][2])


# ---------------------------------------------------------------------------------- full size --
class _Grl(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha):
        ctx.alpha = alpha
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.neg() * ctx.alpha, None


def _full_size_model(monkeypatch, layers=2):
    from bench import make_cfg_a
    src, tgt = make_cfg_a()
    m = pygda_amd.models.SAGDA(src.x.size(1), 128, 5, num_layers=layers, adv_dim=40, device=DEV, epoch=1, verbose=0,
                               use_hip_graph=False)
    init = m.init_model
    keep = {}

    def init_no_dropout(**kw):
        net = init(**kw)
        _no_dropout(net)
        keep["init"] = {id(p): p.detach().clone() for p in net.parameters()}
        return net

    monkeypatch.setattr(m, "init_model", init_no_dropout)
    seen = []
    m.epoch_hook = lambda e, loss, acc, secs: seen.append(loss)
    return m, src, tgt, keep, seen


def _restate_step(m, src, tgt, init, dt, layers):
    """The SAGDA step (sagda.py:262-312, epoch 0 of 1, Dropouts zeroed) on the host in dtype ``dt``: the loss and the
    gradients by autograd."""
    net = m.sagda
    P = {id(p): init[id(p)].cpu().to(dt).requires_grad_(True) for p in net.parameters()}
    q = lambda p: P[id(p)]                                                                  # noqa: E731

    def prop(graph, x):
        row, col, w = _coo(graph)
        return torch.zeros(x.size(0), x.size(1), dtype=dt).index_add_(0, row, x[col] * w.to(dt)[:, None])

    xt, xs = tgt.x.to(dt), src.x.to(dt)
    views = []
    for enc in (net.encoder, net.ppmi_encoder):
        x = xt
        for i, conv in enumerate(enc.conv_layers):
            x = prop(conv.cache_dict["target"], x @ q(conv.weight)) + q(conv.bias)
            if i < layers - 1:
                x = torch.relu(x)
        views.append(x)
    st = torch.stack(views, 1)
    att = net.att_model.dense_weight
    et = (st * torch.softmax(st @ q(att.weight).t() + q(att.bias), dim=1)).sum(1)
    row, col, w = _fa_weights(src.edge_index, xs.size(0), dt)
    x = xs
    for sg in net.src_encoder.conv_layers:
        h, sl, sr = x @ q(sg.weight), x @ q(sg.conv.att_l.weight).t(), x @ q(sg.conv.att_r.weight).t()
        coef = torch.tanh(sl[col, 0] + sr[row, 0]) * w
        x = torch.zeros_like(h).index_add_(0, row, h[col] * coef[:, None]) + 0.1 * h + q(sg.bias)
    es = x
    cls, dm = net.cls_model[0], net.domain_model
    logits_s = es @ q(cls.weight).t() + q(cls.bias)
    disc = lambda e: torch.relu(e @ q(dm[0].weight).t() + q(dm[0].bias)) @ q(dm[3].weight).t() + q(dm[3].bias)  # noqa
    alpha = min(1 / m.epoch, 0.05)
    ds, dtg = disc(_Grl.apply(es, alpha)), disc(_Grl.apply(et, alpha))
    loss = F.cross_entropy(logits_s, src.y) + F.cross_entropy(ds, torch.zeros(ds.size(0), dtype=torch.long)) \
        + F.cross_entropy(dtg, torch.ones(dtg.size(0), dtype=torch.long))
    p = torch.softmax(et @ q(cls.weight).t() + q(cls.bias), 1).clamp(min=1e-9, max=1.0)
    loss = loss + torch.mean(torch.sum(-p * torch.log(p), 1)) * (0 / m.epoch * 0.01)
    loss.backward()
    return loss.detach(), {k: v.grad.clone() for k, v in P.items()}


def _restate_adam(m, init, grads, dt):
    """torch's per-tensor Adam (sagda.py:251) over the optimiser's listing -- itertools.chain of the six models, the
    shared conv weights and biases three times, each listing updated after the previous one -- in dtype ``dt``."""
    P = {k: v.detach().cpu().to(dt).clone() for k, v in init.items()}
    state = {}
    lr, wd, b1, b2, eps = m.lr, m.weight_decay, 0.9, 0.999, 1e-8
    for mod in m.sagda.models:
        for prm in mod.parameters():
            v = P[id(prm)]
            st = state.setdefault(id(prm), [0, torch.zeros_like(v), torch.zeros_like(v)])
            st[0] += 1
            stp, ea, eq = st
            gr = grads[id(prm)].cpu().to(dt) + wd * v
            ea.mul_(b1).add_(gr, alpha=1 - b1)
            eq.mul_(b2).addcmul_(gr, gr, value=1 - b2)
            denom = (eq.sqrt() / (1 - b2 ** stp) ** 0.5).add_(eps)
            v.addcdiv_(ea, denom, value=-lr / (1 - b1 ** stp))
    return P


def test_sagda_full_size_step_against_float64(monkeypatch):
    layers = 2
    m, src, tgt, keep, seen = _full_size_model(monkeypatch, layers)
    torch.manual_seed(0)
    np.random.seed(0)
    m.fit(src, tgt)
    torch.cuda.synchronize()
    names = {id(p): n for n, p in m.sagda.named_parameters()}
    res = {dt: _restate_step(m, src, tgt, keep["init"], dt, layers) for dt in (torch.float64, torch.float32)}
    f64, f32 = res[torch.float64], res[torch.float32]
    # slack: 8 fp32 ulps of the largest magnitude -- the bias gradients are column sums over 10^4 rows, whose order the
    # host restatement (torch's vectorised CPU sums) cannot mirror
    bad = [_bound_msg(np.array([seen[0]]), f32[0].double().numpy()[None], f64[0].numpy()[None], "loss", 1e-6)]
    for p in m.sagda.parameters():
        bad.append(_bound_msg(p.grad, f32[1][id(p)], f64[1][id(p)], "grad " + names[id(p)], 1e-6))
    # the update on the device's own gradients: Adam's 1 / (sqrt(v) + eps) amplifies a gradient's last bits a
    # thousandfold where |g| ~ eps, so the three rounds on the shared weights are checked on the same inputs
    after = {dt: _restate_adam(m, keep["init"], {id(p): p.grad for p in m.sagda.parameters()}, dt)
             for dt in (torch.float64, torch.float32)}
    for p in m.sagda.parameters():
        bad.append(_bound_msg(p.detach(), after[torch.float32][id(p)], after[torch.float64][id(p)],
                              "param " + names[id(p)], 1e-6))
    bad = [b for b in bad if b is not None]
    assert not bad, "\n".join(bad)


def test_no_blas_product_on_the_sagda_path(monkeypatch):
    m, src, tgt, keep, seen = _full_size_model(monkeypatch)
    m.use_hip_graph = None
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
