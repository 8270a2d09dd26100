"""SEPA on the MI355X: the fused prototype term of csrc/gda_sepa.hip (forward and every input gradient) against the
float64 composition of the host lines at four shapes, one with an unpredicted class; the class-grouped mean, the
prototype kernel and ``ops.ppr`` on their own; 3-epoch fits against the fixtures recorded from the reference's own
sepa.py, bounded by its float64 run, with the recorded arg-max; eager and captured fits bit-identical; no BLAS product
on the path; two epochs at the ACMv9 -> DBLPv7 stand-in shapes."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import ops
from pygda_amd.data import Data
from pygda_amd.graph import as_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ("sepa_fit3_gcn.npz", "sepa_fit3_gat.npz", "sepa_fit3_gin_empty.npz")
LAM = dict(lamda_im=0.2, lamda_pp=0.1, lamda_sep=1.0, tau=1.5)


def _close(gpu, f32, f64, name, slack=2e-6):
    """|gpu - f64| <= 8 |fp32 torch - f64| + slack max|f64|."""
    gpu, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                     for v in (gpu, f32, f64))
    e_gpu, e_ref = np.abs(gpu - f64).max(), np.abs(f32 - f64).max()
    lim = 8 * e_ref + slack * max(np.abs(f64).max(), 1e-30)
    print(f"{name}: |gpu - f64| = {e_gpu:.3e}, |fp32 torch - f64| = {e_ref:.3e}, bound {lim:.3e}")
    assert e_gpu <= lim, f"{name}: |gpu - f64| = {e_gpu:.3e} > {lim:.3e} (fp32 torch {e_ref:.3e})"


def _edges(n, seed):
    """Directed random edges with duplicates, a self loop and an isolated node (node 1)."""
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n, (3 * n,), generator=g), torch.randint(0, n, (3 * n,), generator=g)
    keep = (src != 1) & (dst != 1)
    src, dst = src[keep], dst[keep]
    src = torch.cat([src, src[:3], torch.tensor([0, n - 1])])
    dst = torch.cat([dst, dst[:3], torch.tensor([0, 2])])
    return torch.stack([src, dst])


def _inputs(n, h, c, empty, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, c, generator=g, dtype=torch.float64)
    if empty:
        z[:, c - 1] -= 10.0                                        # the last class is predicted by no node
    z[torch.arange(n), z.argmax(1)] += 0.5                         # every node well inside its class
    ns = n + 37
    ys = torch.randint(0, c, (ns,), generator=g)
    ys[:c] = torch.arange(c)
    return (z, 0.5 * torch.randn(n, h, generator=g, dtype=torch.float64),
            torch.randn(ns, h, generator=g, dtype=torch.float64), ys, _edges(n, seed + 1))


def _host_term(z, f, fs, ys, ei, c, dtype):
    m = pygda_amd.models.SEPA(f.size(1), f.size(1), c, device="cpu", **LAM)
    z, f, fs = (v.to(dtype).requires_grad_(True) for v in (z, f, fs))
    prob = F.softmax(z, dim=1)
    im, _, _, ent = m.cls_im(prob)
    sp = m.obtain_source_prototype(fs, ys)
    pp = m.proto_alignment(m.obtain_target_prototype(prob, f, ei, ent), sp)
    sep = m.seperate_center(sp, fs, ys)
    total = LAM["lamda_im"] * im + LAM["lamda_pp"] * pp + LAM["lamda_sep"] * sep
    grads = torch.autograd.grad(total, (z, f, fs))
    return total.detach(), torch.stack([im, pp, sep]).detach(), grads, prob.detach()


@pytest.mark.parametrize("n,h,c,empty", [(260, 16, 3, False), (1037, 48, 7, True), (5484, 128, 5, False),
                                         (4099, 1024, 32, False)])
def test_fused_term_against_float64(n, h, c, empty):
    z, f, fs, ys, ei = _inputs(n, h, c, empty, 100 + n)
    t64, p64, g64, prob = _host_term(z, f, fs, ys, ei, c, torch.float64)
    top = prob.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 1e-3
    assert (torch.unique(prob.argmax(1)).numel() < c) == empty
    t32, p32, g32, _ = _host_term(z, f, fs, ys, ei, c, torch.float32)
    zd, fd, fsd = (v.float().to(DEV).requires_grad_(True) for v in (z, f, fs))
    graph = as_graph(ei.to(DEV), n, None, False, True, True, "col")
    total, parts, pred = ops.sepa_term(zd, fd, fsd, ys.to(DEV, torch.int32), graph, LAM["lamda_im"], LAM["lamda_pp"],
                                       LAM["lamda_sep"], LAM["tau"])
    grads = torch.autograd.grad(total, (zd, fd, fsd))
    assert torch.equal(pred.cpu().long(), prob.argmax(1))
    _close(total, t32, t64, "total")
    _close(parts, p32, p64, "parts")
    for name, a, b, d in zip(("dZ", "dF", "dFs"), grads, g32, g64):
        _close(a, b, d, name)
    total2, _, _ = ops.sepa_term(zd, fd, fsd, ys.to(DEV, torch.int32), graph, LAM["lamda_im"], LAM["lamda_pp"],
                                 LAM["lamda_sep"], LAM["tau"])
    again = torch.autograd.grad(total2, (zd, fd, fsd))
    assert torch.equal(total, total2) and all(torch.equal(a, b) for a, b in zip(grads, again))


@pytest.mark.parametrize("n,d,c", [(260, 16, 3), (1037, 7, 2), (4099, 1024, 32)])
def test_class_mean_and_loss_methods_on_device_tensors(n, d, c):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    idx = torch.randint(0, c, (n,), generator=g)
    up = torch.randn(c, d, generator=g, dtype=torch.float64)
    t = torch.randn(c, d, generator=g, dtype=torch.float64)

    def run(dtype, dev):
        m = pygda_amd.models.SEPA(d, d, c, device=dev, **LAM)
        xx, tt = x.to(dev, dtype).requires_grad_(True), t.to(dev, dtype).requires_grad_(True)
        proto = m.obtain_source_prototype(xx, idx.to(dev))
        val = (proto * up.to(dev, dtype)).sum() + m.proto_alignment(tt, proto) + m.seperate_center(proto, xx, None)
        return (val.detach(),) + torch.autograd.grad(val, (xx, tt))

    r64, r32, rg = run(torch.float64, "cpu"), run(torch.float32, "cpu"), run(torch.float32, DEV)
    for name, a, b, e in zip(("value", "dx", "dT"), rg, r32, r64):
        _close(a, b, e, name)


def test_ppr_uses_the_transposed_csr_backward():
    n, d, k, alpha = 300, 20, 5, 0.9
    ei = _edges(n, 5)
    x = torch.randn(n, d, dtype=torch.float64)
    up = torch.randn(n, d, dtype=torch.float64)

    def host(dtype):
        from pygda_amd.nn.pagerank import host_gcn_graph
        row, col, norm = host_gcn_graph(ei, n, dtype)
        x0 = x.to(dtype).requires_grad_(True)
        cur = x0
        for _ in range(k):
            cur = (1 - alpha) * torch.zeros(n, d, dtype=dtype).index_add_(0, col, norm[:, None] * cur[row]) + alpha * x0
        return cur.detach(), torch.autograd.grad((cur * up.to(dtype)).sum(), x0)[0]

    (o64, g64), (o32, g32) = host(torch.float64), host(torch.float32)
    xd = x.float().to(DEV).requires_grad_(True)
    pr = pygda_amd.nn.PageRank()
    assert (pr.k, pr.alpha) == (5, 0.9)
    out = pr(xd, ei.to(DEV))
    (gd,) = torch.autograd.grad((out * up.float().to(DEV)).sum(), xd)
    _close(out, o32, o64, "ppr")
    _close(gd, g32, g64, "ppr backward")


def _fixture(name):
    f = np.load(os.path.join(HERE, name))
    s = Data(x=torch.from_numpy(f["src_x"]), edge_index=torch.from_numpy(f["src_ei"]), y=torch.from_numpy(f["src_y"]))
    t = Data(x=torch.from_numpy(f["tgt_x"]), edge_index=torch.from_numpy(f["tgt_ei"]), y=torch.from_numpy(f["tgt_y"]))
    return f, s, t


def _fit(f, s, t, epochs=3, **kw):
    m = pygda_amd.models.SEPA(16, 16, int(f["num_classes"]), num_layers=2, lr=4e-3, gnn=str(f["gnn"]), device=DEV,
                              epoch=epochs, verbose=0, record=True, **kw)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    torch.manual_seed(int(f["init_seed"]))
    m.fit(s, t)
    return m, log


@pytest.mark.parametrize("name", FIXTURES)
def test_fit3_against_the_reference_bounded_by_its_float64_run(name):
    f, s, t = _fixture(name)
    m, log = _fit(f, s, t)
    for p, q in zip(m.pred_log, f["pred"]):
        assert (p.numpy() == q).all()
    _close(np.array([l for l, _ in log]), f["losses"], f["f64/losses"], "losses", 1e-5)
    _close(np.array(m.parts_log), f["parts"], f["f64/parts"], "parts", 1e-5)
    for k, v in m.gnn.state_dict().items():
        _close(v, f["final/" + k], f["f64/final/" + k], k, 1e-4)
    for data, key in ((s, "src_logits"), (t, "tgt_logits")):
        lo, _ = m.predict(data)
        _close(lo, f[key], f["f64/" + key], key, 1e-4)


def test_eager_and_captured_fits_are_bit_identical():
    f, s, t = _fixture("sepa_fit3_gin_empty.npz")

    def run(graph):
        m, log = _fit(f, s, t, epochs=7, use_hip_graph=graph, epochs_per_graph=3)
        lo, _ = m.predict(t)
        return log, lo, [p.detach().clone() for p in m.gnn.parameters()]

    le, oe, pe = run(False)
    lc, oc, pc = run(True)
    lc2, oc2, pc2 = run(True)
    assert len(le) == 7 and le == lc and lc == lc2
    assert torch.equal(oe, oc) and all(torch.equal(a, b) for a, b in zip(pe, pc))
    assert torch.equal(oc, oc2) and all(torch.equal(a, b) for a, b in zip(pc, pc2))


def test_no_blas_product_on_the_sepa_path(monkeypatch):
    f, s, t = _fixture("sepa_fit3_gcn.npz")
    calls = []

    def spy(name, fn):
        def wrapped(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapped

    for owner, attr in ((torch, "mm"), (torch, "matmul"), (torch.Tensor, "mm"), (torch.Tensor, "__matmul__"),
                        (F, "linear")):
        monkeypatch.setattr(owner, attr, spy(attr, getattr(owner, attr)))
    m, _ = _fit(f, s, t, epochs=5)
    m.predict(t)
    torch.cuda.synchronize()
    assert calls == [], sorted(set(calls))


@pytest.mark.parametrize("gnn", ["gcn", "gat"])
def test_two_epochs_at_the_acm_dblp_shapes(gnn):
    from bench import make_cfg_a
    src, tgt = make_cfg_a()
    m = pygda_amd.models.SEPA(src.x.size(1), 128, 5, gnn=gnn, device=DEV, epoch=2, verbose=0)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    m.fit(src, tgt)
    logits, _ = m.predict(tgt)
    assert len(log) == 2 and all(np.isfinite(v) for v in log)
    assert logits.shape == (5484, 5) and torch.isfinite(logits).all()
