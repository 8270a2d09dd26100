"""ASN on the MI355X: the kernels of csrc/gda_asn.hip against float64 -- the all-pairs reconstruction loss and its
gradient up to N = 9,360 at K in {2, 10, 33, 128} on graphs with duplicate edges, self loops, directed edges and
isolated nodes; KLD, DiffLoss, the reparameterisation and the normalised PPMI graph -- two runs bit-identical, the
3-epoch fit against the host restatement of the reference (given noise, dropout off), one full-size epoch at the
ACMv9 -> DBLPv7 shapes without an N x N buffer, and no BLAS product on the path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import ops
from pygda_amd.data import Data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(gpu, f32, f64, name, slack=2e-6):
    """|gpu - f64| <= 8 |fp32 torch - f64| + slack max|f64|."""
    gpu, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                     for v in (gpu, f32, f64))
    e_gpu, e_ref = np.abs(gpu - f64).max(), np.abs(f32 - f64).max()
    lim = 8 * e_ref + slack * max(np.abs(f64).max(), 1e-30)
    assert e_gpu <= lim, f"{name}: |gpu - f64| = {e_gpu:.3e} > {lim:.3e} (fp32 torch {e_ref:.3e})"


def _edges(n, seed):
    """Random directed edges with duplicates, a self loop, an isolated non-last node (when n > 2) and the last node
    touched (so that edge_index.max() + 1 == n)."""
    g = torch.Generator().manual_seed(seed)
    e = max(2 * n, 1)
    src, dst = torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    if n > 2:
        keep = (src != 1) & (dst != 1)                     # node 1 isolated
        src, dst = src[keep], dst[keep]
        src = torch.cat([src, src[:3], torch.tensor([0, n - 1, 2])])       # three duplicates, a self loop, a last node
        dst = torch.cat([dst, dst[:3], torch.tensor([0, 2, n - 1])])
    else:
        src, dst = torch.cat([src, torch.tensor([n - 1])]), torch.cat([dst, torch.tensor([n - 1])])
    return torch.stack([src, dst])


def _bce_ref(z, labels, dtype):
    z = z.detach().to(dtype).requires_grad_(True)
    y = labels.dense().to(DEV, dtype)
    x = z @ z.t()
    pw = labels.pos_weight
    f = (1 - y) * x + (1 + (pw - 1) * y) * (torch.log1p(torch.exp(-x.abs())) + torch.clamp(-x, min=0))
    loss = labels.norm * f.mean()
    (g,) = torch.autograd.grad(loss, z)
    return loss.detach(), g


@pytest.mark.parametrize("n", [1, 7, 130, 270, 1000, 9360])   # 270: ragged tiles, chunks of 3 and 2 column tiles
@pytest.mark.parametrize("k", [2, 10, 30, 33, 128])             # every padded width: 8, 16, 32, 64, 128
def test_recon_kernel_against_float64(n, k):
    ei = _edges(n, n + k).to(DEV)
    labels = ops.AsnLabels(ei, n)
    torch.manual_seed(n * 131 + k)
    z = (torch.randn(n, k, device=DEV) * (1.5 / k ** 0.5)).requires_grad_(True)
    loss = ops.asn_recon_loss(z, labels)
    (dz,) = torch.autograd.grad(loss, z)
    l64, g64 = _bce_ref(z, labels, torch.float64)
    l32, g32 = _bce_ref(z, labels, torch.float32)
    _close(loss, l32, l64, f"loss n={n} k={k}", 1e-5)
    _close(dz, g32, g64, f"dz n={n} k={k}", 1e-5)


def test_recon_kernel_two_runs_bit_identical_and_rejects_wide_k():
    n, k = 1000, 10
    labels = ops.AsnLabels(_edges(n, 3).to(DEV), n)
    z = torch.randn(n, k, device=DEV, requires_grad=True)
    a = torch.autograd.grad(ops.asn_recon_loss(z, labels), z)[0]
    la = ops.asn_recon_loss(z, labels).item()
    b = torch.autograd.grad(ops.asn_recon_loss(z, labels), z)[0]
    assert torch.equal(a, b) and la == ops.asn_recon_loss(z, labels).item()
    with pytest.raises(ValueError):
        ops.asn_recon_loss(torch.zeros(n, 129, device=DEV), labels)


@pytest.mark.parametrize("n,d", [(1, 4), (257, 20), (9360, 20)])
def test_kld_and_reparam_against_float64(n, d):
    torch.manual_seed(n + d)
    mu = torch.randn(n, d, device=DEV, requires_grad=True)
    lv = (0.3 * torch.randn(n, d, device=DEV)).requires_grad_(True)
    eps = torch.randn(n, d, device=DEV)
    out = ops.asn_kld(mu, lv, 2 * n) + (ops.asn_reparam(mu, lv, eps) ** 2).sum() * 1e-3
    gm, gl = torch.autograd.grad(out, [mu, lv])

    def ref(dtype):
        m, l = mu.detach().to(dtype).requires_grad_(True), lv.detach().to(dtype).requires_grad_(True)
        o = (-0.5 / (2 * n) * torch.mean(torch.sum(1 + 2 * l - m.pow(2) - l.exp().pow(2), 1))
             + ((eps.to(dtype) * l.exp() + m) ** 2).sum() * 1e-3)
        return (o.detach(), *torch.autograd.grad(o, [m, l]))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, a, b, name in zip((out, gm, gl), r32, r64, ("loss", "dmu", "dlogvar")):
        _close(got, a, b, name, 1e-5)
    z1 = ops.asn_reparam(mu.detach(), lv.detach())
    z2 = ops.asn_reparam(mu.detach(), lv.detach())
    assert torch.isfinite(z1).all() and not torch.equal(z1, z2)         # a fresh Philox draw per call site


@pytest.mark.parametrize("n,k1,k2", [(1, 5, 5), (300, 5, 5), (9360, 32, 7)])
def test_diff_loss_against_float64(n, k1, k2):
    torch.manual_seed(n)
    a = torch.randn(n, k1, device=DEV, requires_grad=True)
    b = torch.randn(n, k2, device=DEV, requires_grad=True)
    loss = ops.asn_diff_loss(a, b)
    ga, gb = torch.autograd.grad(loss, [a, b])

    def ref(dtype):
        x, y = a.detach().to(dtype).requires_grad_(True), b.detach().to(dtype).requires_grad_(True)
        o = ops._asn_diff_host(x, y)
        return (o.detach(), *torch.autograd.grad(o, [x, y]))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, x, y, name in zip((loss, ga, gb), r32, r64, ("loss", "ga", "gb")):
        _close(got, x, y, name, 1e-5)


@pytest.mark.parametrize("n", [9, 500])
def test_ppmi_graph_against_the_host_restatement(n):
    ei = _edges(n, 11)
    g = ops.asn_ppmi_graph(ei.to(DEV), n, 3)
    src, dst, w = _coo(g)
    dense = torch.zeros(n, n, dtype=torch.float64)
    dense[dst.cpu(), src.cpu()] = w.double().cpu()
    host = ops.asn_ppmi_graph(ei, n, 3).double()
    _ppmi_agree(dense, host)


def _ppmi_agree(dev, host):
    """Entries present on both sides agree closely; an entry may appear or vanish only where the PPMI sits at its
    ppmi < 0 threshold, i.e. where the other side's value is tiny."""
    both = (dev != 0) & (host != 0)
    assert torch.allclose(dev[both], host[both], rtol=1e-4, atol=1e-7), (dev[both] - host[both]).abs().max()
    flip = (dev != 0) ^ (host != 0)
    assert np.abs(dev[flip].numpy()).max(initial=0) < 1e-3 and np.abs(host[flip].numpy()).max(initial=0) < 1e-3


def test_ppmi_graph_against_the_reference_fixture():
    from tests.conftest import load_golden
    g = load_golden("asn_fit3")
    for dom, key in (("s", "src_ei"), ("t", "tgt_ei")):
        P = torch.sparse_csr_tensor(torch.from_numpy(g[f"ppmi_{dom}_crow"]), torch.from_numpy(g[f"ppmi_{dom}_col"]),
                                    torch.from_numpy(g[f"ppmi_{dom}_val"])).to_dense()
        n = P.size(0)
        gr = ops.asn_ppmi_graph(torch.from_numpy(g[key]).to(DEV), n, 3)
        src, dst, w = _coo(gr)
        dense = torch.zeros(n, n, dtype=torch.float64)
        dense[dst.cpu(), src.cpu()] = w.double().cpu()
        _ppmi_agree(dense, ops.asn_gcn_norm_sparse(P.double()))


def _coo(g):
    rp, ci, val = g.rowptr.long(), g.colidx.long(), g.val
    nnz = int(rp[-1])
    dst = torch.repeat_interleave(torch.arange(g.num_nodes, device=rp.device), rp[1:] - rp[:-1])
    return ci[:nnz], dst, val[:nnz]


def _pair(seed, ns=60, nt=45, f=20, c=3):
    def graph(n, s):
        gen = torch.Generator().manual_seed(s)
        return Data(x=torch.rand(n, f, generator=gen), edge_index=_edges(n, s), y=torch.randint(0, c, (n,), generator=gen))
    return graph(ns, seed), graph(nt, seed + 1)


class _NoDropASN(pygda_amd.models.ASN):
    def init_model(self, **kwargs):
        net = super().init_model(**kwargs)
        for m in net.models:
            for enc in [m] if hasattr(m, "dropout_layers") else []:
                for d in enc.dropout_layers:
                    d.p = 0.0
        net.domain_model[2].p = 0.0
        return net


def _fit(device, s, t, epochs=3, cls=_NoDropASN, **kw):
    gen = torch.Generator().manual_seed(5)
    noise = [[torch.randn(n, 5, generator=gen) for n in (s.x.size(0), t.x.size(0)) * 4] for _ in range(epochs)]
    # per epoch the reference's encoder call order: s_l, t_l, s_g, t_g, shared_l (s, t), shared_g (s, t)
    hook = lambda ep: [noise[ep][i].to(device) for i in range(8)]
    m = cls(20, 16, 5, 3, device=device, epoch=epochs, verbose=0, lr=1e-2, dropout=0.0, eps_hook=hook, **kw)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    torch.manual_seed(0)
    if device != "cpu":
        ops.dropout_state.counter(torch.device(device)).zero_()   # the Philox stream restarts: same masks, same noise
    m.fit(s, t)
    logits, _ = m.predict(t)
    return m, log, logits


def test_fit3_matches_the_host_restatement():
    s, t = _pair(3)
    _, log_c, lo_c = _fit("cpu", s, t)
    m, log_g, lo_g = _fit(DEV, s, t)
    for (lc, ac), (lg, ag) in zip(log_c, log_g):
        assert abs(lc - lg) <= 2e-4 * abs(lc) + 1e-5, (log_c, log_g)
    assert np.allclose(lo_g.cpu().numpy(), lo_c.numpy(), rtol=2e-3, atol=2e-4), (lo_g - lo_c.to(DEV)).abs().max()


def test_two_gpu_fits_are_bit_identical():
    s, t = _pair(8)
    _, log_a, lo_a = _fit(DEV, s, t, cls=pygda_amd.models.ASN)
    _, log_b, lo_b = _fit(DEV, s, t, cls=pygda_amd.models.ASN)
    assert log_a == log_b and torch.equal(lo_a, lo_b)


def _cfg(ns, es, nt, et, seed=7):
    from bench import make_cfg_a
    src, tgt = make_cfg_a(seed=seed, ns=ns, es=es, nt=nt, et=et)
    for d in (src, tgt):
        n = d.x.size(0)
        if int(d.edge_index.max()) + 1 != n:                # the reference needs the last node in edge_index
            d.edge_index = torch.cat([d.edge_index, torch.tensor([[n - 1, 0], [0, n - 1]])], 1)
    return src, tgt


def test_one_full_size_epoch_at_acm_dblp_shapes_without_an_nxn_buffer():
    src, tgt = (Data(x=d.x.to(DEV), edge_index=d.edge_index.to(DEV), y=d.y.to(DEV))
                for d in _cfg(9360, 15556, 5484, 8117))       # inputs resident: the second fit copies nothing in
    m = pygda_amd.models.ASN(src.x.size(1), 64, 5, 5, dropout=0.1, adv_dim=10, lr=1e-3, device=DEV, epoch=1,
                             verbose=0)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    m.fit(src, tgt)                                           # warm: process_graph (dense N x N scratch) is cached
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m.fit(src, tgt)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    assert len(log) == 2 and all(np.isfinite(v) and v > 0 for v in log)
    assert grow < 9360 * 9360 * 4, f"the epoch allocated {grow / 2**20:.1f} MiB"
    logits, _ = m.predict(tgt)
    assert logits.shape == (5484, 5) and torch.isfinite(logits).all()


def test_no_blas_product_on_the_asn_path(monkeypatch):
    src, tgt = _cfg(1200, 1800, 1000, 1500)
    m = pygda_amd.models.ASN(src.x.size(1), 64, 5, 5, dropout=0.1, device=DEV, epoch=2, verbose=0)
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


def test_fit3_against_the_reference_bounded_by_its_float64_run():
    from tests.conftest import load_golden
    from tests.test_asn_host import _fixture_pair, fixture_model
    g = load_golden("asn_fit3")
    s, t = _fixture_pair(g)
    m = fixture_model(g, DEV)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(int(g["init_seed"]))
    m.fit(s, t)
    _close(np.array(log), g["losses"], g["f64/losses"], "losses", 1e-5)
    for k, v in m.asn.state_dict().items():
        _close(v, g["final/" + k], g["f64/final/" + k], k, 1e-4)
    for data, key in ((s, "src_logits"), (t, "tgt_logits")):
        lo, _ = m.predict(data)
        _close(lo, g[key], g["f64/" + key], key, 1e-4)


def test_eager_and_captured_fits_are_bit_identical():
    s, t = _pair(12)

    def run(graph):
        m = pygda_amd.models.ASN(20, 16, 5, 3, device=DEV, epoch=7, verbose=0, lr=1e-2, dropout=0.1,
                                 use_hip_graph=graph, epochs_per_graph=3)
        log = []
        m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
        torch.manual_seed(0)
        ops.dropout_state.counter(torch.device(DEV)).zero_()
        m.fit(s, t)
        lo, _ = m.predict(t)
        return log, lo, [p.detach().clone() for p in m.asn.parameters()]

    le, oe, pe = run(False)
    lc, oc, pc = run(True)
    assert len(le) == 7 and le == lc
    assert torch.equal(oe, oc) and all(torch.equal(a, b) for a, b in zip(pe, pc))
