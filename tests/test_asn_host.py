"""ASN without a GPU: the public surface (signature, defaults, the alias import), the rejections raised before any
device work, the module names and init stream, and the host operators against float64 restatements of the
reference's lines (reconstruction cost, KLD, DiffLoss, the normalised PPMI adjacency) and a host fit."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pygda_amd import ops
from pygda_amd.data import Data


def _graph(n, f=12, c=3, seed=0, last=True):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n - 1, (2 * n,), generator=g), torch.randint(0, n - 1, (2 * n,), generator=g)
    if last:
        src, dst = torch.cat([src, torch.tensor([n - 1, 0])]), torch.cat([dst, torch.tensor([0, n - 1])])
    return Data(x=torch.rand(n, f, generator=g), edge_index=torch.stack([src, dst]),
                y=torch.randint(0, c, (n,), generator=g))


def test_signature_defaults_and_alias():
    from pygda.models import ASN as Alias
    from pygda_amd.models import ASN
    assert Alias is ASN
    sig = inspect.signature(ASN.__init__)
    want = dict(num_layers=3, step=3, dropout=0., act=F.relu, lambda_r=1.0, lambda_d=0.1, lambda_f=0.001, adv_dim=10,
                weight_decay=5e-4, lr=3e-2, epoch=200, device='cuda:0', batch_size=0, num_neigh=-1, verbose=2)
    for k, v in want.items():
        assert sig.parameters[k].default == v, k
    assert sig.parameters["hid_dim_vae"].default is inspect.Parameter.empty
    assert list(sig.parameters)[:5] == ["self", "in_dim", "hid_dim", "hid_dim_vae", "num_classes"]


def test_rejections_before_device_work():
    from pygda_amd.models import ASN
    with pytest.raises(ValueError):
        ASN(12, 16, 5, 3, batch_size=64, device="cpu")
    with pytest.raises(ValueError):
        ASN(12, 16, 5, 3, num_layers=2, device="cpu")
    s, t = _graph(20), _graph(15, last=False)                  # a trailing isolated target node
    m = ASN(12, 16, 5, 3, device="cpu", epoch=1, verbose=0)
    with pytest.raises(ValueError, match="max"):
        m.fit(s, t)
    bad = _graph(15)
    bad.edge_index[0, 0] = 99
    with pytest.raises(ValueError):
        m.fit(s, bad)
    wide = ASN(12, 16, 65, 3, device="cuda:0", epoch=1, verbose=0)
    with pytest.raises(ValueError):
        wide._check(s)                                          # 2 * 65 > ASN_MAX_K, raised without a device


def test_state_dict_keys_and_init_stream():
    from pygda_amd.nn import ASNBase
    torch.manual_seed(3)
    net = ASNBase(12, 16, 5, 3, adv_dim=10)
    keys = set(net.state_dict())
    for enc in ("private_encoder_s_l", "private_encoder_t_l", "private_encoder_s_g", "private_encoder_t_g",
                "shared_encoder_l", "shared_encoder_g"):
        for i, (fi, fo) in enumerate([(12, 16), (16, 5), (16, 5)]):
            assert net.state_dict()[f"{enc}.conv_layers.{i}.lin.weight"].shape == (fo, fi)
            assert f"{enc}.conv_layers.{i}.bias" in keys
    for k in ("cls_model.0.weight", "domain_model.0.weight", "domain_model.3.bias", "att_model.dense_weight.weight",
              "att_model_self_s.dense_weight.bias", "att_model_self_t.dense_weight.weight"):
        assert k in keys
    assert len(net.models) == 13
    torch.manual_seed(3)
    again = ASNBase(12, 16, 5, 3, adv_dim=10)
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), again.state_dict().values()))
    assert not any(d.training is False for d in net.private_encoder_s_l.dropout_layers)
    net.eval()
    assert all(d.training for d in net.shared_encoder_l.dropout_layers)      # never reached by eval()


def test_labels_pos_weight_and_norm():
    ei = torch.tensor([[0, 0, 1, 2, 2], [1, 1, 2, 2, 0]])          # a duplicate and a self loop
    lab = ops.AsnLabels(ei, 3)
    A = torch.zeros(3, 3)
    A.index_put_((ei[0], ei[1]), torch.ones(5), accumulate=True)
    assert torch.equal(lab.dense(), A + torch.eye(3))
    assert lab.dense()[2, 2] == 2
    pw = (9 - A.sum()) / A.sum()
    assert lab.pos_weight == float(pw) and lab.norm == float(9 / ((9 - A.sum()) * 2))
    with pytest.raises(ValueError):
        ops.AsnLabels(torch.tensor([[0], [1]]), 3)


def test_host_recon_kld_diff_against_float64():
    d = _graph(30)
    lab = ops.AsnLabels(d.edge_index, 30)
    torch.manual_seed(1)
    z = torch.randn(30, 10)
    got = ops.asn_recon_loss(z, lab)
    x = z.double() @ z.double().t()
    y = lab.dense().double()
    pw = lab.pos_weight
    f = (1 - y) * x + (1 + (pw - 1) * y) * (torch.log1p(torch.exp(-x.abs())) + torch.clamp(-x, min=0))
    assert abs(float(got) - float(lab.norm * f.mean())) < 1e-5 * abs(float(got))
    mu, lv = torch.randn(30, 20), 0.3 * torch.randn(30, 20)
    k64 = -0.5 / 60 * torch.mean(torch.sum(1 + 2 * lv.double() - mu.double() ** 2 - lv.double().exp() ** 2, 1))
    assert abs(float(ops.asn_kld(mu, lv, 60)) - float(k64)) < 1e-5 * abs(float(k64))
    a, b = torch.randn(30, 5), torch.randn(30, 5)
    an = a.double() / (a.double().norm(dim=1, keepdim=True) + 1e-6)
    bn = b.double() / (b.double().norm(dim=1, keepdim=True) + 1e-6)
    assert abs(float(ops.asn_diff_loss(a, b)) - float(((an.t() @ bn) ** 2).mean())) < 1e-5


def test_host_ppmi_adjacency_is_pyg_gcn_norm_of_the_scaled_ppmi():
    d = _graph(25)
    adj = ops.asn_ppmi_graph(d.edge_index, 25, 3)
    P = ops._asn_ppmi_host(d.edge_index, 25, 3).double()
    assert torch.count_nonzero(torch.diagonal(P)) == 0          # the PPMI diagonal is zero: the loops add 1
    M = P + torch.eye(25, dtype=torch.float64)
    dis = M.sum(1).pow(-0.5)
    assert torch.allclose(adj.double(), dis[None, :] * M * dis[:, None], rtol=1e-5, atol=1e-7)
    assert torch.allclose(P.sum(1)[P.sum(1) > 0], torch.ones(1, dtype=torch.float64), atol=1e-5)


def test_host_fit_runs_the_reference_lines():
    from pygda_amd.models import ASN
    s, t = _graph(40, seed=1), _graph(30, seed=2)
    m = ASN(12, 16, 5, 3, device="cpu", epoch=3, verbose=0, lr=1e-2)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    m.fit(s, t)
    assert len(log) == 3 and all(np.isfinite(log))
    logits, y = m.predict(t)
    assert logits.shape == (30, 3) and y is t.y


# ------------------------------------------------------------ against the reference's own run (asn_fit3.npz) --
def _fixture():
    from tests.conftest import load_golden
    return load_golden("asn_fit3")


def _fixture_pair(g):
    T = torch.from_numpy
    return (Data(x=T(g["src_x"]), edge_index=T(g["src_ei"]), y=T(g["src_y"])),
            Data(x=T(g["tgt_x"]), edge_index=T(g["tgt_ei"]), y=T(g["tgt_y"])))


def fixture_model(g, device, **kw):
    """The fixture's configuration with the hidden and discriminator dropout at 0 and its recorded eps fed."""
    from pygda_amd.models import ASN

    class NoDrop(ASN):
        def init_model(self, **k):
            net = super().init_model(**k)
            for enc in (net.private_encoder_s_l, net.private_encoder_t_l, net.private_encoder_s_g,
                        net.private_encoder_t_g, net.shared_encoder_l, net.shared_encoder_g):
                for d in enc.dropout_layers:
                    d.p = 0.0
            net.domain_model[2].p = 0.0
            return net

    eps = [torch.from_numpy(g[f"eps/{k}"]) for k in range(24)]
    return NoDrop(16, 16, 5, 3, step=3, dropout=0.0, adv_dim=10, lr=1e-2, weight_decay=5e-4, epoch=3, verbose=0,
                  device=device, eps_hook=lambda e: [eps[8 * e + i].to(device) for i in range(8)], **kw)


def test_init_stream_matches_the_reference():
    from pygda_amd.nn import ASNBase
    g = _fixture()
    torch.manual_seed(int(g["init_seed"]))
    sd = ASNBase(16, 16, 5, 3, adv_dim=10, dropout=0.0).state_dict()
    ref = {k[len("init/"):] for k in g if k.startswith("init/")}
    assert set(sd) == ref
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), g["init/" + k]), k


def test_host_ppmi_against_the_reference_csr():
    g = _fixture()
    for dom, key in (("s", "src_ei"), ("t", "tgt_ei")):
        ref32 = torch.sparse_csr_tensor(torch.from_numpy(g[f"ppmi_{dom}_crow"]), torch.from_numpy(g[f"ppmi_{dom}_col"]),
                                        torch.from_numpy(g[f"ppmi_{dom}_val"])).to_dense().double()
        ref64 = torch.from_numpy(g[f"ppmi64_{dom}"])
        n = ref64.size(0)
        ours = ops._asn_ppmi_host(torch.from_numpy(g[key]), n, 3).double()
        assert torch.allclose(ref32, ref64, rtol=1e-6, atol=1e-7)
        # numpy 2 computes the reference's PPMI in float64, the port in float32: an entry may appear or vanish at the
        # ppmi < 0 threshold (one side exactly zero); every other entry agrees closely
        both = (ours != 0) & (ref64 != 0)
        assert torch.allclose(ours[both], ref64[both], rtol=1e-4, atol=1e-6)
        flip = (ours != 0) ^ (ref64 != 0)
        assert np.abs(ours[flip].numpy()).max(initial=0) < 1e-3 and np.abs(ref64[flip].numpy()).max(initial=0) < 1e-3


def test_float64_run_of_the_reference_bounds_its_float32_run():
    g = _fixture()
    assert np.allclose(g["f64/losses"], g["losses"], rtol=1e-5)
    assert np.allclose(g["f64/tgt_logits"], g["tgt_logits"], rtol=1e-4, atol=1e-5)


def test_cpu_fit_matches_the_reference():
    g = _fixture()
    s, t = _fixture_pair(g)
    m = fixture_model(g, "cpu")
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    torch.manual_seed(int(g["init_seed"]))
    m.fit(s, t)
    assert np.allclose([l for l, _ in log], g["losses"], rtol=1e-6)
    assert [a for _, a in log] == list(g["accs"])
    for k, v in m.asn.state_dict().items():
        assert np.allclose(v.numpy(), g["final/" + k], rtol=1e-4, atol=1e-5), k
    for data, key in ((s, "src_logits"), (t, "tgt_logits")):
        lo, y = m.predict(data)
        assert np.allclose(lo.numpy(), g[key], rtol=1e-4, atol=1e-5) and y is data.y


def test_host_gcn_takes_an_int32_edge_index():
    from pygda_amd.nn.asn_base import host_gcn
    from pygda_amd.nn import GCNConv
    conv = GCNConv(4, 3)
    x = torch.rand(6, 4)
    ei = torch.tensor([[0, 1, 2, 5], [1, 2, 3, 0]])
    assert torch.equal(host_gcn(conv, x, ei.to(torch.int32)), host_gcn(conv, x, ei))


def test_fixture_regenerates_bit_for_bit(tmp_path):
    from tests.golden import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not on this machine")
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.golden.make_golden_asn", "--out", str(tmp_path)], cwd=root,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    new, old = np.load(tmp_path / "asn_fit3.npz"), _fixture()
    assert sorted(new.files) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k]), k
