"""JHGDA without a GPU: the public surface (signature, defaults, the alias import), the rejections raised before any
device work, the module names and init stream, the proximity loss of both branches against float64, the dense GCN's
edge-weight gradient against autograd of the PyG lines, and host fits against the fixtures recorded from the
reference's own jhgda.py (tests/golden/make_golden_jhgda.py)."""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pygda_amd.data import Data

HERE = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = {"jhgda_fit3.npz": {}, "jhgda_fit3_sparse_share.npz": dict(sparse=True, share=True)}


def _pair(name):
    f = np.load(os.path.join(HERE, name))
    s = Data(x=torch.from_numpy(f["src_x"]), edge_index=torch.from_numpy(f["src_ei"]), y=torch.from_numpy(f["src_y"]))
    t = Data(x=torch.from_numpy(f["tgt_x"]), edge_index=torch.from_numpy(f["tgt_ei"]), y=torch.from_numpy(f["tgt_y"]))
    return f, s, t


def test_signature_defaults_and_alias():
    from pygda.models import JHGDA as Alias
    from pygda_amd.models import JHGDA
    assert Alias is JHGDA
    sig = inspect.signature(JHGDA.__init__)
    want = dict(num_layers=3, dropout=0., act=F.relu, weight_decay=0., share=False, sparse=False, classwise=True,
                pool_ratio=0.2, g_mmd=0.5, c_mmd=0.5, d_weight=0.1, ce_weight=0.1, prox_weight=0.1, cce_weight=0.1,
                lm_weight=0.1, ls_weight=0.1, lr=4e-3, epoch=200, device='cuda:0', batch_size=0, num_neigh=-1,
                verbose=2)
    for k, v in want.items():
        assert sig.parameters[k].default == v, k
    assert list(sig.parameters)[:4] == ["self", "in_dim", "hid_dim", "num_classes"]
    from pygda.nn import GCNPooling, JHGDABase
    assert JHGDABase.__module__ == "pygda_amd.nn.jhgda_base" and GCNPooling is not None


def test_rejections_before_device_work():
    from pygda_amd.models import JHGDA
    with pytest.raises(ValueError):
        JHGDA(16, 16, 3, batch_size=64, device="cpu")
    with pytest.raises(ValueError):
        JHGDA(16, 16, 3, classwise=False, device="cpu")
    JHGDA(16, 16, 3, classwise=False, pool_ratio=1.0, device="cpu")
    _, s, t = _pair("jhgda_fit3.npz")
    m = JHGDA(16, 16, 3, num_layers=4, device="cpu", epoch=1, verbose=0)      # 300 -> 60 -> 12 -> 2 -> 0
    with pytest.raises(ValueError, match="width 0"):
        m.fit(s, t)
    wide = JHGDA(16, 16, 3, pool_ratio=0.9, device="cuda:0", epoch=1, verbose=0)
    big = Data(x=torch.rand(5000, 16), edge_index=torch.tensor([[0, 1], [1, 0]]), y=torch.zeros(5000, dtype=torch.long))
    with pytest.raises(ValueError, match="proximity kernel"):
        wide._check(big, big)                                   # 4500 > JHGDA_PROX_MAX_K, raised without a device


def test_state_dict_keys_and_init_stream():
    from pygda_amd.nn import JHGDABase
    f = np.load(os.path.join(HERE, "jhgda_fit3.npz"))
    torch.manual_seed(int(f["init_seed"]))
    net = JHGDABase(16, 16, 3, device="cpu", pool_ratio=0.2, num_s=300, num_t=260, num_layers=3, classwise=True)
    want = {k[5:] for k in f.files if k.startswith("init/")}
    assert set(net.state_dict()) == want
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), f["init/" + k]), k
    assert [p.gcn.out_channels for p in net.gnn_pool_src] == [60, 12, 2]
    assert [p.gcn.out_channels for p in net.gnn_pool_tgt] == [52, 10, 2]
    g = np.load(os.path.join(HERE, "jhgda_fit3_sparse_share.npz"))
    torch.manual_seed(int(g["init_seed"]))
    net = JHGDABase(16, 16, 3, device="cpu", pool_ratio=0.2, num_s=300, num_t=260, share=True, sparse=True)
    assert set(net.state_dict()) == {k[5:] for k in g.files if k.startswith("init/")}
    assert all(np.array_equal(v.numpy(), g["init/" + k]) for k, v in net.state_dict().items())


def _prox64(A, S):
    S = S.double()
    n = S.size(0)
    p = torch.clamp(S @ S.T, max=1.0)
    pos, neg = torch.log(p + 1e-7), torch.log(1 - p + 1e-7)
    if A.shape[0] < A.shape[1]:
        a = torch.zeros(n, n, dtype=torch.float64).index_put_((A[0], A[1]), torch.ones(A.size(1), dtype=torch.float64),
                                                              accumulate=True)
    else:
        a = A.double()
    return torch.sum(-a * pos - (1 - a) * neg) / (n * n)


def test_proximity_branches_against_float64():
    from pygda_amd.ops import jhgda_prox
    g = torch.Generator().manual_seed(5)
    S = torch.softmax(torch.randn(40, 7, generator=g) * 3, dim=1)
    ei = torch.randint(0, 40, (2, 90), generator=g)
    ei = torch.cat([ei, ei[:, :3]], 1)                          # duplicates count each time
    assert abs(float(jhgda_prox(ei, S)) - float(_prox64(ei, S))) < 1e-5
    A = torch.rand(40, 40, generator=g)
    assert abs(float(jhgda_prox(A, S)) - float(_prox64(A, S))) < 1e-5


def test_dense_gcn_edge_weight_gradient_against_autograd_of_the_stub():
    """dense_gcn(conv, x, A) = GCNConv(x, *adj2coo(A)): forward and the gradients to A and x against autograd of the PyG
    stub's GCNConv (tests/golden/_pyg_stub.py: add_remaining_self_loops keeping the diagonal weight, destination
    degrees) on adj2coo's complete graph.  Column 3 has degree 0: the stub's deg^-1/2 is masked to 0 there and its
    gradient is 0 * inf; dense_gcn passes 0, which is what both give wherever the column has any weight."""
    from pygda_amd.nn.gcn_conv import GCNConv
    from pygda_amd.nn.jhgda_base import JHGDABase, dense_gcn, host_gcn
    from tests.golden import _pyg_stub
    torch.manual_seed(2)
    conv = GCNConv(6, 4).double()
    stub = _pyg_stub.GCNConv(6, 4).double()
    with torch.no_grad():
        conv.bias.uniform_(-1, 1)
        stub.lin.weight.copy_(conv.lin.weight)
        stub.bias.copy_(conv.bias)
    x = torch.randn(9, 6, dtype=torch.float64, requires_grad=True)
    A = torch.rand(9, 9, dtype=torch.float64)
    A[:, 3] = 0
    A.requires_grad_(True)
    w = torch.randn(9, 4, dtype=torch.float64)
    out = dense_gcn(conv, x, A)
    gA, gx = torch.autograd.grad((out * w).sum(), (A, x))
    ei, ew = JHGDABase.adj2coo(None, A)
    ref = stub(x, ei, ew)
    rA, rx = torch.autograd.grad((ref * w).sum(), (A, x))
    assert torch.allclose(out, ref, atol=1e-12)
    assert torch.allclose(gx, rx, atol=1e-12)
    keep = [c for c in range(9) if c != 3]
    assert torch.allclose(gA[:, keep], rA[:, keep], atol=1e-12)
    assert torch.all(gA[:, 3] == 0)
    own = host_gcn(conv, x, ei, ew)                             # the host fit's edge-list lines agree as well
    assert torch.allclose(own, ref, atol=1e-12)


@pytest.fixture
def one_thread():
    """The generator records on one CPU thread; the host fit runs the same way, so that its reductions take one order
    whatever pool size the session picked."""
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(old)


def check_fit(f, log, lm, sd, src_logits, tgt_logits, n_src, tol_loss=1e-5, tol_param=1e-5, tol_logit=1e-4):
    """A fit against the reference's record.  label_matching is an argmax count: on exact ties (empty clusters give
    uniform label rows) the engine's rounding decides it, and it has no gradient.  So the losses are compared with it
    taken out, and it is held to within one flipped row per level and domain.  The parameters are bounded by the
    reference's own float32 - float64 distance, and the source accuracy to one flipped prediction."""
    losses, accs = np.array([l for l, _ in log]), np.array([a for _, a in log])
    np.testing.assert_allclose(losses - 0.1 * np.array(lm), f["losses"] - 0.1 * f["lm"], rtol=tol_loss, atol=tol_loss)
    assert np.abs(np.array(lm) - f["lm"]).max() <= 1.0 + 1e-6
    assert np.abs(accs - f["accs"]).max() <= 1.0 / n_src + 1e-12
    for k, v in sd.items():
        ref32, ref64 = f["final/" + k], f["f64/final/" + k]
        tol = tol_param + 2 * np.abs(ref32 - ref64).max()       # Adam on near-zero gradients: the float64 arbiter
        assert np.abs(v.double().cpu().numpy() - ref32).max() <= tol, k
    np.testing.assert_allclose(src_logits, f["src_logits"], atol=tol_logit)
    np.testing.assert_allclose(tgt_logits, f["tgt_logits"], atol=tol_logit)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_host_fit_against_reference(name, one_thread):
    from pygda_amd.models import JHGDA
    f, s, t = _pair(name)
    m = JHGDA(16, 16, 3, num_layers=3, lr=4e-3, device="cpu", epoch=3, verbose=0, **FIXTURES[name])
    log = []
    m.epoch_hook = lambda e, loss, acc, secs: log.append((loss, acc))
    torch.manual_seed(int(f["init_seed"]))
    m.fit(s, t)
    check_fit(f, log, m.lm_log, m.jhgda.state_dict(), m.predict(s)[0].numpy(), m.predict(t)[0].numpy(),
              s.x.size(0))


def test_fixture_regenerates_bit_for_bit(tmp_path):
    from tests.golden import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not on this machine")
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.golden.make_golden_jhgda", "--out", str(tmp_path)], cwd=root,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in FIXTURES:
        a, b = np.load(os.path.join(HERE, name)), np.load(tmp_path / name)
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), (name, k)
