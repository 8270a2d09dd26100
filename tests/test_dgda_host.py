"""DGDA without a GPU: the public surface, the refusals raised before any device work, the host path of the trainer
against the reference's own run (dgda_fit3.npz: losses, accuracies, final parameters, two successive ``predict`` calls),
the reference's quirks one assertion each, the bit rule of the manipulated adjacency against a dense restatement of
``drop_edges`` fed the same masks, the density that rule predicts, and DeepWalk's host walks."""
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
    src, dst = torch.cat([src, dst, src[:2]]), torch.cat([dst, src, dst[:2]])      # undirected, two duplicates
    if last:
        src, dst = torch.cat([src, torch.tensor([n - 1, 0])]), torch.cat([dst, torch.tensor([0, n - 1])])
    return Data(x=torch.rand(n, f, generator=g), edge_index=torch.stack([src, dst]),
                y=torch.randint(0, c, (n,), generator=g))


def _emb(*ns, dim=8, seed=9):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(n, dim, generator=g) for n in ns)


def _small(**kw):
    from pygda_amd.models import DGDA
    args = dict(dec_dim=8, d_dim=4, y_dim=6, m_dim=5, device="cpu", epoch=2, verbose=0, lr=1e-2,
                pretrained_emb=_emb(40, 30))
    args.update(kw)
    return DGDA(12, 16, 3, **args)


def test_signature_defaults_and_alias():
    from pygda.models import DGDA as Alias
    from pygda.nn import DGDABase, DWPretrain                         # noqa: F401
    from pygda_amd.models import DGDA
    assert Alias is DGDA
    sig = inspect.signature(DGDA.__init__)
    want = dict(num_layers=3, dropout=0., act=F.relu, dec_dim=64, d_dim=64, y_dim=256, m_dim=128, recons_w=1.0, beta=0.5,
                ent_w=1.0, d_w=1.0, y_w=1.0, m_w=0.1, edge_drop_rate=0.1, edge_add_rate=0.1, weight_decay=5e-4,
                lr=0.001, epoch=400, device='cuda:0', batch_size=0, num_neigh=-1, verbose=2)
    for k, v in want.items():
        assert sig.parameters[k].default == v, k
    assert list(sig.parameters)[:4] == ["self", "in_dim", "hid_dim", "num_classes"]
    dw = inspect.signature(DWPretrain.__init__)
    for k, v in dict(epoch=200, embedding_dim=128, walk_length=20, context_size=10, walks_per_node=10,
                     num_negative_samples=1).items():
        assert dw.parameters[k].default == v, k


def test_rejections_before_device_work(monkeypatch):
    from pygda_amd.models import DGDA
    with pytest.raises(ValueError):
        DGDA(12, 16, 3, batch_size=64, device="cpu")
    s, t = _graph(40), _graph(30, last=False)                      # a trailing isolated target node
    with pytest.raises(ValueError, match="max"):
        _small().fit(s, t)
    bad = _graph(30)
    bad.edge_index[0, 0] = 99
    with pytest.raises(ValueError):
        _small().fit(s, bad)
    with pytest.raises(ValueError):
        _small(device="cuda:0", dec_dim=ops.DGDA_MAX_K + 1)._check(s)            # raised without a device
    with pytest.raises(ValueError):
        _small(device="cuda:0", y_dim=ops.DGDA_MAX_C)._check(s)
    with pytest.raises(NotImplementedError):
        from pygda_amd.nn.dgda_base import GNN_VGAE_Encoder
        GNN_VGAE_Encoder(8, 8, 2, 2, 2, 0.0, backbone="gat")
    import pygda_amd.distributed as dist
    monkeypatch.setattr(dist, "active", lambda: True)
    with pytest.raises(NotImplementedError):
        _small().fit(s, _graph(30))


# --------------------------------------------------------- against the reference's own run (dgda_fit3.npz) --
def _fixture():
    from tests.conftest import load_golden
    return load_golden("dgda_fit3")


def _fixture_pair(g):
    T = torch.from_numpy
    return (Data(x=T(g["src_x"]), edge_index=T(g["src_ei"]), y=T(g["src_y"])),
            Data(x=T(g["tgt_x"]), edge_index=T(g["tgt_ei"]), y=T(g["tgt_y"])))


def fixture_nadj(g, epoch, dom, n):
    return torch.from_numpy(np.unpackbits(g[f"nadj/{epoch}/{dom}"])[:n * n].reshape(n, n).astype(np.float32))


def fixture_model(g, device, **kw):
    """The fixture's configuration with its recorded embeddings, eps and nadj fed."""
    from pygda_amd.models import DGDA
    ns, nt = g["src_x"].shape[0], g["tgt_x"].shape[0]
    eps = [torch.from_numpy(g[f"eps/{k}"]) for k in range(36)]
    return DGDA(16, 16, 3, dropout=0.0, dec_dim=8, d_dim=4, y_dim=6, m_dim=5, lr=1e-3, weight_decay=5e-4,
                edge_drop_rate=0.1, edge_add_rate=0.1, epoch=3, verbose=0, device=device,
                pretrained_emb=(torch.from_numpy(g["emb_s"]), torch.from_numpy(g["emb_t"])),
                eps_hook=lambda e: [eps[12 * e + i].to(device) for i in range(12)],
                manip_hook=lambda e: (fixture_nadj(g, e, "s", ns).to(device), fixture_nadj(g, e, "t", nt).to(device)),
                **kw)


def test_init_stream_and_state_dict_match_the_reference():
    from pygda_amd.nn import DGDABase
    g = _fixture()
    s, t = _fixture_pair(g)
    torch.manual_seed(int(g["init_seed"]))
    net = DGDABase(16, 3, 16, 8, 4, 6, 5, 0.0, "gcn", torch.from_numpy(g["emb_s"]), s.x, torch.from_numpy(g["emb_t"]),
                   t.x)
    sd = net.state_dict()
    assert set(sd) == {k[len("init/"):] for k in g if k.startswith("init/")}
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), g["init/" + k]), k
    assert sd["encoder.gnn0.weight"].shape == (16 + 8 + 16, 16)              # cat(x, emb, x)


def test_float64_run_of_the_reference_bounds_its_float32_run():
    g = _fixture()
    assert np.allclose(g["f64/losses"], g["losses"], rtol=1e-5)
    assert np.allclose(g["f64/tgt_logits_2"], g["tgt_logits_2"], rtol=1e-4, atol=1e-5)


def _cpu_fit():
    g = _fixture()
    s, t = _fixture_pair(g)
    m = fixture_model(g, "cpu")
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    torch.manual_seed(int(g["init_seed"]))
    m.fit(s, t)
    return g, s, t, m, log


def test_cpu_fit_matches_the_reference():
    g, s, t, m, log = _cpu_fit()
    assert np.allclose([l for l, _ in log], g["losses"], rtol=1e-6)
    assert [a for _, a in log] == list(g["accs"])
    for k, v in m.dgda.state_dict().items():
        assert np.allclose(v.numpy(), g["final/" + k], rtol=1e-4, atol=1e-5), k
    for key in ("tgt_logits_1", "tgt_logits_2"):
        lo, y = m.predict(s)                                    # the argument's graph is ignored: the stored target's
        assert np.allclose(lo.numpy(), g[key], rtol=1e-4, atol=1e-5) and y is s.y
    # quirk: predict stacks another I onto the stored adjacency at every call (A + I after fit, A + 3 I now)
    diag = torch.zeros(t.x.size(0)).index_add_(0, t.edge_index[0][t.edge_index[0] == t.edge_index[1]],
                                               torch.ones(int((t.edge_index[0] == t.edge_index[1]).sum())))
    assert np.array_equal(m.t_adj.diagonal().numpy(), g["t_adj_diag"]) and np.array_equal(g["t_adj_diag"], diag + 3)
    assert not np.allclose(g["tgt_logits_1"], g["tgt_logits_2"], rtol=1e-4, atol=1e-5)
    # quirk: the second pass runs DGDA_loss with manipulate=False -- neither the noise decoder nor the graph
    # discriminator ever receives a gradient (in the fixture their parameters never move)
    for mod in (m.dgda.noise_decoder, m.dgda.graphDiscriminator):
        assert all(p.grad is None for p in mod.parameters())
    frozen = [k[len("init/"):] for k in g if k.startswith(("init/noise_decoder", "init/graphDiscriminator"))]
    assert len(frozen) == 8 and all(np.array_equal(g["final/" + k], g["init/" + k]) for k in frozen)
    # quirk: the input is cat(x, emb, x) -- both x blocks of gnn0.weight receive their gradient
    w0, w1 = g["init/encoder.gnn0.weight"], g["final/encoder.gnn0.weight"]
    assert not np.allclose(w0[:16], w1[:16]) and not np.allclose(w0[24:], w1[24:])


def test_encoder_mutates_its_adjacency_in_place_and_the_labels_see_it():
    from pygda_amd.models.dgda import dense_adj
    g, s, t, m, _ = _cpu_fit()
    adj = dense_adj(t.edge_index, t.x.size(0))
    before = adj.clone()
    m.dgda.train()
    m.dgda(t.x, torch.arange(t.x.size(0)), adj, 1)
    assert torch.equal(adj, before + torch.eye(t.x.size(0)))
    # the second pass: nadj (diagonal 1) comes back with diagonal 2
    nadj = fixture_nadj(g, 0, "t", t.x.size(0))
    assert torch.equal(nadj.diagonal(), torch.ones(t.x.size(0))) and torch.equal(nadj, nadj.t())
    m.dgda(t.x, torch.arange(t.x.size(0)), nadj, 1)
    assert torch.equal(nadj.diagonal(), torch.full((t.x.size(0),), 2.0))


def test_kl_loss_divides_by_the_latent_width():
    from pygda_amd.models import DGDA
    mu, lv = torch.ones(7, 5), torch.zeros(7, 5)             # sum_k (1 + 0 - 1 - 1) = -5 per row
    assert float(DGDA.kl_loss(mu, lv)) == 0.5                # -0.5 / 5 * -5; by the 7 nodes it would be 0.357
    assert float(ops.asn_kld(mu, lv, mu.shape[1])) == 0.5    # the device path's operator, called with the width


def test_the_loss_is_clamped_at_zero():
    s, t = _graph(40, seed=1), _graph(30, seed=2)
    m = _small(ent_w=-100.0, epoch=1)                          # every other term is non-negative
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    m.fit(s, t)
    assert log == [0.0]


def test_host_fit_draws_its_own_noise_and_masks():
    s, t = _graph(40, seed=1), _graph(30, seed=2)
    m = _small(epoch=3)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    m.fit(s, t)
    assert len(log) == 3 and all(np.isfinite(log))
    logits, y = m.predict(t)
    assert logits.shape == (30, 3) and y is t.y


# ------------------------------------------------------------------------------------------- the bit rule --
def _drop_edges_dense(adj, drop_mask, add_mask):
    """drop_edges restated densely with its two Bernoulli masks given."""
    n = adj.size(0)
    nadj = adj.clone()
    nadj -= drop_mask
    nadj[nadj < 0] = 0
    nadj += add_mask
    nadj = nadj.tril() + nadj.tril().permute(1, 0)
    nadj += torch.eye(n)
    nadj[nadj < 0] = 0
    nadj[nadj > 0] = 1
    return nadj


def _adj_plus_i(d):
    from pygda_amd.models.dgda import dense_adj
    n = d.x.size(0)
    return dense_adj(d.edge_index, n) + torch.eye(n)


def test_bit_rule_against_the_dense_restatement_of_drop_edges():
    d = _graph(70, seed=5)
    adj = _adj_plus_i(d)
    assert adj.max() >= 2                                        # a duplicate edge: it survives its drop
    gen = torch.Generator().manual_seed(3)
    for p_drop, p_add in ((0.1, 0.1), (0.9, 0.02), (1.0, 0.0), (0.0, 1.0)):
        drop = torch.bernoulli(torch.full_like(adj, p_drop), generator=gen)
        add = torch.bernoulli(torch.full_like(adj, p_add), generator=gen)
        got = ops.dgda_manip_host(adj, drop, add)
        assert torch.equal(got, _drop_edges_dense(adj, drop, add))
        assert torch.equal(got, got.t()) and torch.equal(got.diagonal(), torch.ones(70))


def predicted_bits(adj, p_drop, p_add):
    """Mean and standard deviation of ``sum(bits)`` under the rule, from the rates and the edge counts alone: of the
    N (N - 1) / 2 pairs below the diagonal, one with no edge is set with p_add, one with a single edge with
    1 - p_drop (1 - p_add), one with a duplicate edge always; every pair counts twice, the diagonal once."""
    n = adj.size(0)
    low = torch.tril(adj, -1)
    m1, m2 = int((low == 1).sum()), int((low >= 2).sum())
    m0 = n * (n - 1) // 2 - m1 - m2
    q = 1 - p_drop * (1 - p_add)
    mean = n + 2 * (m0 * p_add + m1 * q + m2)
    std = 2 * (m0 * p_add * (1 - p_add) + m1 * q * (1 - q)) ** 0.5
    return mean, std


def test_predicted_density_against_the_dense_restatement_at_1000_nodes():
    d = _graph(1000, seed=7)
    adj = _adj_plus_i(d)
    p_drop, p_add = 0.1, float((adj.sum() + 1000 * 1000) / (1000 * 1000) * 0.1)
    gen = torch.Generator().manual_seed(11)
    drop = torch.bernoulli(torch.full_like(adj, p_drop), generator=gen)
    add = torch.bernoulli(torch.full_like(adj, p_add), generator=gen)
    mean, std = predicted_bits(adj, p_drop, p_add)
    assert abs(float(_drop_edges_dense(adj, drop, add).sum()) - mean) <= 5 * std
    lab = ops.AsnLabels(d.edge_index, 1000)
    assert abs(ops.dgda_p_add(lab, 0.1) - p_add) < 1e-7


def test_host_drop_edges_fills_an_almost_empty_graph_to_the_add_rate():
    # torch.bernoulli(adj, p=...) ignores adj: on a 200-node graph with two edges the trainer's drop_edges still
    # returns a ~10 % dense matrix, as the rule predicts
    ei = torch.tensor([[0, 199], [199, 0]])
    adj = _adj_plus_i(Data(x=torch.zeros(200, 1), edge_index=ei, y=None))
    torch.manual_seed(0)
    nadj = _small().drop_edges(adj, 0.1, 0.1)
    mean, std = predicted_bits(adj, 0.1, float((adj.sum() + 200 * 200) / (200 * 200) * 0.1))
    assert abs(float(nadj.sum()) - mean) <= 5 * std and 0.08 < float(nadj.mean()) < 0.12


def test_host_fit_draws_the_references_noise_and_masks():
    """No hooks: at the fixture's seed the host path's own randn_like and torch.bernoulli calls come in the reference's
    order with its probabilities, so it redraws the recorded eps and nadj and lands on the recorded losses."""
    from pygda_amd.models import DGDA
    g = _fixture()
    s, t = _fixture_pair(g)
    m = fixture_model(g, "cpu")
    m.eps_hook = m.manip_hook = None
    drawn, drop = [], m.drop_edges

    def recording(adj, *a):
        out = drop(adj, *a)
        drawn.append(out.clone())                     # the encoder adds I to what it is handed
        return out

    m.drop_edges = recording
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(int(g["init_seed"]))
    m.fit(s, t)
    assert len(drawn) == 6
    for k, a in enumerate(drawn):
        assert torch.equal(a, fixture_nadj(g, k // 2, "st"[k % 2], a.size(0))), k
    assert np.allclose(log, g["losses"], rtol=1e-6)
    for k, v in m.dgda.state_dict().items():
        assert np.allclose(v.numpy(), g["final/" + k], rtol=1e-4, atol=1e-5), k


# ----------------------------------------------------------------------------------------------- DeepWalk --
def test_host_walks_follow_edges_and_the_loss_falls_on_two_cliques():
    from pygda_amd.nn import DWPretrain
    # two 160-cliques and node 320 without edges: three batches per epoch, so five epochs are 15 optimiser steps and
    # the fall of the loss (about 0.3) is well above the sampling noise of the negatives (about 0.05 per epoch)
    a = torch.combinations(torch.arange(160)).t()
    ei = torch.cat([a, a.flip(0), a + 160, (a + 160).flip(0)], 1)
    d = Data(x=torch.zeros(321, 1), edge_index=ei, y=torch.zeros(321, dtype=torch.long))
    torch.manual_seed(0)
    p = DWPretrain(d, epoch=5, embedding_dim=8, walk_length=8, context_size=4, walks_per_node=4, verbose=False)
    w = p.walks(torch.arange(321))
    assert w.shape == (321, 8) and torch.equal(w[:, 0], torch.arange(321))
    dense = torch.zeros(321, 321, dtype=torch.bool)
    dense[ei[0], ei[1]] = True
    assert dense[w[:320, :-1], w[:320, 1:]].all() and (w[320] == 320).all()
    losses = [p.train() for _ in range(5)]
    assert losses[-1] < losses[0]
    assert p.get_embedding().shape == (321, 8)


def test_fixture_regenerates_bit_for_bit(tmp_path):
    from tests.golden import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not on this machine")
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.golden.make_golden_dgda", "--out", str(tmp_path)], cwd=root,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    new, old = np.load(tmp_path / "dgda_fit3.npz"), _fixture()
    assert sorted(new.files) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k]), k
