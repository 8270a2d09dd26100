"""SEPA without a GPU: the public surface (signature, defaults, the alias import, ``PageRank``), the rejections raised
before any device work, the state-dict keys and init stream, the conditions the fixtures were recorded under, host fits
against the fixtures recorded from the reference's own sepa.py (tests/golden/make_golden_sepa.py), each loss method and
``PageRank.forward`` against float64 autograd of an independently composed expression, and the C ABI of gda_sepa.hip."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pygda_amd import _lib
from pygda_amd.data import Data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ("sepa_fit3_gcn.npz", "sepa_fit3_gat.npz", "sepa_fit3_gin_empty.npz")


def _fixture(name):
    f = np.load(os.path.join(HERE, name))
    s = Data(x=torch.from_numpy(f["src_x"]), edge_index=torch.from_numpy(f["src_ei"]), y=torch.from_numpy(f["src_y"]))
    t = Data(x=torch.from_numpy(f["tgt_x"]), edge_index=torch.from_numpy(f["tgt_ei"]), y=torch.from_numpy(f["tgt_y"]))
    return f, s, t


def _model(f, **kw):
    from pygda_amd.models import SEPA
    return SEPA(16, 16, int(f["num_classes"]), num_layers=2, lr=4e-3, gnn=str(f["gnn"]), verbose=0, **kw)


def test_signature_defaults_alias_and_pagerank():
    from pygda.models import SEPA as Alias
    from pygda_amd.models import SEPA
    from pygda_amd.nn import PageRank
    assert Alias is SEPA
    sig = inspect.signature(SEPA.__init__)
    want = dict(num_layers=2, dropout=0., gnn='gcn', lamda_im=0.2, lamda_pp=0.1, lamda_sep=1.0, tau=1.5, act=F.relu,
                weight_decay=0.01, lr=0.001, epoch=200, device='cuda:0', batch_size=0, num_neigh=-1, verbose=2)
    for k, v in want.items():
        assert sig.parameters[k].default == v, k
    assert list(sig.parameters)[:4] == ["self", "in_dim", "hid_dim", "num_classes"]
    m = SEPA(16, 16, 3, device="cpu")
    assert m.gnn == "gcn" and isinstance(m.pagerank, PageRank) and (m.pagerank.k, m.pagerank.alpha) == (5, 0.9)
    assert list(inspect.signature(PageRank.forward).parameters) == ["self", "x", "edge_index", "edge_weight"]
    for name in ("init_model", "forward_model", "fit", "predict", "process_graph", "cls_im", "obtain_source_prototype",
                 "obtain_target_prototype", "seperate_center", "proto_alignment"):
        assert callable(getattr(m, name)), name


def test_rejections_before_device_work():
    from pygda_amd.models import SEPA
    with pytest.raises(ValueError, match="full-batch"):
        SEPA(16, 16, 3, batch_size=64, device="cuda:0")
    with pytest.raises(ValueError, match="classes"):
        SEPA(16, 16, 33, device="cuda:0")
    with pytest.raises(ValueError, match="hidden widths"):
        SEPA(16, 1025, 3, device="cuda:0")
    SEPA(16, 1025, 33, device="cpu")
    f, s, t = _fixture("sepa_fit3_gcn.npz")
    m = SEPA(16, 16, 4, device="cuda:0", epoch=1, verbose=0)         # labels 0..2 only: class 3 has no node
    with pytest.raises(ValueError, match="class 3"):
        m.fit(s, t)
    y = s.y.clone()
    y[y == 1] = 0
    with pytest.raises(ValueError, match="class 1"):
        SEPA(16, 16, 3, device="cuda:0", epoch=1, verbose=0).fit(Data(x=s.x, edge_index=s.edge_index, y=y), t)


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_and_init_stream(name):
    f, _, _ = _fixture(name)
    m = _model(f, device="cpu")
    torch.manual_seed(int(f["init_seed"]))
    net = m.init_model()
    keys = sorted(k[5:] for k in f.files if k.startswith("init/"))
    assert sorted(net.state_dict()) == keys
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), f["init/" + k]), k


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_conditions(name):
    f, _, _ = _fixture(name)
    assert np.array_equal(f["pred"], f["f64/pred"])                   # no node on a class boundary in either run
    assert min(f["gaps"].min(), f["f64/gaps"].min()) >= 1e-4
    assert f["pred"].shape == (3, 260) and np.isfinite(f["losses"]).all()
    if name == "sepa_fit3_gcn.npz":
        assert (f["n_pred"] == int(f["num_classes"])).all()
    if name == "sepa_fit3_gin_empty.npz":
        assert (f["n_pred"] < int(f["num_classes"])).any()            # some class predicted by no node in some epoch


@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_fit_matches_the_reference(name):
    f, s, t = _fixture(name)
    m = _model(f, device="cpu", epoch=3, record=True)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    torch.manual_seed(int(f["init_seed"]))
    assert m.gnn == str(f["gnn"])
    m.fit(s, t)
    assert np.allclose([l for l, _ in log], f["losses"], rtol=1e-6, atol=0)
    assert np.allclose([a for _, a in log], f["accs"], rtol=0, atol=1e-12)
    assert np.allclose(np.array(m.parts_log), f["parts"], rtol=1e-6, atol=1e-9)
    for p, q in zip(m.pred_log, f["pred"]):
        assert np.array_equal(p.numpy(), q)
    for k, v in m.gnn.state_dict().items():
        assert np.allclose(v.numpy(), f["final/" + k], rtol=1e-4, atol=1e-5), k
    for data, key in ((s, "src_logits"), (t, "tgt_logits")):
        assert np.allclose(m.predict(data)[0].numpy(), f[key], rtol=1e-4, atol=1e-5), key


# -- the loss methods against an independent composition (loops over classes and nodes, float64 autograd) --------------
def _unit(v):
    return v / torch.sqrt((v * v).sum()).clamp(min=1e-12)


def _dense_ppr(x, ei, k=5, alpha=0.9):
    n = x.size(0)
    A = torch.zeros(n, n, dtype=x.dtype)
    for r, c in ei.t().tolist():
        if r != c:
            A[c, r] += 1.0
    A = A + torch.eye(n, dtype=x.dtype)
    dis = A.sum(1).pow(-0.5)
    A = dis[:, None] * A * dis[None, :]
    cur = x
    for _ in range(k):
        cur = (1 - alpha) * (A @ cur) + alpha * x
    return cur


def _independent(prob, feat, fs, ys, ei, C, tau, pred):
    n = prob.size(0)
    mean = prob.sum(0) / n
    ent = torch.stack([-(p * torch.log(p + 1e-12)).sum() for p in prob])
    im = (mean * torch.log(mean + 1e-12)).sum() + ent.sum() / n
    sp = torch.stack([fs[ys == c].sum(0) / int((ys == c).sum()) for c in range(C)])
    members = [(pred == c).nonzero().flatten() for c in range(C)]
    biased = torch.stack([feat[ix].sum(0) / (len(ix) + 1e-12) for ix in members])
    rows = []
    for c, ix in enumerate(members):
        r = prob[ix].sum(0) / len(ix) if len(ix) else torch.zeros(C, dtype=prob.dtype)
        mask = torch.ones(C, dtype=prob.dtype)
        mask[c] = 0
        rows.append(_unit(r * mask))
    M = torch.stack(rows)
    U = []
    for i in range(n):
        w = _unit(prob[i] * M[pred[i]])
        U.append((w[:, None] * biased).sum(0) / (w + 1e-12).sum() - biased[pred[i]])
    R = _dense_ppr(torch.stack(U), ei)
    T = torch.stack([biased[pred[i]] + ent[i] * _unit(R[i]) for i in range(n)])
    tp = torch.stack([T[ix].sum(0) / (len(ix) + 1e-12) if len(ix) else torch.zeros_like(T[0]) for ix in members])

    def expcos(a, b):
        return torch.exp(torch.stack([torch.stack([(_unit(x) * _unit(y)).sum() for y in b]) for x in a]) / tau)

    ts, tt, ss, pp_ = expcos(tp + 1e-6, sp + 1e-6), expcos(tp + 1e-6, tp + 1e-6), expcos(sp + 1e-6, sp + 1e-6), expcos(sp, sp)
    off = 1 - torch.eye(C, dtype=prob.dtype)
    den = ((ts + tt + ss) * off).sum(1)
    pp = -torch.log((ts.diagonal() / den.clamp(min=1e-6)).clamp(min=1e-6)).sum() / C
    sep = torch.log((pp_ * off).sum(1) / (C - 1) + 1e-8).sum() / C
    return im, pp, sep


@pytest.mark.parametrize("C,empty", [(3, False), (5, True), (2, False)])
def test_loss_methods_against_an_independent_float64_composition(C, empty):
    from pygda_amd.models import SEPA
    g = torch.Generator().manual_seed(40 + C)
    n, ns, h = 41, 30, 6
    z = torch.randn(n, C, generator=g, dtype=torch.float64)
    if empty:
        z[:, C - 1] -= 10.0
    z[torch.arange(n), z.argmax(1)] += 0.5
    feat = torch.randn(n, h, generator=g, dtype=torch.float64)
    fs = torch.randn(ns, h, generator=g, dtype=torch.float64)
    ys = torch.randint(0, C, (ns,), generator=g)
    ys[:C] = torch.arange(C)
    src, dst = torch.randint(0, n, (80,), generator=g), torch.randint(0, n, (80,), generator=g)
    keep = (src != 1) & (dst != 1) & (src != dst)                       # node 1 isolated; directed, with duplicates
    ei = torch.stack([torch.cat([src[keep], src[keep][:2]]), torch.cat([dst[keep], dst[keep][:2]])])
    m = SEPA(h, h, C, device="cpu", tau=1.3)

    def ours(z, feat, fs):
        prob = F.softmax(z, dim=1)
        im, _, _, ent = m.cls_im(prob)
        sp = m.obtain_source_prototype(fs, ys)
        return im, m.proto_alignment(m.obtain_target_prototype(prob, feat, ei, ent), sp), m.seperate_center(sp, fs, ys)

    def theirs(z, feat, fs):
        prob = torch.exp(z - torch.logsumexp(z, dim=1, keepdim=True))
        return _independent(prob, feat, fs, ys, ei, C, 1.3, z.detach().argmax(1))

    pred = z.argmax(1)
    assert (torch.unique(pred).numel() < C) == empty
    for i in range(3):
        a = [v.clone().requires_grad_(True) for v in (z, feat, fs)]
        b = [v.clone().requires_grad_(True) for v in (z, feat, fs)]
        va, vb = ours(*a)[i], theirs(*b)[i]
        assert abs(va.item() - vb.item()) <= 1e-12, (i, va.item(), vb.item())
        ga = torch.autograd.grad(va, a, allow_unused=True)
        gb = torch.autograd.grad(vb, b, allow_unused=True)
        for x, y in zip(ga, gb):
            assert (x is None) == (y is None)
            if x is not None:
                assert float((x - y).abs().max()) <= 1e-12, i


def test_pagerank_forward_on_a_graph_with_an_isolated_node():
    from pygda_amd.nn import PageRank
    ei = torch.tensor([[0, 2, 2, 3, 0, 4], [2, 0, 3, 2, 2, 0]])          # node 1 isolated, 0 -> 2 twice, 4 -> 0 directed
    x = torch.randn(5, 3, dtype=torch.float64, requires_grad=True)
    y = x.detach().clone().requires_grad_(True)
    a, b = PageRank()(x, ei), _dense_ppr(y, ei)
    assert float((a - b).abs().max()) <= 1e-12
    up = torch.randn(5, 3, dtype=torch.float64)
    ga, gb = torch.autograd.grad((a * up).sum(), x)[0], torch.autograd.grad((b * up).sum(), y)[0]
    assert float((ga - gb).abs().max()) <= 1e-12


# -- the C ABI -------------------------------------------------------------------------------------------------------------
def _declared():
    header = open(os.path.join(ROOT, "include", "gda_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(gda_sepa_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", header, flags=re.S):
        out[name] = len([a for a in args.split(",") if a.strip()])
    return out


def test_every_sepa_entry_is_bound_with_the_declared_argument_count():
    decl = _declared()
    assert len(decl) == 12, sorted(decl)
    L = _lib.lib()
    for name, nargs in decl.items():
        assert name in _lib.EXPORTED_SYMBOLS and len(getattr(L, name).argtypes) == nargs, name
    src = open(os.path.join(ROOT, "include", "gda_hip.h")).read()
    assert "#define GDA_SEPA_MAX_CLASSES 32" in src and "#define GDA_SEPA_MAX_WIDTH 1024" in src
    from pygda_amd import ops
    assert (ops.SEPA_MAX_CLASSES, ops.SEPA_MAX_WIDTH) == (32, 1024)


def test_sepa_entries_validate_before_touching_a_device():
    L = _lib.lib()
    p = ctypes.c_void_p(64)                                               # never dereferenced
    assert L.gda_sepa_workspace_bytes(5484, 5, 128) >= 86 * 5 * 129 * 4
    calls = {
        "stats": lambda n=10, C=5, Z=p: L.gda_sepa_stats_f32(Z, n, C, p, p, p, None),
        "group_sum": lambda n=10, C=5, d=16, X=p, wsb=1 << 20: L.gda_sepa_group_sum_f32(X, d, p, None, n, d, C, 1, 0.0,
                                                                                       None, p, p, p, wsb, None),
        "class_mean_bwd": lambda n=10, C=5, d=16, G=p: L.gda_sepa_class_mean_bwd_f32(G, p, p, None, n, d, C, 0.0, p, None),
        "mid": lambda n=10, C=5, d=16, X=p: L.gda_sepa_mid_f32(X, p, p, p, n, C, d, p, p, p, None),
        "unbias": lambda n=10, C=5, d=16, X=p: L.gda_sepa_unbias_rows_f32(X, p, p, p, n, C, d, p, None),
        "center_bwd": lambda n=10, C=5, d=16, X=p: L.gda_sepa_center_rows_bwd_f32(X, p, p, p, p, None, n, C, d,
                                                                                 ctypes.c_void_p(128), p, None),
        "unbias_bwd": lambda n=10, C=5, d=16, X=p, wsb=1 << 20: L.gda_sepa_unbias_rows_bwd_f32(X, p, p, p, p, n, C, d, p,
                                                                                             p, p, p, wsb, None),
        "mid_bwd": lambda n=10, C=5, d=16, X=p: L.gda_sepa_mid_bwd_f32(X, p, p, p, p, None, 0.2, n, C, d, p, p, p, None),
    }
    for name, fn in calls.items():
        assert fn(n=0) == -2, name                                        # no rows
        assert fn(C=33) == -4, name                                       # classes over the limit
        assert fn(**({"Z": None} if name == "stats" else {"G": None} if name == "class_mean_bwd" else {"X": None})) == -1
        if name != "stats":
            assert fn(d=1025) == -4, name                                 # width over the limit
    assert calls["group_sum"](wsb=16) == -3 and calls["unbias_bwd"](wsb=16) == -3
    assert L.gda_sepa_row_weight_f32(None, p, 10, 16, p, None) == -1 and L.gda_sepa_row_weight_f32(p, p, 0, 16, p, None) == -2
    assert L.gda_sepa_row_weight_f32(p, p, 10, 1025, p, None) == -4
    assert L.gda_sepa_dz_rows_f32(p, p, p, p, p, p, 0, 5, p, None) == -2
    assert L.gda_sepa_dz_rows_f32(p, p, p, p, p, p, 10, 33, p, None) == -4
    assert L.gda_sepa_dz_rows_f32(None, p, p, p, p, p, 10, 5, p, None) == -1
    q, r = ctypes.c_void_p(128), ctypes.c_void_p(192)
    assert L.gda_sepa_proto_f32(None, p, 5, 16, 1.5, 0.1, 1.0, p, q, r, None) == -1
    assert L.gda_sepa_proto_f32(p, q, 33, 16, 1.5, 0.1, 1.0, p, r, r, None) == -4
    assert L.gda_sepa_proto_f32(p, q, 5, 1025, 1.5, 0.1, 1.0, p, r, r, None) == -4
    assert L.gda_sepa_proto_f32(p, q, 0, 16, 1.5, 0.1, 1.0, p, r, r, None) == -2
    assert L.gda_sepa_proto_f32(p, q, 5, 16, 0.0, 0.1, 1.0, p, r, r, None) == -2
    assert L.gda_sepa_proto_f32(p, q, 5, 16, 1.5, 0.1, 1.0, p, r, None, None) == -1      # one gradient without the other
    assert L.gda_sepa_proto_f32(p, q, 5, 16, 1.5, 0.1, 1.0, r, p, r, None) == -5         # dT aliases T


def test_fixture_regenerates_bit_for_bit(tmp_path):
    from tests.golden import _ref_loader
    if not _ref_loader.available():
        pytest.skip("needs the reference checkout (build container only)")
    import subprocess
    import sys
    subprocess.run([sys.executable, "-m", "tests.golden.make_golden_sepa", "--out", str(tmp_path)], cwd=ROOT, check=True,
                   env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), stdout=subprocess.DEVNULL)
    for name in FIXTURES:
        a, b = np.load(os.path.join(HERE, name)), np.load(os.path.join(str(tmp_path), name))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), (name, k)
