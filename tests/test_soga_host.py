"""SOGA without a GPU: the public surface (signature, defaults, the alias import), the two NotImplementedErrors, the
state-dict keys and init stream, ``soga_samples`` against the tables the reference drew, the host fallbacks of
``soga_smooth_ce`` and ``soga_adapt`` against an independently composed float64 expression (value, autograd gradient
and finite differences), the reverse index of ``soga_plan``, host fits against the fixtures recorded from the
reference's own soga.py (tests/golden/make_golden_soga.py), and the argument checks of gda_soga.hip's C ABI."""
import ctypes
import inspect
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pygda_amd import _lib
from pygda_amd.data import Data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ("soga_fit3_gcn.npz", "soga_fit3_gin.npz", "soga_fit3_gat.npz")
VIEWS = ("struct", "neigh")


def fixture(name):
    f = np.load(os.path.join(HERE, name))
    s = Data(x=torch.from_numpy(f["src_x"]), edge_index=torch.from_numpy(f["src_ei"]), y=torch.from_numpy(f["src_y"]))
    t = Data(x=torch.from_numpy(f["tgt_x"]), edge_index=torch.from_numpy(f["tgt_ei"]), y=torch.from_numpy(f["tgt_y"]))
    return f, s, t


def fixture_tables(f):
    return [tuple(f[f"tables/{k}_{v}"] for k in ("center_nodes", "positive_samples", "negative_samples")) for v in VIEWS]


def run_fit(f, s, t, device, epochs=3, **kw):
    """A fit under the fixture's three seeds; what :func:`check_fit_against_fixture` reads."""
    from pygda_amd.models import SOGA
    m = SOGA(16, 16, int(f["num_classes"]), num_layers=2, lr=4e-3, gnn=str(f["gnn"]), device=device, epoch=epochs,
             verbose=0, record=True, **kw)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    seeds = [int(v) for v in f["seeds"]]
    torch.manual_seed(seeds[0])
    random.seed(seeds[1])
    np.random.seed(seeds[2])
    m.fit(s, t)
    got = dict(src_losses=np.array([l for l, a in log if a is not None]),
               accs=np.array([a for _, a in log if a is not None]),
               tgt_losses=np.array([l for l, a in log if a is None]), parts=np.array(m.parts_log),
               src_logits=m.predict(s)[0].double().cpu().numpy(), tgt_logits=m.predict(t)[0].double().cpu().numpy())
    got.update({"final/" + k: v.double().cpu().numpy() for k, v in m.soga.state_dict().items()})
    got["tables"] = [tuple(getattr(m.soga, f"{k}_{v}").numpy() for k in ("center_nodes", "positive_samples",
                                                                          "negative_samples")) for v in VIEWS]
    return m, got


def check_fit_against_fixture(got, f):
    """Every recorded figure of a fit -- the pretraining losses, the adaptation losses and their four parts, both
    predict outputs and the final parameters -- is held against the fixture's own float32-versus-float64 distance:

        |ours - f64| <= 8 |reference fp32 - f64| + 1e-6 max(|f64|, 1)        (max norm per figure)

    and each figure is printed before it is asserted.  The multiple: ours and the reference's float32 run are two
    roundings of the same expressions, so their errors against float64 come from one distribution, but a figure here is
    the max over as few as three numbers (the per-epoch losses).  The ratio of two such maxima is not close to 1: the
    reference's can fall to a third of the common scale while ours reaches 2.5 times it, each with a chance of about
    one in a hundred, which is the factor 8 that the GPU tests' ``_close`` (tests/test_gpu_acdne.py) uses for the
    same reason.  The floor is DMGNN's: 16 float32 ulps of the figure's magnitude, for a figure the reference happens to
    hit exactly.  The source accuracies are arg-max counts on rows whose top-2 gap is at least 1e-4: equal."""
    keys = ["src_losses", "tgt_losses", "parts", "src_logits", "tgt_logits"] + [k for k in f.files if k.startswith("final/")]
    for k in keys:
        f64, ref32 = f["f64/" + k].astype(np.float64), f[k].astype(np.float64)
        floor = 1e-6 * max(np.abs(f64).max(), 1.0)
        err, lim = np.abs(got[k] - f64).max(), 8 * np.abs(ref32 - f64).max() + floor
        print(f"{k}: |ours - f64| = {err:.3e}, |ref fp32 - f64| = {np.abs(ref32 - f64).max():.3e}, bound {lim:.3e}")
        assert err <= lim, f"{k}: {err:.3e} > {lim:.3e}"
    np.testing.assert_array_equal(got["accs"], f["accs"])
    for ours, theirs in zip(got["tables"], fixture_tables(f)):
        for a, b in zip(ours, theirs):
            np.testing.assert_array_equal(a, b)


# -- the public surface ---------------------------------------------------------------------------------------------------
def test_signature_defaults_and_alias():
    from pygda.models import SOGA as Alias
    from pygda.nn import SOGABase as AliasBase
    from pygda_amd.models import SOGA, BaseGDA
    from pygda_amd.nn import SOGABase
    import pygda
    assert Alias is SOGA and AliasBase is SOGABase and issubclass(SOGA, BaseGDA) and "SOGA" in pygda.__doc__
    sig = inspect.signature(SOGA.__init__)
    want = dict(num_layers=3, dropout=0., act=F.relu, num_negative_samples=5, num_positive_samples=2, struct_lambda=1.0,
                neigh_lambda=1.0, weight_decay=0., lr=4e-3, epoch=200, gnn='gcn', device='cuda:0', batch_size=0,
                num_neigh=-1, verbose=2)
    names = list(sig.parameters)
    assert names[:4] == ["self", "in_dim", "hid_dim", "num_classes"]
    assert names[4:-1] == list(want) and names[-1] == "kwargs"
    for k, v in want.items():
        assert sig.parameters[k].default == v, k
    bsig = inspect.signature(SOGABase.__init__)
    assert bsig.parameters["num_layers"].default == 1 and bsig.parameters["dropout"].default == 0.1
    for name in ("init_model", "forward_model", "fit", "predict", "process_graph", "NCE_loss", "ent", "div"):
        assert callable(getattr(SOGA, name)), name


def test_unsupported_arguments_raise_not_implemented():
    from pygda_amd.models import SOGA
    with pytest.raises(NotImplementedError, match="batch_size"):
        SOGA(16, 16, 3, batch_size=64)
    with pytest.raises(NotImplementedError, match="num_positive_samples"):
        SOGA(16, 16, 3, num_positive_samples=3)
    SOGA(16, 16, 3, device="cpu")


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_and_init_stream(name):
    from pygda_amd.models import SOGA
    f, _, _ = fixture(name)
    m = SOGA(16, 16, int(f["num_classes"]), num_layers=2, gnn=str(f["gnn"]), device="cpu")
    torch.manual_seed(int(f["seeds"][0]))
    net = m.init_model()
    assert sorted(net.state_dict()) == sorted(k[5:] for k in f.files if k.startswith("init/"))
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), f["init/" + k]), k


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_conditions(name):
    f, s, t = fixture(name)
    assert min(f["gaps"].min(), f["f64/gaps"].min()) >= 1e-4 and np.array_equal(f["accs"], f["f64/accs"])
    assert s.x.shape == (300, 16) and t.x.shape == (260, 16) and f["parts"].shape == (3, 4)
    ei = f["tgt_ei"]
    assert 259 not in ei                                                   # the isolated node
    assert (ei[0] == ei[1]).any()                                          # a self loop
    pairs = set(map(tuple, ei.T.tolist()))
    assert len(pairs) < ei.shape[1]                                        # a duplicate edge
    assert any((v, u) not in pairs for u, v in pairs if u != v)            # a directed-only edge
    np.testing.assert_allclose(f["parts"][:, 0], f["parts"][:, 1] + f["parts"][:, 2] + f["parts"][:, 3], rtol=1e-6)


# -- the sample tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_soga_samples_reproduces_the_reference_tables(name):
    from pygda_amd.utils.sampler import soga_samples
    f, _, t = fixture(name)
    random.seed(int(f["seeds"][1]))
    np.random.seed(int(f["seeds"][2]))
    views = soga_samples(t.edge_index, 260, 5)
    assert len(views) == 2
    for ours, theirs in zip(views, fixture_tables(f)):
        for a, b in zip(ours, theirs):
            assert a.dtype == np.int64 and a.shape == b.shape
            np.testing.assert_array_equal(a, b)
    cen, pos, _ = views[0]
    assert sorted(cen[:, 0].tolist()) == list(range(260))                  # one walk per node, in shuffled order
    row = cen[:, 0].tolist().index(259)
    assert pos[row, 0] == 259                                              # the isolated node is its own positive


# -- the host fallbacks against an independent composition (loops over rows, float64 autograd) ------------------------------
def _tables(n, m, k, v, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, n, (m, 1), generator=g), torch.randint(0, n, (m, 1), generator=g),
             torch.randint(0, n, (m, k), generator=g)) for _ in range(v)]


def independent_adapt(z, tables, lams):
    n = z.size(0)
    p = torch.exp(z - torch.logsumexp(z, dim=1, keepdim=True))
    ent = sum(-(r * torch.log(r + 1e-5)).sum() for r in p) / n
    mean = sum(r for r in p) / n
    im = ent + (mean * torch.log(mean + 1e-8)).sum()
    nce = []
    for cen, pos, neg in tables:
        rows = []
        for i in range(cen.size(0)):
            c = p[int(cen[i, 0])]
            den = sum(torch.exp((c * p[int(j)]).sum()) for j in neg[i])
            rows.append(torch.log(den) - (c * p[int(pos[i, 0])]).sum())
        nce.append(sum(rows) / len(rows))
    total = im + sum(l * v for l, v in zip(lams, nce))
    return total, [total, im] + nce + [torch.zeros((), dtype=z.dtype)] * (2 - len(nce))


def independent_smooth_ce(z, y, eps):
    c = z.size(1)
    rows = []
    for i in range(z.size(0)):
        logp = z[i] - torch.logsumexp(z[i], dim=0)
        rows.append(-sum(((1 - eps) * (k == int(y[i])) + eps / c) * logp[k] for k in range(c)))
    return sum(rows) / len(rows)


@pytest.mark.parametrize("n,c,k,v", [(7, 3, 2, 2), (23, 5, 4, 1), (40, 2, 3, 2)])
def test_host_fallbacks_against_an_independent_float64_composition(n, c, k, v):
    from pygda_amd import ops
    g = torch.Generator().manual_seed(n + c)
    z = torch.randn(n, c, generator=g, dtype=torch.float64)
    y = torch.randint(0, c, (n,), generator=g)
    tables = _tables(n, n + 3, k, v, n)
    plan = ops.soga_plan(tables, n)
    lams = (0.7, 1.3)
    a, b = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    loss, parts = ops.soga_adapt(a, plan, *lams)
    want, wparts = independent_adapt(b, tables, lams)
    assert abs(loss.item() - want.item()) <= 1e-12
    assert float((parts - torch.stack(wparts).detach()).abs().max()) <= 1e-12
    ga, gb = torch.autograd.grad(loss, a)[0], torch.autograd.grad(want, b)[0]
    assert float((ga - gb).abs().max()) <= 1e-12
    a, b = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    ce, wce = ops.soga_smooth_ce(a, y, 0.1), independent_smooth_ce(b, y, 0.1)
    assert abs(ce.item() - wce.item()) <= 1e-12
    assert float((torch.autograd.grad(ce, a)[0] - torch.autograd.grad(wce, b)[0]).abs().max()) <= 1e-12


def test_host_gradients_against_finite_differences():
    from pygda_amd import ops
    n, c, k = 7, 3, 2
    g = torch.Generator().manual_seed(5)
    z = torch.randn(n, c, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.randint(0, c, (n,), generator=g)
    plan = ops.soga_plan(_tables(n, n, k, 2, 9), n)
    assert torch.autograd.gradcheck(lambda x: ops.soga_adapt(x, plan, 0.7, 1.3)[0], (z,), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda x: ops.soga_smooth_ce(x, y, 0.1), (z,), eps=1e-6, atol=1e-7)


# -- the reverse index ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segment", [16, 64])
def test_reverse_index_lists_every_entry_once_under_its_node(segment):
    from pygda_amd import ops
    n, m, k, v = 37, 41, 5, 2
    tables = _tables(n, m, k, v, 3)
    for cen, pos, neg in tables:
        neg[:, 1] = 4                                                      # a hub: a negative of every row
        cen[cen == 11] = 12
        pos[pos == 11] = 12
        neg[neg == 11] = 12                                                # node 11 in no role
    plan = ops.soga_plan(tables, n, segment=segment)
    assert (plan.n, plan.m, plan.k, plan.v, plan.segment) == (n, m, k, v, segment)
    assert plan.rev_ptr.shape == (n + 1,) and plan.rev_ptr[0] == 0 and plan.rev_ptr[-1] == v * m * (k + 2) == plan.nrev
    assert plan.rev_ptr[12] == plan.rev_ptr[11]
    seen = set()
    for j in range(n):
        last = None
        for q in range(plan.rev_ptr[j], plan.rev_ptr[j + 1]):
            view, row, code = int(plan.rev_row[q]) // m, int(plan.rev_row[q]) % m, int(plan.rev_code[q])
            cen, pos, neg = tables[view]
            named = cen[row, 0] if code == 0 else pos[row, 0] if code == 1 else neg[row, code - 2]
            assert int(named) == j
            key = (view, row, code)
            assert key not in seen and (last is None or key > last)
            seen.add(key)
            last = key
            src, sig = int(plan.rev_src[q]), int(plan.rev_sig[q])
            assert src == (view * m + row if code == 0 else int(cen[row, 0]))
            assert sig == ((view * m + row) * k + code - 2 if code >= 2 else (-1 - view if code == 1 else -3 - view))
    assert len(seen) == v * m * (k + 2)
    seg_off, node_seg = plan.seg_off.numpy(), plan.node_seg.numpy()
    assert seg_off[0] == 0 and seg_off[-1] == plan.nrev and len(seg_off) == plan.nseg + 1 and node_seg[-1] == plan.nseg
    assert plan.nseg <= n + plan.nrev // ops.SOGA_MIN_SEGMENT
    for j in range(n):
        offs = seg_off[node_seg[j]:node_seg[j + 1] + 1] if node_seg[j + 1] > node_seg[j] else []
        if len(offs):
            assert offs[0] == plan.rev_ptr[j] and offs[-1] == plan.rev_ptr[j + 1]
            assert (np.diff(offs) <= segment).all() and (np.diff(offs)[:-1] == segment).all()
        else:
            assert plan.rev_ptr[j] == plan.rev_ptr[j + 1]
    assert node_seg[5] - node_seg[4] >= 2 * m // segment                  # the hub's list spans several segments


def test_plan_rejects_bad_tables():
    from pygda_amd import ops
    t = _tables(10, 10, 3, 2, 1)
    bad = [(t[0][0], t[0][1], t[0][2].clone())] + t[1:]
    bad[0][2][3, 1] = 10
    with pytest.raises(_lib.GdaError, match=r"outside \[0, 10\)"):
        ops.soga_plan(bad, 10)
    with pytest.raises(_lib.GdaError, match="K mismatch"):
        ops.soga_plan([t[0], (t[1][0], t[1][1], t[1][2][:, :2])], 10)
    with pytest.raises(_lib.GdaError, match="one or two views"):
        ops.soga_plan(t + t[:1], 10)
    plan = ops.soga_plan(t, 10)
    with pytest.raises(_lib.GdaError, match="logits"):
        ops.soga_adapt(torch.zeros(9, 3), plan)


# -- host fits against the reference's fixtures -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_fit_matches_the_reference(name):
    f, s, t = fixture(name)
    m, got = run_fit(f, s, t, "cpu")
    assert len(got["src_losses"]) == 3 and len(got["tgt_losses"]) == 3
    check_fit_against_fixture(got, f)


# -- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_soga_entries_validate_before_touching_a_device():
    L = _lib.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)                      # never dereferenced
    n, c, m, k, v = 100, 5, 100, 5, 2
    nrev = v * m * (k + 2)
    assert L.gda_soga_workspace_bytes(n, c, m, k, v) >= 4 * (n * 8 + v * m * (k + 8))
    big = 1 << 30

    def adapt(n=n, c=c, m=m, k=k, v=v, nrev=nrev, nseg=n, logits=p, ws=p, wsb=big, neg=p):
        return L.gda_soga_adapt_f32(logits, n, c, p, p, neg, v, m, k, 1.0, 1.0, p, p, nseg, p, p, nrev, p, p, ws, wsb,
                                    None)

    assert adapt(c=65) == -4                                               # classes over the limit
    assert adapt(n=0) == -2 and adapt(k=0) == -2 and adapt(v=3) == -2
    assert adapt(nrev=v * m * (k + 1)) == -2                               # a reverse index built for another K
    assert adapt(nseg=n + nrev // 16 + 2) == -2                            # more segments than the contract allows
    assert adapt(logits=None) == -1 and adapt(neg=None) == -1
    assert adapt(logits=odd) == -4 and adapt(neg=odd) == -4                # misaligned buffers
    assert adapt(ws=ctypes.c_void_p(72)) == -4                             # the workspace wants 16 bytes
    assert adapt(wsb=64) == -3

    def ce(n=n, c=c, logits=p, labels=p, wsb=big):
        return L.gda_soga_smooth_ce_f32(logits, labels, n, c, 0.1, p, p, None, p, wsb, None)

    assert ce(c=65) == -4 and ce(n=0) == -2 and ce(logits=None) == -1 and ce(logits=odd) == -4
    assert ce(labels=ctypes.c_void_p(68)) == -4 and ce(wsb=4) == -3
    for name in ("gda_soga_ce_workspace_bytes", "gda_soga_smooth_ce_f32", "gda_soga_workspace_bytes",
                 "gda_soga_adapt_f32"):
        assert name in _lib.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "gda_hip.h")).read()
    assert "#define GDA_SOGA_MAX_CLASSES 64" in header and "#define GDA_SOGA_MIN_SEGMENT 16" in header
    with pytest.raises(_lib.GdaError, match="gda_soga_adapt_f32"):
        _lib.call("gda_soga_adapt_f32", p, n, 65, p, p, p, v, m, k, 1.0, 1.0, p, p, n, p, p, nrev, p, p, p, big, None)


def test_fixture_regenerates_bit_for_bit(tmp_path):
    from tests.golden import _ref_loader
    if not _ref_loader.available():
        pytest.skip("needs the reference checkout (build container only)")
    pytest.importorskip("networkx")
    import subprocess
    import sys
    subprocess.run([sys.executable, "-m", "tests.golden.make_golden_soga", "--out", str(tmp_path)], cwd=ROOT, check=True,
                   env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), stdout=subprocess.DEVNULL)
    for name in FIXTURES:
        a, b = np.load(os.path.join(HERE, name)), np.load(os.path.join(str(tmp_path), name))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), (name, k)
