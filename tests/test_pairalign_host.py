"""CPU: PairAlign's solver, host path, schedules and surface against the fixture ``pairalign_fit.npz`` (the reference's
own ``pa.py`` run on the PyG stub, tests/golden/make_golden_pairalign.py).

Bounds.  The layers apply the linear map before the aggregation and the statistics are summed in float64, so the host
fit has fp32-rounding parity with the record, not bit parity: losses, logits and parameters are held to
``rtol = atol = 1e-5`` and per-edge weights to ``1e-6``, the bounds tests/test_oracle_golden.py
(``test_strurw_fit_trajectory``) uses for the same ``ReweightGNN`` layers.  The class-pair table ``ew`` and the label
weights ``lw`` are solutions of programs whose data are those fp32 logits; they take the logits' ``1e-5``."""
import numpy as np
import pytest
import torch

from pygda_amd import _build, _lib, ops
from pygda_amd.data import Data
from pygda_amd.models import PairAlign
from pygda_amd.models.pairalign import ratio_weight
from pygda_amd.qp import solve_simplex_ls
from tests.conftest import T, load_golden, sub

TOL, EDGE_TOL = 1e-5, 1e-6
FITS = dict(GS=(dict(backbone="GS", weight_CE_src=True), 12), GCN=(dict(backbone="GCN", weight_CE_src=False), 6))
COMMON = dict(cls_dim=8, dropout=0.0, lr=0.02, weight_decay=1e-4, ew_freq=3, lw_freq=4, label_rw=True, edge_rw=True)


@pytest.fixture(scope="module")
def G():
    return load_golden("pairalign_fit")


def pair(g, device="cpu", dtype=torch.float32):
    s = Data(x=T(g["src_x"]).to(dtype), edge_index=T(g["src_ei"]), y=T(g["src_y"]), train_mask=T(g["src_mask"]))
    t = Data(x=T(g["tgt_x"]).to(dtype), edge_index=T(g["tgt_ei"]), y=T(g["tgt_y"]))
    s.edge_weight = t.edge_weight = None
    return s.to(device), t.to(device)


def trainer(g, tag, device="cpu", **over):
    kw, epochs = FITS[tag]
    cfg = dict(COMMON, epoch=epochs, device=device, verbose=0, **kw)
    cfg.update(over)
    return PairAlign(16, 16, 4, **cfg)


def run_fit(g, tag, device="cpu", dtype=torch.float32, m=None, **over):
    """A fit from the recorded seed: ``(trainer, source, target, log)`` with ``log[e] = (loss, acc, ew, lw,
    edge_weight)`` as they stand once epoch ``e`` is complete."""
    s, t = pair(g, device, dtype)
    m = m or trainer(g, tag, device, **over)
    log = []
    m.epoch_hook = lambda e, loss, acc, secs: log.append(
        (loss, acc, np.array(s.ew, dtype=np.float64), np.array(s.lw, dtype=np.float64),
         s.edge_weight.detach().cpu().numpy().copy()))
    torch.manual_seed(int(g["init_seed"]))
    m.fit(s, t)
    return m, s, t, log


def certificate(cov, m, mu, lam, x):
    """The KKT conditions of ``min |cov x - m|^2 + lam |x - 1|^2, mu . x = 1, x >= 0`` at ``x``, relative to the
    gradient's scale: ``(stationarity on the support with one multiplier, most negative reduced gradient off it,
    |mu . x - 1|, min x)``.  The program is strictly convex: the point that passes is THE solution."""
    grad = 2.0 * cov.T @ (cov @ x - m) + 2.0 * lam * (x - 1.0)
    scale = max(1.0, float(np.abs(2.0 * cov.T @ m + 2.0 * lam).max()))
    sup = x > 0
    nu = -float(grad[sup] @ mu[sup]) / float(mu[sup] @ mu[sup])
    red = (grad + nu * mu) / scale
    return float(np.abs(red[sup]).max()), float(min(red[~sup].min(), 0.0)) if (~sup).any() else 0.0, \
        abs(float(mu @ x) - 1.0), float(x.min())


def passes(cert):
    stat, off, eq, low = cert
    return stat <= 1e-10 and off >= -1e-10 and eq <= 1e-12 and low >= 0.0


def recorded_solves(g, tag):
    for i in range(int(g[f"{tag}/n_solves"])):
        r = sub(g, f"{tag}/solve/{i}/")
        yield str(r["kind"]), int(r["epoch"]), r["cov"], r["m"], r["mu"], float(r["lam"]), r["x"]


# ---------------------------------------------------------------------------------------------------------- solver --
@pytest.mark.parametrize("tag", ["GS", "GCN"])
def test_recorded_solutions_are_certified_and_reproduced(G, tag):
    seen = 0
    for kind, epoch, cov, m, mu, lam, x in recorded_solves(G, tag):
        assert passes(certificate(cov, m, mu, lam, x)), (kind, epoch, certificate(cov, m, mu, lam, x))
        assert np.abs(solve_simplex_ls(cov, m, mu, lam) - x).max() <= 1e-8, (kind, epoch)
        seen += 1
    assert seen == int(G[f"{tag}/n_solves"]) > 0


def random_program(n, seed, absent=False, sparse=False):
    rng = np.random.default_rng(seed)
    cov = rng.random((n, n)) * (0.1 if not sparse else 1.0)
    mu = rng.random(n)
    if absent and n > 2:                       # class pairs without a source edge: a zero column and a zero mu entry
        mu[::3] = 0.0
        cov[:, ::3] = 0.0
    mu /= mu.sum()
    m = rng.random(n) * (5.0 if sparse else 0.1)
    return cov, m, mu


@pytest.mark.parametrize("n,lam,absent,sparse", [(1, 1.0, False, False), (2, 0.005, False, False),
                                                 (9, 1.0, True, False), (25, 0.005, False, True),
                                                 (400, 0.005, True, True), (400, 1.0, False, False)])
def test_solver_passes_the_certificate_on_random_programs(n, lam, absent, sparse):
    cov, m, mu = random_program(n, 100 + n, absent, sparse)
    x = solve_simplex_ls(cov, m, mu, lam)                       # raises where the cap of 10 n iterations is reached
    assert passes(certificate(cov, m, mu, lam, x)), certificate(cov, m, mu, lam, x)
    if absent:
        assert np.all(x[::3] == 1.0)                            # nothing but the regulariser sees those coordinates
    if sparse:
        assert (x == 0).sum() > n // 2 or n < 100               # most coordinates at the bound


def test_solver_cap_raises_and_arguments_are_checked():
    cov, m, mu = random_program(25, 7, sparse=True)
    with pytest.raises(RuntimeError, match="iterations"):
        solve_simplex_ls(cov, m, mu, 0.005, max_iter=2)
    with pytest.raises(ValueError):
        solve_simplex_ls(cov, m, mu, 0.0)
    with pytest.raises(ValueError):
        solve_simplex_ls(cov, m, -mu, 1.0)


# -------------------------------------------------------------------------------------------- fit against the record --
def close(a, b, tol, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    np.testing.assert_allclose(a, np.asarray(b), rtol=tol, atol=tol, err_msg=what)


def check_fit_against_record(g, tag, m, s, t, log, tol=TOL, edge_tol=EDGE_TOL):
    close([l for l, *_ in log], g[f"{tag}/losses"], tol, "losses")
    np.testing.assert_array_equal([a for _, a, *_ in log], g[f"{tag}/accs"])
    close(np.stack([e for _, _, e, _, _ in log]), g[f"{tag}/ew"], tol, "ew")
    close(np.stack([l for _, _, _, l, _ in log]), g[f"{tag}/lw"], tol, "lw")
    close(np.stack([w for *_, w in log]), g[f"{tag}/edge_weight"], max(edge_tol, 0.0), "edge_weight")
    state = m.gnn.state_dict()
    final = sub(g, f"{tag}/final/")
    assert set(final) == set(state)
    for k, v in final.items():
        close(state[k], v, tol, k)
    close(m.predict(s)[0], g[f"{tag}/src_logits"], tol, "predict(source)")
    close(m.predict(t)[0], g[f"{tag}/tgt_logits"], tol, "predict(target)")
    np.testing.assert_array_equal(t.y_hat.cpu().numpy(), g[f"{tag}/y_hat"])


@pytest.mark.parametrize("tag", ["GS", "GCN"])
def test_host_fit_matches_the_reference_record(G, tag):
    s, t = pair(G)
    m = trainer(G, tag)
    m._src_data, m._tgt_data = s, t
    torch.manual_seed(int(G["init_seed"]))
    m._init_fit(m._dom(s, torch.device("cpu")), m._dom(t, torch.device("cpu")))
    for k, v in sub(G, f"{tag}/init/").items():                # the same draws from the same seed
        np.testing.assert_array_equal(m.gnn.state_dict()[k].numpy(), v, err_msg=k)
    m, s, t, log = run_fit(G, tag)
    check_fit_against_record(G, tag, m, s, t, log)
    # the programs solved here are the recorded ones at the epochs whose result is stored
    rec = {(k, e): x for k, e, *_, x in recorded_solves(G, tag)}
    assert len(m.solves) < len(rec)
    epochs = dict(edge=[e for e in range(m.epoch) if m._fires(e)[0]], label=[e for e in range(m.epoch) if m._fires(e)[1]])
    at = dict(edge=0, label=0)
    for kind, cov, mm, mu, lam, x in m.solves:
        e = epochs[kind][at[kind]]
        at[kind] += 1
        close(x, rec[(kind, e)], TOL, f"{kind} program after epoch {e}")


def test_setup_attributes_match_the_record(G):
    m, s, t, _ = run_fit(G, "GS", epoch=1)
    for name, dtype, shape in (("true_ew", np.float64, (4, 4)), ("ew", np.float64, (4, 4)), ("true_lw", np.float32, (4,)),
                               ("true_beta", np.float64, (16,))):
        v = getattr(s, name)
        assert isinstance(v, np.ndarray) and v.dtype == dtype and v.shape == shape, name
    np.testing.assert_allclose(s.true_ew, G["true_ew"], rtol=1e-13)
    np.testing.assert_allclose(s.true_beta, G["true_beta"], rtol=1e-13)
    np.testing.assert_allclose(s.true_lw, G["true_lw"], rtol=1e-6)
    assert s.true_beta[0 * 4 + 3] == 1.0 and s.true_beta[3 * 4 + 1] == 1.0       # the inf and the nan pair
    assert s.lw.shape == (4,) and np.all(s.ew == 1.0)
    assert s.edge_weight.dtype == torch.float32 and s.edge_weight.shape == (s.edge_index.size(1),)
    assert torch.equal(t.edge_weight, torch.ones(t.edge_index.size(1)))
    assert t.y_hat.shape == (t.x.size(0),) and t.y_hat.dtype == torch.int64


# ------------------------------------------------------------------------------------------------------- schedules --
def five_forward_fit(m, s_data, t_data):
    """The reference's epoch, plainly: two forwards, the step, two forwards, the re-weightings (the label program at
    EVERY epoch), and ``predict`` for the log."""
    m._src_data, m._tgt_data = s_data, t_data
    m._check(s_data, t_data)
    s, t = m._dom(s_data, torch.device("cpu")), m._dom(t_data, torch.device("cpu"))
    opt = torch.optim.Adam(m._init_fit(s, t), lr=m.lr, weight_decay=m.weight_decay)
    log = []
    for epoch in range(m.epoch):
        m.gnn.train()
        pred_src, _ = m._forward(s), m._forward(t)
        loss = m._loss(pred_src)
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            pred_src, pred_tgt = m._forward(s), m._forward(t)
        t_data.y_hat = pred_tgt.argmax(dim=1)
        fire_ew, fire_lw = m._fires(epoch)
        if fire_ew:
            m.update_ew(pred_src, pred_tgt)
        label_weight = m.update_lw(pred_src, pred_tgt)
        if fire_lw:
            s_data.lw = label_weight
            m._set_coef()
        logits, labels = m.predict(s_data)
        log.append((loss.item(), float((logits.argmax(dim=1) == labels).sum()) / labels.numel()))
    return log


@pytest.mark.parametrize("tag", ["GS", "GCN"])
def test_one_forward_schedule_equals_the_five_forward_schedule(G, tag):
    m1, s1, t1, log1 = run_fit(G, tag)
    s2, t2 = pair(G)
    m2 = trainer(G, tag)
    torch.manual_seed(int(G["init_seed"]))
    log2 = five_forward_fit(m2, s2, t2)
    assert [(l, a) for l, a, *_ in log1] == log2                                   # same operations: same bits
    for (k, a), b in zip(m1.gnn.state_dict().items(), m2.gnn.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(s1.edge_weight, s2.edge_weight) and np.array_equal(s1.lw, s2.lw)
    assert torch.equal(t1.y_hat, t2.y_hat)
    assert len(m2.solves) > len(m1.solves)


def test_update_lw_skipped_equals_update_lw_every_epoch(G):
    m1, s1, _, log1 = run_fit(G, "GS")
    m3 = trainer(G, "GS")
    m3._lw_every_epoch = True
    m3, s3, _, log3 = run_fit(G, "GS", m=m3)
    assert [(l, a) for l, a, *_ in log1] == [(l, a) for l, a, *_ in log3]
    assert np.array_equal(s1.lw, s3.lw) and torch.equal(s1.edge_weight, s3.edge_weight)
    assert sum(k == "label" for k, *_ in m3.solves) == 12 and sum(k == "label" for k, *_ in m1.solves) == 3


# ------------------------------------------------------------------------------------------- surface and refusals --
def test_alias_signature_and_exports():
    import inspect
    from pygda.models import PairAlign as Alias
    assert Alias is PairAlign
    sig = inspect.signature(PairAlign.__init__).parameters
    want = dict(num_layers=2, cls_dim=128, cls_layers=2, dropout=0., backbone='GS', pooling='mean',
                ew_type='pseudobeta', rw_lmda=1.0, ls_lambda=1.0, lw_lambda=0.005, label_rw=False, edge_rw=False,
                ew_start=0, ew_freq=10, lw_start=0, lw_freq=10, gamma_reg=1e-4, weight_CE_src=False, bn=False,
                weight_decay=0.0001, lr=0.001, epoch=200, device='cuda:0', batch_size=0, num_neigh=-1, verbose=2)
    for k, v in want.items():
        assert sig[k].default == v, k
    L = _lib.lib()
    for name, nargs in (("gda_pa_edge_stats_f64", 15), ("gda_pa_softmax_sums_f64", 15), ("gda_pa_ce_fwd_f32", 12),
                        ("gda_pa_ce_bwd_f32", 10), ("gda_pa_refresh_values_f32", 13)):
        assert name in _lib.EXPORTED_SYMBOLS and len(getattr(L, name).argtypes) == nargs, name
    assert "gda_pairalign.hip" in _build.SOURCES
    header = open(_build.os.path.join(_build.os.path.dirname(_build.HERE), "include", "gda_hip.h")).read()
    assert f"#define GDA_PA_MAX_CLASSES {ops.PA_MAX_CLASSES}" in header
    assert f"#define GDA_PA_SEGMENT {ops.PA_SEGMENT}" in header and f"#define GDA_PA_MAX_ITEMS {ops.PA_MAX_ITEMS}" in header
    assert ops.PA_MAX_CLASSES >= 5
    # the entry points validate before they touch a device
    assert L.gda_pa_ce_fwd_f32(None, None, 4, 3, None, 0, None, None, None, None, 0, None) == -1
    assert L.gda_pa_ce_fwd_f32(None, None, 4, ops.PA_MAX_CLASSES + 1, None, 0, None, None, None, None, 0, None) == -4
    assert L.gda_pa_edge_stats_f64(None, None, None, 4, ops.PA_MAX_CLASSES + 1, 1, None, 0, None, 0, None, None, None, 0,
                                   None) == -4
    assert L.gda_pa_refresh_values_f32(None, None, None, None, 4, 8, None, None, 0, 1.0, 0.0, 0, None) == -2


def test_refusals(G):
    s, t = pair(G)
    for kw in (dict(batch_size=8), dict(backbone="GIN"), dict(pooling="max")):
        with pytest.raises(NotImplementedError):
            PairAlign(16, 16, 4, device="cpu", epoch=1, verbose=0, **kw).fit(s, t)
    with pytest.raises(NotImplementedError, match="classes"):
        PairAlign(16, 16, ops.PA_MAX_CLASSES + 1, device="cuda:0", epoch=1, verbose=0).fit(s, t)
    bad = Data(x=s.x, edge_index=s.edge_index, y=s.y + 1)
    with pytest.raises(ValueError):
        PairAlign(16, 16, 4, device="cpu", epoch=1, verbose=0).fit(bad, t)


@pytest.mark.parametrize("ew_type", ["truth", "ratio"])
def test_truth_and_ratio_modes_against_a_plain_restatement(G, ew_type):
    m, s, t, _ = run_fit(G, "GS", epoch=2, ew_freq=1, ew_type=ew_type, label_rw=False, weight_CE_src=False)
    C, ei, y = 4, s.edge_index, s.y
    if ew_type == "truth":
        want = s.true_ew
    else:                                     # calc_ratio_weight from the edge list, pair by pair
        p_src = np.zeros((C, C))
        for i, j in ei.t().tolist():
            p_src[int(y[i]), int(y[j])] += 1.0 / ei.size(1)
        p_tgt = p_src * s.true_beta.reshape(C, C)
        num = (p_tgt + m.gamma_reg) / (p_tgt + m.gamma_reg).sum(axis=1, keepdims=True)
        den = (p_src + m.gamma_reg) / (p_src + m.gamma_reg).sum(axis=1, keepdims=True)
        want = num / den
        np.testing.assert_allclose(ratio_weight(p_src.reshape(-1), s.true_beta, m.gamma_reg, C)[0], want, rtol=1e-13)
    np.testing.assert_allclose(s.ew, want, rtol=1e-12)
    per_edge = np.array([want[int(y[i]), int(y[j])] for i, j in ei.t().tolist()]).astype(np.float32)
    np.testing.assert_array_equal(s.edge_weight.numpy(), per_edge)


def test_fixture_regenerates_bit_for_bit(G, tmp_path):
    from tests.golden import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not on this machine")
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.golden.make_golden_pairalign", "--out", str(tmp_path)], cwd=root,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    new = np.load(tmp_path / "pairalign_fit.npz")
    assert sorted(new.files) == sorted(G)
    for k in G:
        assert np.array_equal(new[k], G[k]), k
