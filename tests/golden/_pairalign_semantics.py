"""PairAlign fixture support: the driver that runs the reference's own ``pygda/models/pa.py`` on the PyG stub (build
container only, via ``make_golden_pairalign``), and what is injected around it.

INJECTED (``_pyg_stub.py`` and ``_ref_loader.py`` are not edited):
- an empty placeholder module named ``cvxpy``, so that ``pa.py`` imports (cvxpy and SCS are not installed);
- ``LS_optimization`` and ``calc_label_rw`` are replaced ON THE INSTANCE by :func:`fixture_qp` behind the same
  arguments and the same return value.  The bodies of these two methods are the only lines of the reference that do
  not run: they state the program ``min |cov x - m|^2 + lam |x - 1|^2, mu . x = 1, x >= 0`` for cvxpy and hand it to
  SCS.  The fixture solves the same program in float64 with scipy's SLSQP to a tight tolerance and polishes the result
  on the support SLSQP found (an equality-constrained solve, exact to rounding); the tests certify every recorded
  solution by its KKT conditions, independently of how it was found.  Nothing here imports ``pygda_amd``.

RECORDED by wrapping, not by editing: ``init_model`` (the initial state), ``forward_model`` (after every epoch ``ew``,
``lw`` and ``edge_weight``), the two solver entries (inputs and solution of every call) and the module's ``logger``."""
import contextlib
import io
import sys
import types

import numpy as np
import torch
from scipy.optimize import minimize

from . import _pyg_stub


def fixture_qp(cov, m, mu, lam):
    """``argmin |cov x - m|^2 + lam |x - 1|^2`` subject to ``mu . x = 1``, ``x >= 0``: SLSQP, then the exact
    equality-constrained solution on its support, the support corrected until every sign condition holds."""
    n = cov.shape[1]
    H = 2.0 * (cov.T @ cov + lam * np.eye(n))
    g = -2.0 * (cov.T @ m + lam * np.ones(n))
    res = minimize(lambda x: float(np.sum((cov @ x - m) ** 2) + lam * np.sum((x - 1.0) ** 2)), np.ones(n),
                   jac=lambda x: H @ x + g, method="SLSQP", bounds=[(0.0, None)] * n,
                   constraints=[dict(type="eq", fun=lambda x: float(mu @ x - 1.0), jac=lambda x: mu)],
                   options=dict(ftol=1e-15, maxiter=2000))
    sup = res.x > 1e-7
    for _ in range(4 * n + 4):
        idx = np.flatnonzero(sup)
        k = idx.size
        K = np.zeros((k + 1, k + 1))
        K[:k, :k] = H[np.ix_(idx, idx)]
        K[:k, k] = K[k, :k] = mu[idx]
        sol = np.linalg.solve(K, np.concatenate([-g[idx], [1.0]]))
        x = np.zeros(n)
        x[idx] = sol[:k]
        if (x[idx] < 0).any():
            sup[idx[np.argmin(x[idx])]] = False
            continue
        red = H @ x + g + sol[k] * mu
        off = np.flatnonzero(~sup)
        if off.size and red[off].min() < -1e-12 * max(1.0, np.abs(g).max()):
            sup[off[np.argmin(red[off])]] = True
            continue
        return x
    raise RuntimeError("fixture_qp: the support did not settle")


def load_pairalign(ref):
    from . import _ref_loader
    sys.modules.setdefault("cvxpy", types.ModuleType("cvxpy"))
    pa = _ref_loader._load("pygda.models.pa", "pygda/models/pa.py")
    ref.PairAlign, ref.pa_module = pa.PairAlign, pa
    return ref


def _np64(t):
    return t.cpu().detach().numpy().astype(np.double)


def run_fit(ref, s, t, kw, epochs, init_seed):
    """The reference's ``PairAlign.fit`` and a ``predict`` per domain."""
    pa = ref.pa_module
    s = _pyg_stub.Data(x=s.x, edge_index=s.edge_index, y=s.y, train_mask=s.train_mask, edge_weight=None)
    t = _pyg_stub.Data(x=t.x, edge_index=t.edge_index, y=t.y, edge_weight=None)
    m = ref.PairAlign(device="cpu", epoch=epochs, verbose=0, num_neigh=[-1, -1], **kw)
    rec, log, solves, per_epoch = {}, [], [], []
    init, forward_model = m.init_model, m.forward_model

    def init_rec(**k):
        net = init(**k)
        rec["init"] = {k2: v.detach().numpy().copy() for k2, v in net.state_dict().items()}
        return net

    def ls_optimization(cov, muhat_tgt, mu_src, lambda_reg):
        cov, mt, ms = _np64(cov), _np64(muhat_tgt).reshape(-1), _np64(mu_src).reshape(-1)
        x = fixture_qp(cov, mt, ms, lambda_reg)
        solves.append(("edge", len(per_epoch), cov, mt, ms, float(lambda_reg), x))
        return x

    def calc_label_rw(y_src, y_hat_tgt, cov, lambda_reg):
        ys, yt, cov = _np64(y_src), _np64(y_hat_tgt), _np64(cov)
        x = fixture_qp(cov, yt, ys, lambda_reg)
        solves.append(("label", len(per_epoch), cov, yt, ys, float(lambda_reg), x))
        return x

    def forward_rec(source_data, target_data, epoch):
        out = forward_model(source_data, target_data, epoch)
        per_epoch.append((np.array(source_data.ew, dtype=np.float64), np.array(source_data.lw, dtype=np.float64),
                          source_data.edge_weight.detach().numpy().astype(np.float32).copy()))
        return out

    m.init_model, m.forward_model = init_rec, forward_rec
    m.LS_optimization, m.calc_label_rw = ls_optimization, calc_label_rw
    old = pa.logger
    pa.logger = lambda **k: log.append((k["loss"], k["source_train_acc"]))
    try:
        torch.manual_seed(init_seed)
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(divide="ignore", invalid="ignore"):
            m.fit(s, t)
            ps, _ = m.predict(s)
            pt, _ = m.predict(t)
    finally:
        pa.logger = old
    return dict(init=rec["init"], final={k: v.detach().numpy().copy() for k, v in m.gnn.state_dict().items()},
                losses=np.array([l for l, _ in log], dtype=np.float64),
                accs=np.array([a for _, a in log], dtype=np.float64), solves=solves,
                ew=np.stack([e for e, _, _ in per_epoch]), lw=np.stack([l for _, l, _ in per_epoch]),
                edge_weight=np.stack([w for _, _, w in per_epoch]),
                true_ew=np.asarray(s.true_ew), true_lw=np.asarray(s.true_lw), true_beta=np.asarray(s.true_beta),
                src_logits=ps.detach().numpy().copy(), tgt_logits=pt.detach().numpy().copy(),
                y_hat=t.y_hat.detach().numpy().copy())
