"""GTrans without a GPU: ``utils.perturb`` against the outputs recorded from the reference's own perturb.py, host fits
against the fixtures recorded from its gtrans.py (tests/golden/make_golden_gtrans.py), the host fallbacks of
``wgcn_norm`` / ``weighted_propagate`` and the edge-gradient algebra of include/gda_hip.h against float64 autograd through
a dense ``gcn_norm``, the refusals, the alias import and the argument checks of gda_gtrans.hip's C ABI."""
import ctypes
import inspect
import os
import random

import numpy as np
import pytest
import torch

from pygda_amd import _lib, ops
from pygda_amd.data import Data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ("gtrans_fit_plain.npz", "gtrans_fit_margin.npz")
PROJECT_CASES = ("below", "above", "one", "mid", "mid_below", "big")
# both bisections end within 1e-5 of the root of a monotone function: 2e-5 per entry, and the float32 rounding of the
# clamp's operands (entries and miu are below 2: one ulp of 2 each)
PROJECT_BOUND = 2e-5 + 2 * 2.4e-7


def fixture(name):
    f = np.load(os.path.join(HERE, name))
    s = Data(x=torch.from_numpy(f["src_x"]), edge_index=torch.from_numpy(f["src_ei"]), y=torch.from_numpy(f["src_y"]))
    t = Data(x=torch.from_numpy(f["tgt_x"]), edge_index=torch.from_numpy(f["tgt_ei"]), y=torch.from_numpy(f["tgt_y"]))
    return f, s, t


def fixture_replay(f):
    lens = f["mask_len"]
    off = np.concatenate([[0], np.cumsum((lens + 7) // 8)])
    masks = [np.unpackbits(f["masks"][off[i]:off[i + 1]])[:lens[i]] for i in range(len(lens))]
    return dict(masks=masks, perms=[p.astype(np.int64) for p in f["perms"]])


def run_fit(f, s, t, device, replay=False, **kw):
    """A fit of the fixture's configuration: under its three seeds (the draws are then the reference's), or with its
    recorded masks and permutations replayed; what :func:`check_fit_against_fixture` reads."""
    from pygda_amd.models import GTrans
    if replay:
        kw["replay"] = fixture_replay(f)
    m = GTrans(16, 16, 3, num_layers=2, lr=0.05, ratio=0.1, loop_feat=2, loop_adj=1, margin=float(f["margin"]),
               device=device, epoch=12, verbose=0, record=True, **kw)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    seeds = [int(v) for v in f["seeds"]]
    torch.manual_seed(seeds[0])
    random.seed(seeds[1])
    np.random.seed(seeds[2])
    m.fit(s, t)
    cpu = lambda v: v.detach().double().cpu().numpy()
    got = dict(src_losses=np.array([l for l, a in log if a is not None]), accs=np.array([a for _, a in log if a is not None]),
               steps=np.array(m.parts_log), p_iter=np.stack([cpu(p) for p in m.p_log]),
               w_iter=np.stack([cpu(w) for _, w in m.w_log]), coalesced_ei=m.w_log[0][0].cpu().numpy(),
               new_feat=cpu(m.new_feat), edge_index=m.edge_index.cpu().numpy(), edge_weight=cpu(m.edge_weight),
               logits=cpu(m.predict(t)[0]))
    return m, got


def check_fit_against_fixture(got, f):
    """Every recorded figure of a fit -- the pretraining losses, the loss and both parts of every ``test_time_loss``
    call, the flip weights and the raw edge weights after every iteration, ``new_feat``, the final edge weights and
    ``predict``'s logits -- is held against the fixture's own float32-versus-float64 distance by the project's bound
    (tests/test_gpu_acdne._close):

        |ours - f64| <= 8 |reference fp32 - f64| + 2e-6 max|f64|            (max norm per figure)

    and each figure is printed before it is asserted.  The source accuracies, the coalesced edge list and the final
    edge list are discrete: equal."""
    assert np.array_equal(got["accs"], f["accs"]) and np.array_equal(f["accs"], f["f64/accs"])
    assert np.array_equal(got["coalesced_ei"], f["coalesced_ei"])
    assert np.array_equal(got["edge_index"], f["edge_index"]) and np.array_equal(f["edge_index"], f["f64/edge_index"])
    bad = []
    for k in ("src_losses", "steps", "p_iter", "w_iter", "new_feat", "edge_weight", "logits"):
        f64, ref32 = f["f64/" + k].astype(np.float64), f[k].astype(np.float64)
        assert got[k].shape == f64.shape, (k, got[k].shape, f64.shape)
        err, lim = np.abs(got[k] - f64).max(), 8 * np.abs(ref32 - f64).max() + 2e-6 * np.abs(f64).max()
        print(f"{k}: |ours - f64| = {err:.3e}, |reference fp32 - f64| = {np.abs(ref32 - f64).max():.3e}, bound {lim:.3e}")
        if not err <= lim:
            bad.append(k)
    assert not bad, bad


# -- utils.perturb against the reference's recorded outputs ------------------------------------------------------------------
def test_perturb_names_and_signatures():
    from pygda_amd import utils
    from pygda_amd.utils import perturb
    for name in ("linear_to_triu_idx", "inner", "inner_margin", "diff", "bisection", "project", "to_symmetric",
                 "get_modified_adj"):
        assert getattr(utils, name) is getattr(perturb, name)
    assert list(inspect.signature(perturb.project).parameters) == ["n_perturbations", "values", "eps", "inplace"]
    assert list(inspect.signature(perturb.get_modified_adj).parameters) == [
        "modified_edge_index", "perturbed_edge_weight", "n", "device", "edge_index", "edge_weight", "make_undirected"]
    assert list(inspect.signature(perturb.bisection).parameters) == ["edge_weights", "a", "b", "n_perturbations", "epsilon",
                                                                     "iter_max"]
    assert list(inspect.signature(perturb.to_symmetric).parameters) == ["edge_index", "edge_weight", "n", "op"]
    n = 9
    row, col = torch.triu_indices(n, n, 1)
    lin = (2 * n - row - 1) * row // 2 + col - row - 1
    assert torch.equal(perturb.linear_to_triu_idx(n, lin), torch.stack([row, col]))


@pytest.mark.parametrize("case", PROJECT_CASES)
def test_project_matches_the_reference(case):
    from pygda_amd.utils.perturb import project
    f = np.load(os.path.join(HERE, "gtrans_perturb.npz"))
    v, budget = torch.from_numpy(f[f"project/{case}/in"]), int(f[f"project/{case}/budget"])
    out64 = project(budget, v.double(), 1e-7)
    assert np.array_equal(out64.numpy(), f[f"project/{case}/out64"])            # float64: bit for bit
    assert torch.equal(v, torch.from_numpy(f[f"project/{case}/in"]))            # not in place
    out32 = project(budget, v.clone(), 1e-7).double().numpy()
    err = np.abs(out32 - f[f"project/{case}/out32"]).max()
    print(f"{case}: float32 project against the reference's: {err:.3e} (bound {PROJECT_BOUND:.3e})")
    assert err <= PROJECT_BOUND
    assert np.abs(out32 - f[f"project/{case}/out64"]).max() <= PROJECT_BOUND
    active = float(v.double().clamp(0, 1).sum()) > budget
    assert active == (case in ("above", "one", "mid", "big"))
    if active:
        assert abs(float(out64.sum()) - budget) <= 1e-5 * v.numel() + 1e-7 * v.numel()


@pytest.mark.parametrize("und", (False, True))
def test_get_modified_adj_matches_the_reference(und):
    from pygda_amd.utils.perturb import get_modified_adj
    f = np.load(os.path.join(HERE, "gtrans_perturb.npz"))
    tag = "adj/und" if und else "adj/dir"
    n, ei, mei = int(f["adj/n"]), torch.from_numpy(f["adj/ei"]), torch.from_numpy(f["adj/mei"])
    p = torch.from_numpy(f["adj/p"]).requires_grad_(True)
    w = torch.from_numpy(f["adj/w"])
    e1, w1 = get_modified_adj(mei, p, n, "cpu", ei, w, und)
    e2, w2 = get_modified_adj(mei, p, n, "cpu", e1, w1, und)
    for got, key in ((e1, "e1"), (w1, "w1"), (e2, "e2"), (w2, "w2")):
        assert np.array_equal(got.detach().numpy(), f[f"{tag}/{key}"]), key          # float64: bit for bit
    pre = f[f"{tag}/w1"]
    assert (pre < 1).any() and (pre == 1).any()                                      # both fold branches and the edge
    (g,) = torch.autograd.grad(w2.sum(), p)                                          # differentiable in the flip weights
    assert torch.isfinite(g).all() and g.abs().sum() > 0
    e32, w32 = get_modified_adj(mei, p.detach().float(), n, "cpu", ei, w.float(), und)
    assert np.array_equal(e32.numpy(), f[f"{tag}/e1"]) and np.abs(w32.double().numpy() - f[f"{tag}/w1"]).max() <= 4e-7


# -- the host fallbacks and the edge-gradient algebra ----------------------------------------------------------------------
def crafted_graph(n, seed, hub=False):
    """Edges with a duplicate, an explicit self loop, a one-directional edge, an isolated node (n - 1) and, with ``hub``,
    a node with 270 in-edges and one with 270 out-edges: rows beyond the 128-entry segments of either CSR and beyond
    the 256 entries from which ``graph.RowSplit`` chunks a row of the SpMM."""
    g = torch.Generator().manual_seed(seed)
    if n == 1:
        return torch.zeros(2, 0, dtype=torch.int64), torch.zeros(2, 0, dtype=torch.int64)
    live = n - 1
    k = torch.unique(torch.randint(0, live * live, (3 * n,), generator=g))
    ei = torch.stack([k // live, k % live])
    ei = ei[:, ei[0] < ei[1]]
    both = torch.cat([ei, ei.flip(0)[:, 1:]], dim=1)                                 # the first edge stays one-way
    extra = [both, both[:, :1], torch.tensor([[2], [2]])]                            # a duplicate, a self loop
    if hub and live > 280:
        a = torch.arange(10, 280)
        extra += [torch.stack([a, torch.full_like(a, 3)]), torch.stack([torch.full_like(a, 5), a])]
    ei = torch.cat(extra, dim=1)
    m_ei = ei[:, ei[0] < ei[1]]
    return ei, m_ei


def dense_reference(ei_c, w_prev_edges, mei, p, keep, n, h_list, mean=True):
    """float64 autograd through a DENSE gcn_norm: the flip, the fold, the keep mask, add_remaining_self_loops, the degree
    over the destination, ``D^-1/2 A D^-1/2`` and one aggregation per width."""
    P = torch.zeros(n, n, dtype=torch.float64)
    C = torch.zeros(n, n, dtype=torch.float64)
    for a, b in ((mei[0], mei[1]), (mei[1], mei[0])):
        P = P.index_put((a, b), p, accumulate=True)
        C = C.index_put((a, b), torch.ones_like(p), accumulate=True)
    P = P / C.clamp(min=1) if mean else P
    W = torch.zeros(n, n, dtype=torch.float64).index_put((ei_c[0], ei_c[1]), w_prev_edges)
    listed = torch.zeros(n, n, dtype=torch.bool).index_put((ei_c[0], ei_c[1]), torch.ones(ei_c.size(1), dtype=torch.bool))
    x = W + P
    w = torch.where(x > 1, 2 - x, x)
    K = torch.zeros(n, n, dtype=torch.float64).index_put((ei_c[0], ei_c[1]), keep.double())
    A = w * K * listed
    eye = torch.eye(n, dtype=torch.bool)
    has_loop = (listed & (K > 0) & eye).any(0)
    A = torch.where(eye & ~has_loop[None, :], torch.ones_like(A), A)                 # A[src, dst]
    deg = A.sum(0)
    s = torch.where(deg > 0, deg.clamp(min=1e-300).pow(-0.5), torch.zeros_like(deg))
    N = s[:, None] * A * s[None, :]
    return [N.t() @ h for h in h_list], w


def plan_inputs(n, seed, hub=False, dtype=torch.float64):
    ei, mei = crafted_graph(n, seed, hub)
    plan = ops.wgcn_plan(ei, n, mei)
    g = torch.Generator().manual_seed(seed + 1)
    # pre-fold values on both sides of 1 and exactly 1; zero-weight edges; a row whose edges are all dropped
    w_edges = torch.rand(plan.ec, generator=g, dtype=torch.float64).mul(0.9).add(0.1).float().double()
    p = torch.rand(plan.m, generator=g, dtype=torch.float64).mul(0.9).float().double()
    keep = torch.rand(plan.ec, generator=g) >= 0.2
    if plan.ec:
        w_edges[::5] = 0.0
        w_edges[1::7] = 1.0
        dst7 = plan.edge_index[1] == 7                                               # (not the hub: its row stays live)
        keep[dst7 & (plan.edge_index[0] != 7)] = False
        first = int(plan.kidx[plan.entry_of_edge[0]]) if plan.m else -1
        if first >= 0:                                                               # w_prev + P == 1 exactly
            w_edges[0] = 0.75
            p[plan.pgrp == first] = 0.25
    return plan, ei, mei, w_edges.to(dtype), p.to(dtype), keep


@pytest.mark.parametrize("n,hub", ((1, False), (67, False), (300, True)))
def test_host_norm_and_aggregation_match_dense_float64_autograd(n, hub):
    plan, ei, mei, w_edges, p, keep = plan_inputs(n, 40 + n, hub)
    g = torch.Generator().manual_seed(5)
    h = torch.randn(n, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    G = torch.randn(n, 6, generator=g, dtype=torch.float64)
    p1, p2 = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
    val, w = ops.wgcn_norm(plan, plan.entry_weights(w_edges), p1 if plan.m else None, keep=keep)
    y = ops.weighted_propagate(h, plan, val)
    (yd,), wd = dense_reference(plan.edge_index, w_edges, mei, p2, keep, n, [h])
    assert torch.allclose(y, yd, rtol=1e-12, atol=1e-13)
    assert torch.allclose(w[plan.entry_of_edge], wd[plan.edge_index[0], plan.edge_index[1]], rtol=0, atol=1e-15)
    if plan.m:
        (g1,) = torch.autograd.grad((y * G).sum(), p1)
        (g2,) = torch.autograd.grad((yd * G).sum(), p2)
        assert torch.allclose(g1, g2, rtol=1e-10, atol=1e-12)
        # the chain of include/gda_hip.h, written out: gv, dL/ds, dL/ddeg, dL/dkw, the gather to the parameters
        erow, col = plan.erow, plan.col
        x = plan.entry_weights(w_edges) + torch.where(plan.kidx >= 0, (torch.zeros(plan.mu, dtype=torch.float64)
                                                      .index_add(0, plan.pgrp, p) / (plan.gptr[1:] - plan.gptr[:-1])
                                                      )[plan.kidx.clamp(min=0)], torch.zeros((), dtype=torch.float64))
        sign = torch.where(x > 1, -1.0, 1.0)
        kp = torch.ones(plan.nnz, dtype=torch.float64)
        kp[plan.epos >= 0] = keep.double()[plan.epos[plan.epos >= 0]]
        wv = torch.where(x > 1, 2 - x, x)
        kw = torch.where((kp == 0) & (erow == col), torch.ones_like(wv), kp * wv)
        deg = torch.zeros(n, dtype=torch.float64).index_add(0, erow, kw)
        s = torch.where(deg > 0, deg.clamp(min=1e-300).pow(-0.5), torch.zeros_like(deg))
        gv = (G[erow] * h.detach()[col]).sum(1)
        ds = torch.zeros(n, dtype=torch.float64).index_add(0, erow, gv * kw * s[col]) \
            + torch.zeros(n, dtype=torch.float64).index_add(0, col, gv * kw * s[erow])
        ddeg = -0.5 * s ** 3 * ds
        dkw = s[col] * s[erow] * gv + ddeg[erow]
        de = sign * kp * dkw
        pe = plan.pent[plan.pgrp]
        dp = sum(torch.where(pe[:, j] >= 0, de[pe[:, j].clamp(min=0)], torch.zeros((), dtype=torch.float64)) for j in (0, 1))
        dp = dp / (plan.gptr[1:] - plan.gptr[:-1])[plan.pgrp]
        assert torch.allclose(dp, g2, rtol=1e-10, atol=1e-12)


def test_plan_reproduces_get_modified_adj_call_after_call():
    from pygda_amd.utils.perturb import get_modified_adj
    n = 67
    ei, mei = crafted_graph(n, 3)
    plan = ops.wgcn_plan(ei, n, mei)
    p = torch.rand(mei.size(1), dtype=torch.float64)
    e, w = ei, torch.ones(ei.size(1), dtype=torch.float64)
    wp = plan.entry_weights(plan.w0)
    for _ in range(3):
        e, w = get_modified_adj(mei, p, n, "cpu", e, w, True)
        _, wp = ops.wgcn_norm(plan, wp, p)
        assert torch.equal(e, plan.edge_index) and torch.equal(wp[plan.entry_of_edge], w)
    assert int((plan.gptr[1:] - plan.gptr[:-1]).max()) == 2                          # the duplicate edge: a group of two
    for seg_off, row_seg, ptr in ((plan.seg_off, plan.row_seg, plan.rowptr), (plan.t_seg_off, plan.t_row_seg, plan.t_rowptr)):
        assert int(seg_off[-1]) == plan.nnz and (seg_off[1:] - seg_off[:-1]).max() <= ops.WGCN_SEGMENT
        assert torch.equal(seg_off[row_seg[:-1]], ptr[:-1])


def test_host_loss_handles_a_zero_row_and_both_margins():
    g = torch.Generator().manual_seed(1)
    o = [torch.randn(9, 5, generator=g, dtype=torch.float64) for _ in range(3)]
    for t in o:
        t[4] = 0
    for margin in (-1, 0.3):
        leaves = [t.clone().requires_grad_(True) for t in o]
        loss, parts = ops.gtrans_loss(*leaves, margin)
        grads = torch.autograd.grad(loss, leaves)
        assert torch.isfinite(loss) and all(torch.isfinite(x).all() for x in grads)
        assert torch.allclose(parts[0], parts[1] - parts[2]) and torch.equal(parts[0], loss.detach())


# -- the trainer ------------------------------------------------------------------------------------------------------------
def test_signature_alias_and_refusals():
    from pygda.models import GTrans
    from pygda_amd.models import GTrans as G2
    assert GTrans is G2
    sig = inspect.signature(GTrans.__init__).parameters
    want = dict(num_layers=3, dropout=0., loop_adj=1, loop_feat=4, ratio=0.1, margin=-1, make_undirected=True,
                strategy='dropedge', weight_decay=0., lr=1e-4, epoch=500, gnn='gcn', device='cuda:0', batch_size=0,
                num_neigh=-1, verbose=2)
    for k, v in want.items():
        assert sig[k].default == v, k
    assert list(sig)[1:4] == ["in_dim", "hid_dim", "num_classes"]
    for kw, word in ((dict(gnn='gat'), "gnn"), (dict(batch_size=32), "batch_size"), (dict(strategy='shuffle'), "strategy"),
                     (dict(loop_adj=2), "loop_adj")):
        with pytest.raises(NotImplementedError, match=word):
            GTrans(4, 4, 2, device="cpu", **kw)
    assert sum(ops.gtrans_bytes(1000, 500, 9000, 4000, 64)) >= 4 * 4 * 1000 * 500


@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_fit_matches_the_reference(name):
    f, s, t = fixture(name)
    m, got = run_fit(f, s, t, "cpu")
    assert len(got["src_losses"]) == 12 and got["steps"].shape == (12 + 20, 3)
    check_fit_against_fixture(got, f)
    assert np.array_equal(got["p_iter"], np.full_like(got["p_iter"], np.float32(1e-7)))   # the reference's flip weights
    assert int(f["above_floor"].max()) == 0 and float(f["top_gap"].max()) == 0.0


def test_cpu_fit_with_replayed_draws_and_with_stepped_structure():
    f, s, t = fixture(FIXTURES[0])
    m, got = run_fit(f, s, t, "cpu", replay=True)
    check_fit_against_fixture(got, f)
    m2, got2 = run_fit(f, s, t, "cpu", replay=True, step_structure=True)
    k = int(f["n_perturbations"])
    p = got2["p_iter"]
    assert np.array_equal(got2["steps"][:3], got["steps"][:3])                            # the same up to the first step
    assert (p[0] > 1e-6).sum() > 0 and p.min() >= np.float32(1e-7) and p.max() <= 1 - 1e-7
    assert np.clip(p, 0, 1).sum(1).max() <= k + 1e-5 * p.shape[1]
    assert np.isfinite(got2["logits"]).all()


# -- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_gtrans_entries_validate_before_touching_a_device():
    L = _lib.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)                      # never dereferenced
    big = 1 << 30
    names = ("gda_wgcn_workspace_bytes", "gda_wgcn_norm_f32", "gda_wgcn_edge_grad_f32", "gda_wgcn_norm_bwd_f32",
             "gda_gtrans_loss_workspace_bytes", "gda_gtrans_loss_f32", "gda_gtrans_project_workspace_bytes",
             "gda_gtrans_project_f32")
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)

    def plan(n=10, nnz=30, m=8, mu=8, nseg=10, t_nseg=10, hole=None, ec=20):
        ptrs = {k: 64 for k in ("rowptr", "colidx", "t_rowptr", "t_colidx", "t_to_fwd", "erow", "epos", "kidx", "pent",
                                "gptr", "gidx", "pgrp", "seg_off", "row_seg", "t_seg_off", "t_row_seg")}
        if hole:
            ptrs[hole] = None
        return _lib.WgcnPlanStruct(n, nnz, m, mu, nseg, t_nseg, 1, ec, *ptrs.values())

    def norm(pl=None, w_prev=p, w=p, p_drop=0.0, ws=p, wsb=big, val=p):
        pl = plan() if pl is None else pl
        return L.gda_wgcn_norm_f32(ctypes.byref(pl), w_prev, p, None, p_drop, 0, None, 0, w, ctypes.c_void_p(128),
                                   ctypes.c_void_p(192), p, p, val, p, ws, wsb, None)

    assert L.gda_wgcn_norm_f32(None, p, p, None, 0.0, 0, None, 0, p, p, p, p, p, p, p, p, big, None) == -1
    assert norm(plan(n=0)) == -2 and norm(plan(nnz=5)) == -2 and norm(plan(mu=9)) == -2 and norm(plan(nseg=9)) == -2
    assert norm(plan(ec=31)) == -2                                         # more listed edges than stored entries
    assert norm(plan(nseg=12)) == -2                                       # more segments than the contract allows
    assert norm(plan(hole="kidx")) == -1 and norm(plan(hole="t_seg_off")) == -1
    assert norm(w_prev=None) == -1 and norm(val=None) == -1 and norm(p_drop=1.0) == -2
    assert norm(w=p) == -5                                                 # w aliases w_prev
    assert norm(w=ctypes.c_void_p(256), val=odd) == -4 and norm(w=ctypes.c_void_p(256), ws=ctypes.c_void_p(72)) == -4
    assert norm(w=ctypes.c_void_p(256), wsb=16) == -3

    def grad(pl=None, d=16, G=p):
        pl = plan() if pl is None else pl
        return L.gda_wgcn_edge_grad_f32(ctypes.byref(pl), G, p, d, p, None)

    assert grad(d=0) == -2 and grad(d=257) == -4 and grad(G=None) == -1 and grad(G=odd) == -4 and grad(plan(n=0)) == -2

    def bwd(pl=None, gv=p, wsb=big):
        pl = plan() if pl is None else pl
        return L.gda_wgcn_norm_bwd_f32(ctypes.byref(pl), gv, p, p, p, p, p, wsb, None)

    assert bwd(gv=None) == -1 and bwd(gv=odd) == -4 and bwd(wsb=16) == -3 and bwd(plan(m=-1)) == -2

    def loss(n=10, d=4, o1=p, wsb=big, ws=p):
        return L.gda_gtrans_loss_f32(o1, p, p, n, d, -1.0, p, p, p, p, ws, wsb, None)

    assert loss(n=0) == -2 and loss(d=0) == -2 and loss(o1=None) == -1 and loss(o1=odd) == -4 and loss(wsb=4) == -3
    assert loss(ws=None) == -1

    def proj(m=100, q=p, budget=5.0, lo=1e-7, wsb=big):
        return L.gda_gtrans_project_f32(q, m, budget, lo, p, wsb, None)

    assert proj(m=0) == -2 and proj(budget=-1.0) == -2 and proj(lo=0.7) == -2 and proj(q=None) == -1 and proj(q=odd) == -4
    assert proj(m=100000, wsb=64) == -3
    assert L.gda_gtrans_project_workspace_bytes(100000) >= 23 * 24 + 2 * 3 * 8
    header = open(os.path.join(ROOT, "include", "gda_hip.h")).read()
    assert "#define GDA_WGCN_SEGMENT 128" in header and "#define GDA_WGCN_MAX_WIDTH 256" in header
    from pygda_amd.graph import SPLIT_THRESHOLD
    assert ops.WGCN_SEGMENT == SPLIT_THRESHOLD == 128 and ops.WGCN_MAX_WIDTH == 256
    with pytest.raises(_lib.GdaError, match="gda_gtrans_project_f32"):
        _lib.call("gda_gtrans_project_f32", None, 10, 1.0, 1e-7, p, big, None)


def test_fixture_regenerates_bit_for_bit(tmp_path):
    from tests.golden import _ref_loader
    if not _ref_loader.available():
        pytest.skip("needs the reference checkout (build container only)")
    import subprocess
    import sys
    subprocess.run([sys.executable, "-m", "tests.golden.make_golden_gtrans", "--out", str(tmp_path)], cwd=ROOT, check=True,
                   env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), stdout=subprocess.DEVNULL)
    for name in FIXTURES + ("gtrans_perturb.npz",):
        a, b = np.load(os.path.join(HERE, name)), np.load(os.path.join(str(tmp_path), name))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), (name, k)
