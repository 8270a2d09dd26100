"""GraphCTA without a GPU: the host fallbacks of ``ops.cta_model_loss`` / ``cta_knn`` / ``cta_test_time_loss`` against a
float64 brute-force ``[N, N]`` restatement of the reference's formulas written here (the yardsticks of
tests/test_gpu_graphcta.py, with the inputs both files share and the check that their discrete decisions are decided),
the constructor's signature and refusals, the alias import, the argument checks of gda_graphcta.hip's C ABI, and host
fits against the fixtures recorded from the reference's own graphcta.py (tests/golden/make_golden_graphcta.py)."""
import ctypes
import inspect
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pygda_amd import _lib, ops
from pygda_amd.data import Data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ("graphcta_fit_a.npz", "graphcta_fit_b.npz", "graphcta_fit_c.npz")   # b: make_undirected=False, stopped
MODEL_SHAPES = [(n, d, c) for n in (1, 67, 300) for d in (4, 20, 128, 256) for c in (2, 5, 64)]
KNN_SHAPES = [(n if n else k1, d, k1) for k1 in (2, 6, 16) for n in (0, 67, 513) for d in (4, 128)]   # 0: N = K1
KNN_SEED = {(513, 4, 6): 1, (16, 128, 16): 2, (513, 4, 16): 2, (513, 128, 16): 3}      # see knn_inputs
GAP = 1e-5          # what "decided" asks of an entropy or probability gap: a hundred float32 roundings of an O(1) figure


# ---- the float64 yardsticks: the reference's formulas over the full [N, N] arrays ------------------------------------------
def brute_model_loss(feat, logits, proto, pred, tau, lamb):
    """``instance_proto_alignment`` and the weighted cross-entropy with the diagonal masked out of the ``[N, N]`` array
    (the reference sums it and subtracts it)."""
    n = feat.size(0)
    rows = torch.arange(n)
    fn = feat / feat.norm(dim=1, keepdim=True).clamp_min(1e-12)
    cn = proto / proto.norm(dim=1, keepdim=True).clamp_min(1e-12)
    sim = fn @ cn.t()
    weight = sim[rows, pred]
    sim = torch.exp(sim / tau)
    pos = sim[rows, pred]
    pairs = torch.exp(fn @ fn.t() / tau) * (1 - torch.eye(n, dtype=feat.dtype))
    logit = pos / (sim.sum(dim=1) - pos + pairs.sum(dim=1) + 1e-8)
    cl = -torch.log(logit + 1e-8).mean()
    ce = F.cross_entropy(logits, pred, reduction='none')
    local = torch.sum(weight * ce) / torch.sum(weight).item()
    return local * (1 - lamb) + cl * lamb, local, cl


def brute_knn(feat, mem, k1):
    """Ranks by (value descending, index ascending) over the full ``feat mem^T``."""
    dist = (feat @ mem.t()).numpy()
    idx = np.stack([np.lexsort((np.arange(dist.shape[1]), -row))[:k1] for row in dist])
    return torch.from_numpy(idx), torch.from_numpy(np.take_along_axis(dist, idx, axis=1))


def brute_test_time(logits, feat, mem_fea, mem_cls, idx_near):
    """``test_time_loss``'s lines after the two forward passes, with the neighbour indices handed in."""
    n, c = logits.shape
    k = idx_near.size(1) - 1
    softmax_out = F.softmax(logits, dim=1)
    _, predict = torch.max(softmax_out, 1)
    mean_ent = torch.sum(-softmax_out * torch.log(softmax_out + 1e-8), dim=1)
    est_p = (mean_ent < mean_ent.mean()).sum().item() / mean_ent.size(0)
    value = mean_ent.detach().numpy()
    predict = predict.numpy()
    train_idx = np.zeros(predict.shape)
    for cls in range(c):
        c_idx = np.where(predict == cls)[0]
        order = np.lexsort((c_idx, value[c_idx]))                     # (entropy, index)
        for ei in range(int(len(c_idx) * est_p / 5)):
            train_idx[c_idx[order[ei]]] = 1
    train_idx = np.array(train_idx, dtype=bool)
    ce = F.cross_entropy(logits[train_idx], torch.from_numpy(predict[train_idx]))
    distance = feat @ mem_fea.t()
    mem_near = mem_fea[idx_near[:, 1:].long()]
    nb = torch.mean((feat.unsqueeze(1).expand(-1, k, -1) * mem_near).sum(-1).sum(1) / k)
    _, pred_mem = torch.max(mem_cls, dim=1)
    same = torch.from_numpy(predict).unsqueeze(-1) == pred_mem
    ng = ((distance * ~same).sum(1) / torch.sum(~same, dim=1)).mean()
    return ce - nb * 0.1 + ng * 0.1, ce, nb, ng, torch.from_numpy(predict), torch.from_numpy(train_idx)


# ---- the inputs both test files use ------------------------------------------------------------------------------------------
def model_inputs(n, d, c, seed=0):
    """Features around their predicted prototype (so that W = sum w_i is well away from 0), a zero feature row (row 1,
    n >= 3) and the last class without a member: a zero prototype that some rows are still assigned to."""
    g = torch.Generator().manual_seed(1000 * n + 10 * d + c + seed)
    proto = torch.randn(c, d, generator=g, dtype=torch.float64)
    proto[c - 1] = 0
    pred = torch.randint(0, c, (n,), generator=g)
    pred[0] = 0
    feat = proto[pred] + 0.5 * torch.randn(n, d, generator=g, dtype=torch.float64)
    if n >= 3:
        feat[1] = 0
    logits = 2 * torch.randn(n, c, generator=g, dtype=torch.float64)
    return feat, logits, proto, pred


def knn_inputs(n, d, k1):
    """Rows in clusters of ``k1`` (the last one takes the remainder) around centres of norm 4, the memory a noisy copy:
    a row's ``k1`` best are its cluster and rank 1 is its own copy, both by a clear margin.  Gaussian rows would not do:
    the decided margin grows with ``|f| |m|`` ~ d, the spacing of their inner products with sqrt(d).  The seed of every
    shape is the first of 0, 1, .. that leaves at most 1 % of the rows undecided (:func:`knn_decided`)."""
    g = torch.Generator().manual_seed(977 * n + 13 * d + k1 + 100003 * KNN_SEED.get((n, d, k1), 0))
    clusters = max(n // k1, 1)
    centre = torch.randn(clusters, d, generator=g, dtype=torch.float64)
    centre = 4 * centre / centre.norm(dim=1, keepdim=True)
    feat = centre[(torch.arange(n) // k1).clamp(max=clusters - 1)] + 0.5 / d ** 0.5 * torch.randn(n, d, generator=g, dtype=torch.float64)
    mem = feat + 0.3 / d ** 0.5 * torch.randn(n, d, generator=g, dtype=torch.float64)
    return feat, mem


def knn_decided(feat, mem, k1):
    """Rows whose float64 gaps at the rank boundaries 1|2 and K1|K1+1 exceed ``1e-4 |f_i| max_j |m_j|``."""
    dist = torch.sort(feat @ mem.t(), dim=1, descending=True).values
    tol = 1e-4 * feat.norm(dim=1) * mem.norm(dim=1).max()
    ok = (dist[:, 0] - dist[:, 1]) > tol
    if dist.size(1) > k1:
        ok &= (dist[:, k1 - 1] - dist[:, k1]) > tol
    return ok


def tt_inputs(n, d, c, k1, seed=0, rare_class=False):
    """Logits, bottleneck output, the two memory banks and float64's neighbour indices.  ``rare_class``: class 0 is the
    arg-max of rows 0..2 only, so that ``int(c_num * est_p / 5) = 0`` for it."""
    g = torch.Generator().manual_seed(31 * n + 7 * d + 3 * c + k1 + seed)
    logits = 2 * torch.randn(n, c, generator=g, dtype=torch.float64)
    if rare_class:
        logits[:, 0] = -10
        logits[:3, 0] = 10
    feat = torch.randn(n, d, generator=g, dtype=torch.float64)
    mem_fea = feat + 0.3 * torch.randn(n, d, generator=g, dtype=torch.float64)
    mem_cls = F.softmax(2 * torch.randn(n, c, generator=g, dtype=torch.float64), dim=1)
    idx_near, _ = brute_knn(feat, mem_fea, k1)
    return logits, feat, mem_fea, mem_cls, idx_near


def tt_decided(logits, mem_cls):
    """Whether float32 can be trusted with every discrete decision of the selection: both arg-maxes, ``ent < mean`` and
    the rank boundary of every class clear ``GAP`` in float64."""
    p = F.softmax(logits, dim=1)
    top = lambda m: (lambda s: s[:, 0] - s[:, 1])(torch.sort(m, dim=1, descending=True).values)
    ent = -(p * torch.log(p + 1e-8)).sum(dim=1)
    ok = bool((top(p) > GAP).all()) and bool((top(mem_cls) > GAP).all()) and bool(((ent - ent.mean()).abs() > GAP).all())
    est_p = (ent < ent.mean()).sum().item() / ent.numel()
    pred = p.argmax(dim=1)
    for cls in range(logits.size(1)):
        e = torch.sort(ent[pred == cls]).values
        q = int(e.numel() * est_p / 5)
        ok = ok and (q == 0 or q >= e.numel() or float(e[q] - e[q - 1]) > GAP)
    return ok


def grads(loss, *xs):
    return torch.autograd.grad(loss, xs)


# ---- the host fallbacks against the brute force ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,c", [(1, 4, 2), (67, 20, 5), (300, 128, 64)])
@pytest.mark.parametrize("tau,lamb", [(0.2, 0.2), (0.5, 0.5)])
def test_model_loss_fallback_is_the_brute_force(n, d, c, tau, lamb):
    feat, logits, proto, pred = model_inputs(n, d, c)
    a, b = feat.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    want = brute_model_loss(a, b, proto, pred, tau, lamb)
    gw = grads(want[0], a, b)
    x, y = feat.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    loss, parts = ops.cta_model_loss(x, y, proto, pred, tau, lamb)
    gg = grads(loss, x, y)
    assert torch.isfinite(parts).all() and not parts.requires_grad
    keep = torch.ones(n, dtype=torch.bool)
    if n >= 3:                                                          # the zero row: 1e12 times a gradient of O(1)
        keep[1] = False
        assert torch.allclose(gg[0][1], gw[0][1], rtol=1e-9, atol=0) and float(gw[0][1].abs().max()) > 1e6
    assert torch.allclose(parts, torch.stack(want).detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(gg[0][keep], gw[0][keep], rtol=1e-9, atol=1e-12)
    assert torch.allclose(gg[1], gw[1], rtol=1e-9, atol=1e-12)
    f32 = ops.cta_model_loss(feat.float(), logits.float(), proto.float(), pred, tau, lamb)[1]
    assert f32.dtype == torch.float32 and torch.allclose(f32.double(), parts, rtol=1e-3, atol=1e-4)


def test_knn_fallback_ranks_by_value_then_index_and_refuses_too_few_rows():
    for n, d, k1 in KNN_SHAPES:
        feat, mem = knn_inputs(n, d, k1)
        idx, val = ops.cta_knn(feat, mem, k1)
        bi, bv = brute_knn(feat, mem, k1)
        assert idx.dtype == torch.int64 and torch.equal(idx, bi) and torch.equal(val, bv)
        undecided = int((~knn_decided(feat, mem, k1)).sum())
        print(f"N = {n}, d = {d}, K1 = {k1}: {undecided} undecided rows")
        assert undecided <= n // 100
    feat = torch.tensor([[1.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    mem = torch.tensor([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0]], dtype=torch.float64)     # ties: rows 0, 1, 3
    idx, val = ops.cta_knn(feat, mem, 3)
    assert idx.tolist() == [[0, 1, 3], [2, 0, 1]] and val.tolist() == [[1, 1, 1], [1, 0, 0]]
    with pytest.raises(_lib.GdaError, match="out of range"):
        ops.cta_knn(feat, mem, 5)


@pytest.mark.parametrize("n,d,c,k1,rare", [(2, 4, 2, 2, False), (67, 20, 5, 6, False), (67, 4, 5, 6, True),
                                           (300, 128, 64, 16, False)])
def test_test_time_loss_fallback_is_the_brute_force(n, d, c, k1, rare):
    logits, feat, mem_fea, mem_cls, idx_near = tt_inputs(n, d, c, k1, rare_class=rare)
    assert tt_decided(logits, mem_cls)
    a, b = logits.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    want = brute_test_time(a, b, mem_fea, mem_cls, idx_near)
    x, y = logits.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    loss, parts, pred, sel = ops.cta_test_time_loss(x, y, mem_fea, mem_cls, idx_near)
    assert torch.equal(pred, want[4]) and torch.equal(sel, want[5])
    if rare:
        assert int((pred == 0).sum()) == 3 and not bool(sel[pred == 0].any()) and bool(sel.any())
    assert torch.allclose(parts, torch.stack(want[:4]).detach(), rtol=1e-11, atol=1e-12, equal_nan=True)
    if n == 2:                                                          # nobody is selected: the mean over no rows
        assert torch.isnan(parts[1]) and torch.isnan(parts[0]) and not bool(sel.any())
        return
    gw, gg = grads(want[0], a, b), grads(loss, x, y)
    assert torch.allclose(gg[0], gw[0], rtol=1e-9, atol=1e-13) and torch.allclose(gg[1], gw[1], rtol=1e-9, atol=1e-13)


def test_one_class_memory_gives_nan_as_the_reference_does():
    logits, feat, mem_fea, mem_cls, idx_near = tt_inputs(67, 4, 5, 6)
    mem_cls = torch.zeros_like(mem_cls)
    mem_cls[:, 2] = 1
    want = brute_test_time(logits, feat, mem_fea, mem_cls, idx_near)
    _, parts, pred, _ = ops.cta_test_time_loss(logits, feat, mem_fea, mem_cls, idx_near)
    assert bool((pred == 2).any()) and torch.isnan(want[3]) and torch.isnan(parts[3]) and torch.isfinite(parts[1:3]).all()


# ---- the C ABI's argument checks (no launch) ---------------------------------------------------------------------------------
def test_c_abi_refuses_bad_sizes_and_pointers():
    L = _lib.lib()
    buf = (ctypes.c_float * 4200)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    at = lambda k: ctypes.c_void_p(p.value + k)
    odd = at(2)
    assert L.gda_cta_loss_workspace_bytes(300, 128, 5) >= 4 * (300 * 128 * 2)
    assert L.gda_cta_knn_workspace_bytes(5484, 5484, 6) == -(-2 * 3 * 5484 * 6 * 4 // 256) * 256
    loss = lambda n, d, c, tau=0.2, ws=p, nbytes=1 << 30, feat=p: L.gda_cta_model_loss_f32(
        feat, p, p, p, n, d, c, tau, 0.2, p, at(1024), at(2048), ws, nbytes, None)
    assert loss(0, 4, 2) == -2 and loss(4, 4, 2, tau=0.0) == -2                       # GDA_E_SIZE
    assert loss(4, 257, 2) == -4 and loss(4, 4, 65) == -4                             # GDA_E_UNSUPPORTED
    assert loss(4, 4, 2, ws=None) == -1 and loss(4, 4, 2, nbytes=16) == -3            # GDA_E_NULL, GDA_E_WORKSPACE
    assert loss(4, 4, 2, feat=odd) == -4
    knn = lambda n, nm, d, k1, ws=p, nbytes=1 << 30: L.gda_cta_knn_f32(p, p, n, nm, d, k1, p, p, ws, nbytes, None)
    assert knn(4, 3, 4, 4) == -2 and knn(4, 40, 4, 17) == -4 and knn(4, 40, 300, 4) == -4
    assert knn(4, 40, 4, 4, ws=None) == -1 and knn(4, 40, 4, 4, nbytes=16) == -3
    tt = lambda n, nm, d, c, k1, nbytes=1 << 30: L.gda_cta_test_time_f32(
        p, at(512), p, p, p, p, n, nm, d, c, k1, p, at(1024), at(2048), p, p, p, nbytes, None)
    assert tt(4, 4, 4, 2, 1) == -2 and tt(4, 3, 4, 2, 4) == -2 and tt(4, 40, 4, 2, 17) == -4 and tt(4, 40, 4, 2, 4, 16) == -3


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def fixture(name):
    f = np.load(os.path.join(HERE, name))
    s = Data(x=torch.from_numpy(f["src_x"]), edge_index=torch.from_numpy(f["src_ei"]), y=torch.from_numpy(f["src_y"]))
    t = Data(x=torch.from_numpy(f["tgt_x"]), edge_index=torch.from_numpy(f["tgt_ei"]), y=torch.from_numpy(f["tgt_y"]))
    return f, s, t


def run_fit(f, s, t, device, **kw):
    """A fit of the fixture's configuration under its three seeds (the draws are then the reference's); what
    :func:`check_fit_against_fixture` reads."""
    from pygda_amd.models import GraphCTA
    m = GraphCTA(16, 16, 3, num_layers=2, lr=0.05, dropout=0., loop_model=2, loop_feat=2, loop_adj=1, K=int(f["K"]),
                 tau=float(f["tau"]), lamb=float(f["lamb"]), make_undirected=bool(f["make_undirected"]), device=device,
                 epoch=12, verbose=0, record=True, **kw)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    seeds = [int(v) for v in f["seeds"]]
    torch.manual_seed(seeds[0])
    random.seed(seeds[1])
    np.random.seed(seeds[2])
    stopped = ""
    try:
        m.fit(s, t)
    except AssertionError as e:                     # sample_final_edges' range check, restated from the reference
        stopped = str(e)
    cpu = lambda v: v.detach().double().cpu().numpy()
    choice = np.stack([c.cpu().numpy() for c in m.choice_log])
    got = dict(src_losses=np.array([l for l, a in log if a is not None]), accs=np.array([a for _, a in log if a is not None]),
               model=np.array(m.model_log)[:, [0, 2]], model_pred=np.stack([p.cpu().numpy() for p in m.pred_log]),
               steps=np.array(m.parts_log)[:, 0], tt_pred=choice[:, 0], tt_sel=choice[:, 1].astype(bool),
               tt_near=np.sort(choice[:, 2:].transpose(0, 2, 1), axis=2), mem0=m._mem0.numpy(),
               p_iter=np.stack([cpu(p) for p in m.p_log]), w_iter=np.stack([cpu(w) for _, w in m.w_log]),
               coalesced_ei=m.w_log[0][0].cpu().numpy(), new_feat=cpu(m.new_feat), stopped=np.str_(stopped),
               edge_index=np.zeros((2, 0), dtype=np.int64) if stopped else m.edge_index.cpu().numpy(),
               edge_weight=np.zeros(0) if stopped else cpu(m.edge_weight),
               logits=np.zeros((0, 3)) if stopped else cpu(m.predict(t)[0]))
    return m, got


def check_fit_against_fixture(got, f):
    """Every recorded figure of a fit -- the pretraining losses, the loss and the contrast part of every model step, the
    loss of every ``test_time_loss`` call, the flip weights and the raw edge weights after every iteration, ``new_feat``,
    the final edge weights and ``predict``'s logits -- is held against the fixture's own float32-versus-float64 distance
    by the project's bound

        |ours - f64| <= 8 |reference fp32 - f64| + 2e-6 max|f64|            (max norm per figure)

    and each figure is printed before it is asserted.  The feature memory's first draw, the source accuracies, the
    pseudo labels of the model steps, the arg-max, the selected rows and the neighbour sets of the ``test_time_loss``
    calls the fixture stores, the coalesced edge list and the final edge list are discrete: equal."""
    assert np.array_equal(got["mem0"], f["mem0"])
    bad = []
    for k in ("src_losses", "model", "steps", "p_iter", "w_iter", "new_feat", "edge_weight", "logits"):
        f64, ref32 = f["f64/" + k].astype(np.float64), f[k].astype(np.float64)
        assert got[k].shape == f64.shape, (k, got[k].shape, f64.shape)
        if f64.size == 0:                                               # the figures a stopped fit does not reach
            assert str(f["stopped"])
            continue
        e_ours, e_ref = np.abs(got[k] - f64).max(), np.abs(ref32 - f64).max()
        lim = 8 * e_ref + 2e-6 * max(np.abs(f64).max(), 1e-30)
        print(f"{k}: |ours - f64| = {e_ours:.3e}, |reference fp32 - f64| = {e_ref:.3e}, bound {lim:.3e}")
        if not e_ours <= lim:
            bad.append(k)
    keep = f["tt_pred"].shape[0]
    n = got["tt_pred"].shape[1]
    assert got["tt_pred"].shape[0] == f["steps"].shape[0]
    want = dict(accs=f["accs"], model_pred=f["model_pred"], tt_pred=f["tt_pred"], tt_near=f["tt_near"],
                tt_sel=np.unpackbits(f["tt_sel"], axis=1)[:, :n].astype(bool), coalesced_ei=f["coalesced_ei"],
                edge_index=f["edge_index"])
    assert np.array_equal(f["accs"], f["f64/accs"]) and np.array_equal(f["edge_index"], f["f64/edge_index"])
    for k, w in want.items():
        g = got[k][:keep] if k.startswith("tt_") else got[k]
        same = g.shape == w.shape and np.array_equal(g, w)
        where = "" if same or g.shape != w.shape else f", first at {np.argwhere(g != w)[:6].tolist()}"
        print(f"{k}: {'equal' if same else 'DIFFERS'}{where}")
        if not same:
            bad.append(k)
    # a fit the reference's sample_final_edges stops (fixture b) stops here with the same message, after the same rounds
    print(f"stopped: {str(got['stopped'])!r}, the reference: {str(f['stopped'])!r}")
    assert bool(str(f["stopped"])) == (not bool(f["make_undirected"]))
    if str(got["stopped"]) != str(f["stopped"]):
        bad.append("stopped")
    assert not bad, bad


@pytest.mark.parametrize("name", FIXTURES)
def test_host_fit_agrees_with_the_fixture_recorded_from_the_reference(name):
    f, s, t = fixture(name)
    m, got = run_fit(f, s, t, "cpu")
    assert float(np.abs(got["p_iter"] - 1e-7).max()) < 1e-12          # the flip weights do not move, as in the reference
    check_fit_against_fixture(got, f)


def test_signature_is_the_reference_s_and_the_alias_resolves():
    from pygda_amd.models import GraphCTA
    import pygda.models
    assert pygda.models.GraphCTA is GraphCTA
    sig = inspect.signature(GraphCTA.__init__)
    want = [("in_dim", inspect._empty), ("hid_dim", inspect._empty), ("num_classes", inspect._empty), ("num_layers", 3),
            ("dropout", 0.), ("act", F.relu), ("loop_model", 3), ("loop_adj", 1), ("loop_feat", 4), ("ratio", 0.1), ("K", 5),
            ("tau", 0.2), ("lamb", 0.2), ("momentum", 0.9), ("make_undirected", True), ("weight_decay", 0.), ("lr", 1e-4),
            ("epoch", 500), ("gnn", 'gcn'), ("device", 'cuda:0'), ("batch_size", 0), ("num_neigh", -1), ("verbose", 2)]
    got = [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "kwargs")]
    assert got == want
    from tests.golden import _ref_loader
    ref_file = os.path.join(_ref_loader.REF, "pygda", "models", "graphcta.py")
    if os.path.isfile(ref_file):                                        # the reference checkout, where there is one
        import ast
        tree = ast.parse(open(ref_file).read())
        init = next(n for c in tree.body if isinstance(c, ast.ClassDef) for n in c.body
                    if isinstance(n, ast.FunctionDef) and n.name == "__init__")
        assert [a.arg for a in init.args.args[1:]] == [k for k, _ in want]


def test_refusals_name_their_argument():
    from pygda_amd.models import GraphCTA
    for kw, word in ((dict(gnn='sage'), "gnn"), (dict(batch_size=32), "batch_size"), (dict(loop_adj=2), "loop_adj")):
        with pytest.raises(NotImplementedError, match=word):
            GraphCTA(16, 16, 3, device="cpu", **kw)
    with pytest.raises(ValueError, match="loop_feat"):
        GraphCTA(16, 16, 3, device="cpu", loop_feat=0, loop_adj=0)
    f, s, t = fixture(FIXTURES[0])
    with pytest.raises(ValueError, match="neighbours"):
        GraphCTA(16, 16, 3, device="cpu", K=300).fit(s, t)
    from pygda_amd import distributed
    old = distributed.active
    distributed.active = lambda: True
    try:
        with pytest.raises(NotImplementedError, match="data-parallel"):
            GraphCTA(16, 16, 3, device="cpu").fit(s, t)
    finally:
        distributed.active = old
