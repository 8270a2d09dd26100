"""KBL without a GPU: the host fallbacks of ``ops.kbl_pair_bce`` / ``ops.kbl_bridge_topk`` against float64 brute-force
restatements written here (the yardsticks of tests/test_gpu_kbl.py, with the inputs and shape lists both files share),
the modules' state-dict names and the pair draws against the fixtures recorded from the reference's own kbl.py
(tests/golden/make_golden_kbl.py), host fits against those fixtures, the within-domain quirk, ``predict``'s row slicing,
the refusals, the signature, and the argument checks of gda_kbl.hip's C ABI."""
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

HERE = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ("kbl_fit_a.npz", "kbl_fit_b.npz", "kbl_fit_c.npz")        # c: live dropout, host parity only
PAIR_SHAPES = [(1, 4, 1, 1), (67, 20, 5, 9), (300, 128, 200, 200), (300, 256, 70, 130)]            # (n, d, ma, mb)
TOPK_SHAPES = [(1, 1, 128, 1), (67, 53, 128, 20), (300, 260, 128, 20), (300, 260, 20, 64), (515, 1030, 128, 256)]
TOPK_SEEDS = (0, 1, 2)
GAP = 1e-5          # the float64 gap asked of the k-th against the (k+1)-th cosine: over 30 float32 cosine errors (3e-7)


# ---- the float64 yardsticks ------------------------------------------------------------------------------------------------
def brute_pair_bce(u, ia, ib, y):
    """``(loss, dU)``: every pair of the Cartesian product spelled out -- rows over max(|row|, 1e-8), the ``[ma, mb]``
    cosines, the sigmoid, the BCE with both logarithms clamped at -100 -- and autograd's gradient."""
    u = u.detach().clone().requires_grad_(True)
    uh = u / u.norm(dim=1, keepdim=True).clamp_min(1e-8)
    s = torch.sigmoid(uh[ia] @ uh[ib].t())
    same = (y[ia][:, None] == y[ib][None, :]).to(u.dtype)
    loss = -(same * torch.log(s).clamp_min(-100) + (1 - same) * torch.log1p(-s).clamp_min(-100)).mean()
    loss.backward()
    return loss.detach(), u.grad


def brute_bridge_topk(a, b, k):
    """``(row, col, val, gap)`` over the full ``[na, nb]`` cosine array by (cosine descending, flat index ascending), NaN
    as +inf; ``gap`` the difference of the k-th and the (k+1)-th cosine (inf when there is no (k+1)-th)."""
    ah = a / a.norm(dim=1, keepdim=True).clamp_min(1e-8)
    bh = b / b.norm(dim=1, keepdim=True).clamp_min(1e-8)
    cos = (ah @ bh.t()).reshape(-1).numpy().copy()
    cos[np.isnan(cos)] = np.inf
    order = np.lexsort((np.arange(cos.size), -cos))
    top = order[:k]
    gap = float(cos[order[k - 1]] - cos[order[k]]) if k < cos.size else float("inf")
    nb = b.size(0)
    return (torch.from_numpy(top // nb), torch.from_numpy(top % nb), torch.sigmoid(torch.from_numpy(cos[top])), gap)


# ---- the inputs both test files use ------------------------------------------------------------------------------------------
def pair_inputs(n, d, ma, mb, one_class=False):
    """Gaussian rows with, where there is room, a zero row (1), two identical rows (2, 3: cosine 1) and two opposite
    rows (4, 5); index lists that repeat entries and name all of those; three classes, or one."""
    g = torch.Generator().manual_seed(1000 * n + 10 * d + ma + mb)
    u = torch.randn(n, d, generator=g, dtype=torch.float64)
    if n >= 6:
        u[1] = 0
        u[3] = u[2]
        u[5] = -u[4]
    ia = torch.randint(0, n, (ma,), generator=g)
    ib = torch.randint(0, n, (mb,), generator=g)
    if n >= 6 and ma >= 5 and mb >= 5:
        ia[:5] = torch.tensor([1, 2, 4, 2, 0])
        ib[:5] = torch.tensor([3, 5, 1, 3, 0])
    y = torch.zeros(n, dtype=torch.long) if one_class else torch.randint(0, 3, (n,), generator=g)
    return u, ia, ib, y


def topk_inputs(na, nb, d, seed=0, variant=""):
    """``torch.randn`` rows from generator ``seed``; ``variant='dup'`` copies the target row of the best pair onto its
    neighbour (two pairs tie exactly at the top), ``variant='nan'`` makes source row 0 NaN."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(na, d, generator=g, dtype=torch.float64)
    b = torch.randn(nb, d, generator=g, dtype=torch.float64)
    if variant == "dup":
        _, col, _, _ = brute_bridge_topk(a, b, 1)
        b[(int(col[0]) + 1) % nb] = b[int(col[0])]
    if variant == "nan":
        a[0] = float("nan")
    return a, b


def close(ours, f32, f64, name, slack=2e-6):
    """The project's bound (tests/test_gpu_cwgcn._close), each figure printed before it is asserted."""
    ours, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                      for v in (ours, f32, f64))
    e_ours, e_ref = np.abs(ours - f64).max(), np.abs(f32 - f64).max()
    lim = 8 * e_ref + slack * max(np.abs(f64).max(), 1e-30)
    print(f"{name}: |ours - f64| = {e_ours:.3e}, |fp32 torch - f64| = {e_ref:.3e}, bound {lim:.3e}")
    assert e_ours <= lim, f"{name}: |ours - f64| = {e_ours:.3e} > {lim:.3e} (fp32 torch {e_ref:.3e})"


def pair_yardstick(u, ia, ib, y, dtype):
    """``ops.kbl_pair_bce``'s host fallback -- the reference's torch composition -- with its gradient, in ``dtype``."""
    v = u.detach().to(dtype).clone().requires_grad_(True)
    loss = ops.kbl_pair_bce(v, ia, ib, y)
    loss.backward()
    return loss.detach(), v.grad


# ---- the op fallbacks against the brute force --------------------------------------------------------------------------------
@pytest.mark.parametrize("one_class", [False, True])
@pytest.mark.parametrize("shape", PAIR_SHAPES)
def test_pair_bce_fallback_is_the_brute_force(shape, one_class):
    u, ia, ib, y = pair_inputs(*shape, one_class=one_class)
    want, dwant = brute_pair_bce(u, ia, ib, y)
    got, dgot = pair_yardstick(u, ia, ib, y, torch.float64)
    scale = max(float(dwant.abs().max()), 1e-30)          # (a zero row's gradient is g / 1e-8: the largest by far)
    assert abs(float(got - want)) <= 1e-12 and float((dgot - dwant).abs().max()) <= 1e-12 * scale
    got32, dgot32 = pair_yardstick(u, ia, ib, y, torch.float32)
    assert abs(float(got32) - float(want)) <= 1e-5 and float((dgot32.double() - dwant).abs().max()) <= 1e-4 * scale + 1e-6
    assert torch.isfinite(dwant).all() and (shape[0] < 6 or float(dwant[1].abs().max()) > 0)     # the zero row has a gradient


def test_pair_bce_clamps_are_torch_s():
    """The norm clamp at 1e-8 decides a tiny row; the log clamp at -100 cannot be reached through a sigmoid of [-1, 1]."""
    u = torch.tensor([[1e-9, 0.0], [3.0, 4.0]], dtype=torch.float64)
    ia, ib, y = torch.tensor([0]), torch.tensor([1]), torch.tensor([0, 1])
    want, _ = brute_pair_bce(u, ia, ib, y)
    cos = (1e-9 / 1e-8) * 0.6
    assert abs(float(want) + np.log1p(-1 / (1 + np.exp(-cos)))) < 1e-15
    assert abs(float(ops.kbl_pair_bce(u, ia, ib, y)) - float(want)) < 1e-15


def check_topk(got, a, b, k, name):
    """The set of pairs equals float64's (asserted to be decided), values non-increasing, indices in range."""
    row, col, val, gap = brute_bridge_topk(a, b, k)
    assert gap >= GAP, f"{name}: the float64 gap at the boundary is {gap:.2e}"
    grow, gcol, gval = (v.cpu() for v in got)
    assert grow.shape == (k,) and int(grow.min()) >= 0 and int(grow.max()) < a.size(0)
    assert int(gcol.min()) >= 0 and int(gcol.max()) < b.size(0)
    nb = b.size(0)
    assert set((grow.long() * nb + gcol.long()).tolist()) == set((row * nb + col).tolist()), name
    assert bool((gval[1:] <= gval[:-1]).all()), name
    return row, col, val


@pytest.mark.parametrize("seed", TOPK_SEEDS)
@pytest.mark.parametrize("shape", TOPK_SHAPES)
def test_bridge_topk_fallback_is_the_brute_force(shape, seed):
    na, nb, d, k = shape
    a, b = topk_inputs(na, nb, d, seed)
    row, col, val = check_topk(ops.kbl_bridge_topk(a, b, k), a, b, k, "float64")
    g = ops._kbl_bridge_topk_chunked(a, b, k, rows=37)                       # several chunks, a short last one
    assert torch.equal(g[0], row) and torch.equal(g[1], col) and float((g[2] - val).abs().max()) < 1e-15
    g32 = ops.kbl_bridge_topk(a.float(), b.float(), k)
    check_topk(g32, a, b, k, "float32")
    order = torch.argsort(g32[0] * nb + g32[1]), torch.argsort(row * nb + col)
    assert float((g32[2][order[0]].double() - val[order[1]]).abs().max()) < 1e-6


@pytest.mark.parametrize("shape", TOPK_SHAPES[1:])
def test_bridge_topk_fallback_keeps_ties_in_flat_order_and_ranks_nan_first(shape):
    na, nb, d, k = shape
    a, b = topk_inputs(na, nb, d, variant="dup")
    row, col, val, gap = brute_bridge_topk(a, b, k)
    assert gap >= GAP and int(row[0]) == int(row[1]) and float(val[0]) == float(val[1])
    for dtype in (torch.float64, torch.float32):
        g = ops.kbl_bridge_topk(a.to(dtype), b.to(dtype), k)
        assert g[0][:2].tolist() == row[:2].tolist() and g[1][:2].tolist() == col[:2].tolist()
        assert int(g[1][0]) < int(g[1][1])
    a, b = topk_inputs(na, nb, d, variant="nan")
    g = ops.kbl_bridge_topk(a.float(), b.float(), k)
    m = min(k, nb)
    assert g[0][:m].tolist() == [0] * m and g[1][:m].tolist() == list(range(m)) and bool((g[2][:m] == 1).all())


def test_bridge_topk_refuses_k_out_of_range():
    a, b = topk_inputs(5, 4, 8)
    for k in (0, 21):
        with pytest.raises(_lib.GdaError, match="out of range"):
            ops.kbl_bridge_topk(a, b, k)
    assert ops.kbl_bridge_topk(a, b, 20)[0].numel() == 20


# ---- the C ABI's argument checks (no launch) ---------------------------------------------------------------------------------
def test_c_abi_refuses_bad_sizes_and_pointers():
    L = _lib.lib()
    buf = (ctypes.c_float * 4200)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    at = lambda k: ctypes.c_void_p(p.value + k)
    pair = lambda n, d, ma, mb, ws=p, nbytes=1 << 30, u=p, du=None: L.gda_kbl_pair_bce_f32(
        u, p, p, p, n, d, ma, mb, p, du or at(1024), ws, nbytes, None)
    assert pair(0, 4, 2, 2) == -2 and pair(4, 257, 2, 2) == -2 and pair(4, 4, 1025, 2) == -2 and pair(4, 4, 2, 0) == -2
    assert pair(4, 4, 2, 2, ws=None) == -1 and pair(4, 4, 2, 2, nbytes=16) == -3 and pair(4, 4, 2, 2, u=at(2)) == -4
    assert pair(4, 4, 2, 2, du=p) == -5                                                    # GDA_E_ALIAS
    assert L.gda_kbl_pair_bce_workspace_bytes(128, 200, 200) >= 4 * (2 * 200 * 128 * 2)
    topk = lambda na, nb, d, k, ws=p, nbytes=1 << 30: L.gda_kbl_bridge_topk_f32(p, p, na, nb, d, k, p, p, p, ws, nbytes,
                                                                                 None)
    assert topk(0, 4, 4, 1) == -2 and topk(4, 4, 4, 0) == -2 and topk(4, 4, 4, 17) == -2 and topk(40, 40, 4, 257) == -4
    assert topk(4, 4, 4, 4, ws=None) == -1 and topk(4, 4, 4, 4, nbytes=16) == -3
    assert L.gda_kbl_bridge_topk_workspace_bytes(7410, 5578, 128, 20) < 4 * (7410 + 5578) * 128 + (1 << 20)
    assert ops.KBL_MAX_K == 256 and ops.KBL_MAX_PAIR_ROWS == 1024 and ops.KBL_MAX_WIDTH == 256


# ---- the modules and the trainer against the fixtures ------------------------------------------------------------------------
def fixture(name):
    f = np.load(os.path.join(HERE, name))
    lng = lambda k: torch.from_numpy(f[k].astype(np.int64))
    s = Data(x=torch.from_numpy(f["src_x"]), edge_index=lng("src_ei"), y=lng("src_y"),
             train_mask=torch.from_numpy(f["train_mask"]), val_mask=torch.from_numpy(f["val_mask"]),
             test_mask=torch.from_numpy(f["test_mask"]))
    t = Data(x=torch.from_numpy(f["tgt_x"]), edge_index=lng("tgt_ei"), y=lng("tgt_y"))
    return f, s, t


def initial_state(f):
    """The recorded state: floating tensors are stored as integers on the fixture's grid."""
    out = {}
    for key in f.files:
        if key.startswith("init/"):
            v = f[key]
            out[key[5:]] = torch.from_numpy(v.astype(np.int64)) if "num_batches" in key else \
                torch.from_numpy(v.astype(np.float32) / np.float32(f["grid"]))
    return out


def run_fit(f, s, t, device, **kw):
    """A fit of the fixture's configuration from its initial state under its seeds (the draws are then the
    reference's); what :func:`check_fit_against_fixture` reads."""
    from pygda_amd.models import KBL
    seeds = [int(v) for v in f["seeds"]]
    live = bool(f["live_dropout"])
    drop = {} if live else dict(encoder_dropout=0., clf_dropout=0., gnn_dropout=0.)

    def load(model):
        model.load_state_dict(initial_state(f))
        torch.manual_seed(seeds[3])

    m = KBL(16, 16, int(f["src_y"].max()) + 1, k_cross=int(f["k_cross"]), k_within=int(f["k_within"]), lr=float(f["lr"]),
            epoch=int(f["epochs"]), device=device, verbose=0, bridge_epochs=int(f["num_epoch"]), init_hook=load,
            **drop, **kw)
    torch.manual_seed(seeds[0])
    random.seed(seeds[1])
    np.random.seed(seeds[2])
    m.fit(s, t)
    cpu = lambda v: v.detach().double().cpu().numpy()
    got = dict(ia=m.pair_lists[0].numpy(), ib=m.pair_lists[1].numpy(), stage1=np.array(m.bridge_log, dtype=np.float64),
               cross_row=m.bridge_edges[0].numpy(), cross_col=m.bridge_edges[1].numpy(), cross_val=cpu(m.bridge_edges[2]),
               merged_ei=m.stored_data.edge_index.cpu().numpy(), losses=np.array([l for l, _ in m.train_log]),
               accs=np.array([a for _, a in m.train_log]), logits=cpu(m.predict(t)[0]))
    got.update({"running/" + k: cpu(v) for k, v in m.kbl.bridged_graph.model.state_dict().items()
                if "running_" in k or "num_batches" in k})
    if m.within_edges is not None:
        for d, ei, val in zip(("src", "tgt"), m.within_edges, m.within_values):
            got[f"within_{d}_ei"], got[f"within_{d}_val"] = ei.numpy(), cpu(val)
    return m, got


def check_fit_against_fixture(got, f):
    """Every recorded float figure -- the five stage-1 losses per epoch, the BatchNorm running statistics after stage 1,
    the bridge edges' values, the within-domain values, the stage-3 losses and ``predict``'s output -- is held against
    the fixture's own float32-versus-float64 distance by the project's bound

        |ours - f64| <= 8 |reference fp32 - f64| + 2e-6 max|f64|            (max norm per figure)

    and printed before it is asserted.  The pair lists, the accuracies, the bridge edge set, the within-domain edges and
    the merged edge list are discrete: equal."""
    bad = []
    floats = ["stage1", "cross_val", "losses", "logits"] + [k for k in f.files if k.startswith("running/")] + \
        [k for k in f.files if k.startswith("within_") and k.endswith("_val")]
    for k in floats:
        f64, ref32 = f["f64/" + k].astype(np.float64), f[k].astype(np.float64)
        ours = got[k]
        if k == "cross_val":                                            # by pair: the order inside the set may differ
            ours = ours[np.argsort(got["cross_row"] * 100000 + got["cross_col"])]
            by_pair = np.argsort(f["cross_row"].astype(np.int64) * 100000 + f["cross_col"])
            f64, ref32 = f64[by_pair], ref32[by_pair]
        assert ours.shape == f64.shape, (k, ours.shape, f64.shape)
        e_ours, e_ref = np.abs(ours - f64).max(), np.abs(ref32 - f64).max()
        lim = 8 * e_ref + 2e-6 * max(np.abs(f64).max(), 1e-30)
        print(f"{k}: |ours - f64| = {e_ours:.3e}, |reference fp32 - f64| = {e_ref:.3e}, bound {lim:.3e}")
        if not e_ours <= lim:
            bad.append(k)
    pairs = lambda row, col: sorted(zip(np.asarray(row).tolist(), np.asarray(col).tolist()))
    want = dict(ia=f["ia"], ib=f["ib"], accs=f["accs"], merged_ei=f["merged_ei"])
    want.update({k: f[k] for k in f.files if k.startswith("within_") and k.endswith("_ei")})
    for k, w in want.items():
        same = got[k].shape == w.shape and np.array_equal(got[k], w)
        print(f"{k}: {'equal' if same else 'DIFFERS'}")
        if not same:
            bad.append(k)
    same = pairs(got["cross_row"], got["cross_col"]) == pairs(f["cross_row"], f["cross_col"])
    print(f"bridge edge set: {'equal' if same else 'DIFFERS'}")
    if not same:
        bad.append("bridge edges")
    assert not bad, bad


def test_state_dict_names_are_the_reference_s():
    from pygda_amd.nn import KBLBase
    f, s, t = fixture(FIXTURES[0])
    net = KBLBase(s, t, "cpu", k_cross=20, k_within=6, num_epoch=6, norm_mode='None')
    state = initial_state(f)
    assert set(net.state_dict()) == set(state)
    net.load_state_dict(state)                                            # strict: shapes and names
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in state.items()}
    # a fresh model draws every bias that PyG's Linear draws
    fresh = KBLBase(s, t, "cpu").bridged_graph.model.source_learner.sim_net
    assert all(float(l.bias.detach().abs().max()) > 0 for l in (fresh.biasatt[0], fresh.biasatt[2], fresh.lin_clf))


@pytest.mark.parametrize("name", FIXTURES[:2])
def test_pair_enumerator_draws_the_reference_s_pairs(name):
    from pygda_amd.nn.kbl_base import PairEnumerator, enumerate_pairs
    f, s, _ = fixture(name)
    np.random.seed(int(f["seeds"][2]))
    enum = PairEnumerator(s, mode='train')
    for epoch in range(int(f["num_epoch"])):
        state = np.random.get_state()
        ia, ib = enum.sampling_lists(max_class_num=2, sample_size=40000)
        assert np.array_equal(ia.numpy(), f["ia"][epoch]) and np.array_equal(ib.numpy(), f["ib"][epoch])
        assert bool(s.train_mask[ia].all()) and bool(s.train_mask[ib].all()) and ia.numel() == 200
        np.random.set_state(state)
        i1, i2 = enum.sampling(max_class_num=2, sample_size=40000, shuffle=False)          # the same draws, enumerated
        e1, e2 = enumerate_pairs(ia, ib)
        assert i1.numel() == 40000 and torch.equal(i1, e1) and torch.equal(i2, e2)
        assert i1[:3].tolist() == ia[:3].tolist() and i2[:3].tolist() == [int(ib[0])] * 3


def test_pairnorm_modes():
    from pygda_amd.nn.kbl_base import PairNorm
    x = torch.randn(9, 5, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    c = x - x.mean(dim=0)
    assert torch.equal(PairNorm('None')(x), x)
    assert torch.allclose(PairNorm('PN', 2)(x), 2 * c / (1e-6 + c.pow(2).sum(1).mean()).sqrt())
    assert torch.allclose(PairNorm('PN-SI', 2)(x), 2 * c / (1e-6 + c.pow(2).sum(1, keepdim=True)).sqrt())
    assert torch.allclose(PairNorm('PN-SCS', 2)(x), 2 * x / (1e-6 + x.pow(2).sum(1, keepdim=True)).sqrt() - x.mean(dim=0))


@pytest.mark.parametrize("name", FIXTURES)
def test_host_fit_agrees_with_the_fixture_recorded_from_the_reference(name):
    f, s, t = fixture(name)
    m, got = run_fit(f, s, t, "cpu")
    check_fit_against_fixture(got, f)


def test_within_domain_edges_are_the_reference_s_ties():
    """Every recorded within-domain value is the maximal one, sigmoid(1): ``topk`` chose among ties, and torch's CPU
    ``topk`` chose the flat indices 0 .. k - 1 -- the edges (0, 0 .. k - 1) -- which the port reproduces."""
    f, s, t = fixture(FIXTURES[0])
    k = int(f["k_within"])
    top = float(torch.sigmoid(torch.ones((), dtype=torch.float32)))
    for d in ("src", "tgt"):
        assert np.all(f[f"within_{d}_val"] == top) and np.all(np.abs(f[f"f64/within_{d}_val"] - 1 / (1 + np.exp(-1))) < 1e-15)
        assert sorted(f[f"within_{d}_flat"].tolist()) == list(range(k))
        assert f[f"within_{d}_ei"].tolist() == [[0] * k, list(range(k))]
    m, got = run_fit(f, s, t, "cpu")
    for d in ("src", "tgt"):
        assert np.array_equal(got[f"within_{d}_ei"], f[f"within_{d}_ei"])


def small_fit(s, t, **kw):
    from pygda_amd.models import KBL
    torch.manual_seed(5)
    np.random.seed(6)
    m = KBL(16, 16, 3, k_cross=5, k_within=2, epoch=1, device="cpu", verbose=0, bridge_epochs=1, **kw)
    m.fit(s, t)
    return m


def test_predict_returns_the_last_rows_of_the_stored_graph():
    f, s, t = fixture(FIXTURES[0])
    m = small_fit(s, t)
    full, y = m.predict(t)
    assert full.shape == (t.x.shape[0], 3) and y is t.y
    assert m.stored_data.x.shape[0] == s.x.shape[0] + t.x.shape[0] and bool(m.stored_data.central_mask[:s.x.shape[0]].all())
    assert int(m.stored_data.central_mask.sum()) == s.x.shape[0]
    part = Data(x=torch.zeros(50, 16), edge_index=torch.zeros(2, 0, dtype=torch.long), y=t.y[:50])     # its graph is ignored
    assert torch.equal(m.predict(part)[0], full[-50:])
    ei = m.stored_data.edge_index
    key = ei[0] * m.stored_data.n + ei[1]
    assert torch.equal(key, torch.unique(key))                            # coalesced: sorted, no duplicate
    assert set(zip(ei[0].tolist(), ei[1].tolist())) == set(zip(ei[1].tolist(), ei[0].tolist()))            # undirected


def test_signature_is_the_reference_s_and_the_alias_resolves():
    from pygda_amd.models import KBL
    import pygda.models
    assert pygda.models.KBL is KBL
    sig = inspect.signature(KBL.__init__)
    want = [("in_dim", inspect._empty), ("hid_dim", inspect._empty), ("num_classes", inspect._empty), ("k_cross", 50),
            ("k_within", 10), ("num_layers", 2), ("dropout", 0.), ("act", F.relu), ("weight_decay", 5e-3), ("lr", 1e-3),
            ("epoch", 200), ("device", 'cuda:0'), ("batch_size", 0), ("num_neigh", -1), ("verbose", 2)]
    extras = [("bridge_epochs", 400), ("bridge_hidden", 64), ("bridge_lr", 1e-3), ("bridge_weight_decay", 5e-3),
              ("encoder_dropout", 0.5), ("clf_dropout", 0.6), ("gnn_dropout", 0.1)]
    params = [(k, v) for k, v in sig.parameters.items() if k not in ("self", "kwargs")]
    assert [(k, v.default) for k, v in params] == want + extras
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in params[len(want):])


def test_refusals_name_their_argument():
    from pygda_amd.models import KBL
    with pytest.raises(NotImplementedError, match="batch_size"):
        KBL(16, 16, 3, device="cpu", batch_size=32)
    f, s, t = fixture(FIXTURES[0])
    bare = Data(x=s.x, edge_index=s.edge_index, y=s.y)
    with pytest.raises(ValueError, match="train_mask"):
        KBL(16, 16, 3, device="cpu").fit(bare, t)
    broken = Data(x=t.x, edge_index=t.edge_index.clone(), y=t.y)
    broken.edge_index[1, 0] = t.x.shape[0]
    with pytest.raises(ValueError, match="edge_index"):
        KBL(16, 16, 3, device="cpu").fit(s, broken)
    from pygda_amd import distributed
    old = distributed.active
    distributed.active = lambda: True
    try:
        with pytest.raises(NotImplementedError, match="data-parallel"):
            KBL(16, 16, 3, device="cpu").fit(s, t)
    finally:
        distributed.active = old
    # a missing val_mask / test_mask counts as all false
    only_train = Data(x=s.x, edge_index=s.edge_index, y=s.y, train_mask=s.train_mask)
    m = small_fit(only_train, t)
    assert not bool(m.stored_data.val_mask.any()) and not bool(m.stored_data.test_mask.any())
    assert int(m.stored_data.train_mask.sum()) == int(s.train_mask.sum())
