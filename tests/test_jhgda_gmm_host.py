"""JHGDA's opt-in mixture pseudo-labels (``pseudo='gmm'``) without a GPU: the constructor's surface and refusals, the
CPU trainer on a planted pair (its log, its epoch-0 labels against a by-hand ``GMMClustering.forward``), the condition
that float32 and float64 agree on every label and iteration count of that pair, the fallback on a singular covariance,
and the argument checks of the new C entry points.  tests/test_gpu_jhgda_gmm.py takes its inputs from here."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib
from pygda_amd.data import Data

OK, NULL, SIZE, WORKSPACE, UNSUPPORTED, ALIAS = 0, -1, -2, -3, -4, -5
C, NS, NT, IN_DIM, HID = 3, 240, 210, 16, 8
SEP = 6.0                  # distance between class centres in units of the noise's sigma, per informative coordinate
KW = dict(num_layers=2, pool_ratio=0.2, lr=4e-3, verbose=0)
# The mixture's settings on the planted pair.  reg_covar: the embeddings come from 16 input columns, so at hid_dim 33
# a cluster's covariance has rank <= 16 and sklearn's default 1e-6 would leave its condition to float32's rounding.
GMM = dict(pseudo="gmm", gmm_reg_covar=1e-2)
SEEDS = {8: 9, 33: 25}      # initial models whose classifier labels every class somewhere (searched on the CPU)


# ------------------------------------------------------------------------------------------------ the planted pair --
def _domain(n, seed, shift):
    """``n`` nodes in ``C`` planted classes: features = the class centre (``SEP`` sigma apart) plus unit noise and a
    domain shift; a homophilous graph (9 in 10 edges inside a class), both directions listed."""
    rng = np.random.RandomState(seed)
    y = np.arange(n) % C
    rng.shuffle(y)
    centres = np.zeros((C, IN_DIM))
    for c in range(C):
        centres[c, c * 4:(c + 1) * 4] = SEP
    x = centres[y] + rng.normal(size=(n, IN_DIM)) + shift
    src = rng.randint(0, n, 4 * n)
    same = rng.rand(4 * n) < 0.9
    dst = np.empty_like(src)
    for e, (a, s) in enumerate(zip(src, same)):
        pool = np.flatnonzero((y == y[a]) if s else (y != y[a]))
        dst[e] = pool[rng.randint(len(pool))]
    ei = np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])])
    return x, ei, y


@functools.lru_cache(maxsize=None)
def planted_pair(duplicated=False):
    """(source, target) ``Data`` in float64.  ``duplicated``: every target row is one of ``C`` distinct rows and every
    node carries the same edges as its twin, so each class's embeddings coincide: a singular covariance."""
    xs, eis, ys = _domain(NS, 11, 0.0)
    xt, eit, yt = _domain(NT, 12, 0.3)
    if duplicated:
        xt = xt[np.argsort(yt, kind="stable")[::NT // C]][yt]            # one row per class
        eit = np.stack([np.arange(NT), np.arange(NT)])                   # self loops only: twins stay twins
    mk = lambda x, ei, y: Data(x=torch.tensor(x, dtype=torch.float64), edge_index=torch.tensor(ei, dtype=torch.int64),
                               y=torch.tensor(y, dtype=torch.int64))
    return mk(xs, eis, ys), mk(xt, eit, yt)


def fit(device, dtype, epochs=3, duplicated=False, hid=HID, seed=None, **kw):
    """One fit of the planted pair; returns the trainer, its log and, per epoch, what ``pseudo_label`` saw and gave
    (``z_s, y_s, z_t, y_t_pseudo`` and the classifier's labels, on the CPU).  The model is initialised in float32 and
    converted, so that fits of both precisions start from the same values."""
    s, t = planted_pair(duplicated)
    s, t = (Data(x=d.x.to(dtype), edge_index=d.edge_index, y=d.y) for d in (s, t))
    m = pygda_amd.models.JHGDA(IN_DIM, hid, C, device=device, epoch=epochs, **{**KW, **kw})
    log, seen = [], []
    m.epoch_hook = lambda e, loss, acc, secs: log.append((loss, acc))
    build = m.init_model

    def init_model(**kwargs):
        torch.set_default_dtype(torch.float32)                        # the same initial values in both precisions
        net = build(**kwargs).to(dtype)
        torch.set_default_dtype(dtype)
        inner = net.pseudo_label

        def pseudo_label(z_s, y_s, z_t, *a, **k):
            out = inner(z_s, y_s, z_t, *a, **k)
            if not torch.cuda.is_available() or not torch.cuda.is_current_stream_capturing():
                start = net.cls_model(z_t).argmax(1)
                seen.append(tuple(v.detach().cpu().clone() for v in (z_s, y_s, z_t, out, start)))
            return out

        net.pseudo_label = pseudo_label
        return net

    m.init_model = init_model
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        torch.manual_seed(SEEDS[hid] if seed is None else seed)
        m.fit(s, t)
    finally:
        torch.set_default_dtype(old)
    return m, log, seen


@functools.lru_cache(maxsize=None)
def cpu_fit(dtype, **kw):
    return fit("cpu", dtype, **kw)


def labels_of(seen):
    return [e[3].argmax(1).numpy() for e in seen]


# ------------------------------------------------------------------------------------------------------- surface --
def test_constructs_and_refuses_by_name():
    m = pygda_amd.models.JHGDA(IN_DIM, HID, C, device="cpu", pseudo="gmm", gmm_max_iter=20, gmm_tol=1e-4,
                               gmm_reg_covar=1e-5, gmm_smooth_r=0.5)
    assert (m.pseudo, m.gmm_max_iter, m.gmm_tol, m.gmm_reg_covar, m.gmm_smooth_r) == ("gmm", 20, 1e-4, 1e-5, 0.5)
    d = pygda_amd.models.JHGDA(IN_DIM, HID, C, device="cpu")
    assert (d.pseudo, d.gmm_max_iter, d.gmm_tol, d.gmm_reg_covar, d.gmm_smooth_r) == ("classifier", 100, 1e-3, 1e-6, None)
    with pytest.raises(ValueError, match="pseudo"):
        pygda_amd.models.JHGDA(IN_DIM, HID, C, device="cpu", pseudo="kmeans")
    with pytest.raises(ValueError, match="classwise"):
        pygda_amd.models.JHGDA(IN_DIM, HID, C, device="cpu", pseudo="gmm", classwise=False, pool_ratio=1.0)
    with pytest.raises(ValueError, match="hid_dim"):
        pygda_amd.models.JHGDA(IN_DIM, 129, C, device="cuda:0", pseudo="gmm")
    with pytest.raises(ValueError, match="num_classes"):
        pygda_amd.models.JHGDA(IN_DIM, HID, 33, device="cuda:0", pseudo="gmm")
    pygda_amd.models.JHGDA(IN_DIM, 129, 33, device="cpu", pseudo="gmm")        # the limits are the kernels'
    pygda_amd.models.JHGDA(IN_DIM, 129, 33, device="cuda:0")                   # and the mixture's alone
    from pygda_amd.nn import JHGDABase
    with pytest.raises(ValueError, match="pseudo"):
        JHGDABase(IN_DIM, HID, C, "cpu", 0.2, NS, NT, classwise=True, pseudo="other")


# --------------------------------------------------------------------------------------------------- CPU trainer --
def test_cpu_fit_logs_and_matches_a_by_hand_forward():
    from pygda_amd.nn.gmm_clustering import GMMClustering, get_emb_centers
    m, log, seen = cpu_fit(torch.float64, **GMM)
    assert len(m.gmm_log) == 3 and len(log) == 3 and len(seen) == 3
    for n_iter, converged, fell_back, lower in m.gmm_log:
        assert 1 <= n_iter <= 100 and converged == 1 and fell_back == 0 and np.isfinite(lower)
    assert all(np.isfinite(l) for l, _ in log)
    # epoch 0 by hand.  The classifier's labels come from the initial model, which the seed reproduces.
    z_s, y_s, z_t, got, _ = seen[0]
    m0, _, seen0 = cpu_fit(torch.float64, epochs=1)                   # pseudo='classifier': the same first forward
    assert torch.equal(seen0[0][2], z_t)
    resp0 = seen0[0][3]
    g = GMMClustering(C, "cpu", n_init=1, reg_covar=GMM["gmm_reg_covar"])
    out = g.forward(get_emb_centers(z_s, y_s, C), z_t, None, None, None, False, None, resp0=resp0)
    assert np.array_equal(out["label"].numpy(), got.argmax(1).numpy())
    assert (g.gmm.n_iter_, int(g.gmm.converged_)) == m.gmm_log[0][:2] and g.gmm.lower_bound_ == m.gmm_log[0][3]
    assert got.sum(1).eq(1).all() and got.shape == (NT, C)


def test_float32_and_float64_agree_on_every_label_and_iteration_count():
    """DESIGN 4.27's rule for comparing fits across precisions, as a condition on this input."""
    for kw in (GMM, dict(GMM, gmm_smooth_r=0.5), dict(GMM, hid=33)):
        m64, _, seen64 = cpu_fit(torch.float64, **kw)
        m32, _, seen32 = cpu_fit(torch.float32, **kw)
        print(kw, m64.gmm_log, m32.gmm_log)
        assert [e[:3] for e in m64.gmm_log] == [e[:3] for e in m32.gmm_log]
        assert all(e[2] == 0 for e in m64.gmm_log)
        for a, b in zip(labels_of(seen64), labels_of(seen32)):
            assert np.array_equal(a, b)
        # room to spare, epoch by epoch on the float64 fit's embeddings: a tolerance a quarter tighter or wider keeps
        # the iteration count (float32 moves the lower bound by about 1e-5, a hundredth of the tolerance), and no row's
        # winning responsibility is within 1e-3 of the runner-up (float32 moves one by about 1e-5: test_gpu_gmm.py)
        from pygda_amd.nn.gmm_clustering import GMMClustering
        for (z_s, y_s, z_t, out, start), entry in zip(seen64, m64.gmm_log):
            z = z_t.double()
            resp0 = torch.eye(C, dtype=torch.float64)[start]
            counts = []
            for tol in (8e-4, 1e-3, 1.25e-3):
                g = GMMClustering(C, "cpu", n_init=1, tol=tol, reg_covar=GMM["gmm_reg_covar"])
                counts.append(g.fit_em(z, resp0).n_iter_)
                if tol == 1e-3:
                    top = torch.sort(g.gmm.predict_proba(z), dim=1, descending=True)[0]
                    assert float((top[:, 0] - top[:, 1]).min()) > 1e-3
            assert counts == [entry[0]] * 3, (counts, entry)


def test_singular_covariance_falls_back_to_the_classifier_fit_exactly():
    mg, logg, seeng = cpu_fit(torch.float64, duplicated=True, pseudo="gmm", gmm_reg_covar=0.0)
    mc, logc, seenc = cpu_fit(torch.float64, duplicated=True)
    assert [e[2] for e in mg.gmm_log] == [1, 1, 1] and mc.gmm_log == []
    assert logg == logc and mg.lm_log == mc.lm_log
    for a, b in zip(mg.jhgda.state_dict().values(), mc.jhgda.state_dict().values()):
        assert torch.equal(a, b)
    for a, b in zip(seeng, seenc):
        assert torch.equal(a[3], b[3])


# ----------------------------------------------------------------------------------------------- ABI refusals --
def P(addr):
    return ctypes.c_void_p(addr)


X, LAB, SUMS, CNT, WS, TGT, SRC, C2L, SHUF, ST, RESP, PROB, HOT, COST = (P(0x1000 * k) for k in range(1, 15))
BIG = 1 << 40


def label_sums(x=X, ldx=130, n=100, d=128, k=6, lab=LAB, sums=SUMS, cnt=CNT, ws=WS, ws_bytes=BIG):
    return _lib.lib().gda_gmm_label_sums_f32(x, ldx, n, d, k, lab, sums, cnt, ws, ws_bytes, None)


def lsa_cos(tgt=TGT, src=SRC, k=6, d=128, c2l=C2L, shuf=SHUF, st=ST):
    return _lib.lib().gda_lsa_cos_f32(tgt, src, k, d, c2l, shuf, st, None)


def lsa_cost(cost=COST, k=6, c2l=C2L, shuf=SHUF, st=ST):
    return _lib.lib().gda_lsa_cost_f64(cost, k, c2l, shuf, st, None)


def relabel(resp=RESP, n=100, k=6, c2l=C2L, shuf=SHUF, fb=LAB, st=ST, prob=PROB, lab=LAB, hot=HOT):
    return _lib.lib().gda_gmm_relabel_f32(resp, n, k, c2l, shuf, fb, st, prob, lab, hot, None)


def test_new_entry_points_validate_their_arguments():
    for missing in ("x", "lab", "sums", "cnt"):
        assert label_sums(**{missing: None}) == NULL, missing
    for bad in ("n", "d", "k"):
        assert label_sums(**{bad: -1}) == SIZE and label_sums(**{bad: 0}) == SIZE, bad
    assert label_sums(ldx=127) == SIZE
    assert label_sums(d=129, ldx=129) == UNSUPPORTED and label_sums(k=33) == UNSUPPORTED
    L = _lib.lib()
    assert L.gda_gmm_label_sums_workspace_bytes(100, 128, 6) == 2 * 6 * 129 * 4        # two blocks of 64 rows
    assert label_sums(ws=None, ws_bytes=0) == WORKSPACE and label_sums(ws_bytes=2 * 6 * 129 * 4 - 1) == WORKSPACE
    for missing in ("tgt", "src", "c2l", "shuf"):
        assert lsa_cos(**{missing: None}) == NULL, missing
    for bad in ("k", "d"):
        assert lsa_cos(**{bad: -1}) == SIZE and lsa_cos(**{bad: 0}) == SIZE, bad
    assert lsa_cos(k=33) == UNSUPPORTED and lsa_cos(d=129) == UNSUPPORTED
    for missing in ("cost", "c2l", "shuf"):
        assert lsa_cost(**{missing: None}) == NULL, missing
    assert lsa_cost(k=0) == SIZE and lsa_cost(k=-1) == SIZE and lsa_cost(k=33) == UNSUPPORTED
    for missing in ("resp", "lab"):
        assert relabel(**{missing: None}) == NULL, missing
    assert relabel(c2l=None) == NULL and relabel(shuf=None) == NULL          # both permutations or neither
    for bad in ("n", "k"):
        assert relabel(**{bad: -1}) == SIZE and relabel(**{bad: 0}) == SIZE, bad
    assert relabel(k=33) == UNSUPPORTED and relabel(n=1 << 31) == SIZE
