"""DMGNN without a GPU: the trainer's public surface (pygda/models/dmgnn.py), what it rejects before any device work,
the state dict and init stream against the reference-run fixture, the host fit against the fixture with the bound
taken from the float64 restatement, each host op against that restatement (a batch with an all-zero PPMI row and a
batch with E = A E exactly among them), the C ABI's argument checks, and the fixture's regeneration."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import _lib, ops
from pygda_amd.data import Data
from tests.conftest import GOLDEN, load_golden
from tests.golden import _dmgnn_semantics

KW = dict(in_dim=24, hid_dim=16, num_classes=3, n_emb=12, pair_weight=0.1, step=3, dropout=0.0, lr=0.01,
          weight_decay=0.001, batch_size=40)


def _pair(g):
    return (Data(x=torch.tensor(g["src_x"]), edge_index=torch.tensor(g["src_ei"]), y=torch.tensor(g["src_y"])),
            Data(x=torch.tensor(g["tgt_x"]), edge_index=torch.tensor(g["tgt_ei"]), y=torch.tensor(g["tgt_y"])))


def check_fit_against_fixture(got, g):
    """ACDNE's bound for the losses, both predict outputs and the final parameters: |ours - f64| <= 2 |ref32 - f64| +
    1e-6 max(|f64|, 1), each figure printed before it is asserted; the accuracies are equal."""
    for k in ["losses", "tgt_out", "src_out"] + [k for k in g if k.startswith("final/")]:
        f64, ref32 = g["f64/" + k].astype(np.float64), g[k].astype(np.float64)
        floor = 1e-6 * max(np.abs(f64).max(), 1.0)
        err, lim = np.abs(got[k] - f64).max(), 2 * np.abs(ref32 - f64).max() + floor
        print(f"{k}: |ours - f64| = {err:.3e}, bound {lim:.3e}")
        assert err <= lim, f"{k}: {err:.3e} > {lim:.3e}"
    np.testing.assert_array_equal(got["accs"], g["accs"])


def run_fit(device, **extra):
    g = load_golden("dmgnn_fit3")
    s, t = _pair(g)
    log = []
    m = pygda_amd.models.DMGNN(device=device, epoch=3, verbose=0, **KW, **extra)
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    torch.manual_seed(int(g["seeds"][0]))
    np.random.seed(int(g["seeds"][1]))
    m.fit(s, t)
    out = dict(losses=np.array([l for l, _ in log]), accs=np.array([a for _, a in log]),
               tgt_out=m.predict(t)[0].cpu().numpy(), src_out=m.predict(s, train=True)[0].cpu().numpy())
    out.update({"final/" + k: v.cpu().numpy() for k, v in m.dmgnn.state_dict().items()})
    return out


def test_dmgnn_signature_and_defaults():
    from pygda_amd.models import DMGNN, BaseGDA
    sig = inspect.signature(DMGNN.__init__)
    want = dict(num_layers=0, n_emb=128, pair_weight=0.1, step=3, dropout=0., act=F.relu, weight_decay=0., lr=4e-3,
                epoch=200, device='cuda:0', batch_size=100, num_neigh=-1, verbose=2)
    names = list(sig.parameters)
    assert names[:4] == ["self", "in_dim", "hid_dim", "num_classes"]
    assert names[4:-1] == list(want) and names[-1] == "kwargs"
    for k, v in want.items():
        assert sig.parameters[k].default == v, k
    assert issubclass(DMGNN, BaseGDA)


def test_pygda_alias_resolves_dmgnn():
    import pygda
    from pygda.models import DMGNN
    assert DMGNN is pygda_amd.models.DMGNN and pygda.models.DMGNN is DMGNN
    assert "DMGNN" in pygda.__doc__ and "DMGNN" in pygda_amd.models.__all__


def test_dmgnn_rejects_what_it_does_not_run_before_any_device_work(monkeypatch):
    from pygda_amd.models import DMGNN
    import pygda_amd.models.acdne as A
    g = load_golden("dmgnn_fit3")
    s, t = _pair(g)
    monkeypatch.setattr(A, "acdne_process_graph", None)          # any device work would fail on this
    for bs in (0, 1):
        with pytest.raises(ValueError, match="DMGNN: batch_size"):
            DMGNN(24, 16, 3, batch_size=bs, device="cuda:0").fit(s, t)
    with pytest.raises(ValueError, match="at least"):
        DMGNN(24, 16, 3, batch_size=300, device="cpu").fit(s, t)           # 150 rows > 130 target nodes
    with pytest.raises(ValueError, match="rows per domain"):
        big = Data(x=torch.rand(300, 24), edge_index=s.edge_index, y=torch.arange(300) % 3)
        DMGNN(24, 16, 3, batch_size=258, device="cuda:0").fit(big, big)
    with pytest.raises(ValueError, match="num_classes"):
        DMGNN(24, 16, 4, batch_size=40, device="cuda:0").fit(s, t)
    import pygda_amd.distributed as dist
    monkeypatch.setattr(dist, "active", lambda: True)
    m = DMGNN(24, 16, 3, device="cuda:0")
    with pytest.raises(NotImplementedError, match="DMGNN: data-parallel"):
        m.fit(s, t)
    assert getattr(m, "dmgnn", None) is None and not hasattr(m, "acdne")


def test_state_dict_keys_and_init_stream_match_the_reference():
    g = load_golden("dmgnn_fit3")
    init = {k[len("init/"):]: v for k, v in g.items() if k.startswith("init/")}
    m = pygda_amd.models.DMGNN(device="cpu", **KW)
    torch.manual_seed(int(g["seeds"][0]))
    sd = m.init_model().state_dict()
    assert list(sd) == list(init)
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), init[k], err_msg=k)


def test_the_float64_restatement_reproduces_the_fixture():
    g = load_golden("dmgnn_fit3")
    init = {k[len("init/"):]: v for k, v in g.items() if k.startswith("init/")}
    sem = _dmgnn_semantics.fit(dict(x=g["src_x"], ei=g["src_ei"], y=g["src_y"]),
                               dict(x=g["tgt_x"], ei=g["tgt_ei"], y=g["tgt_y"]), init, 16, 12, 3, 3, 0.1, 0.01, 0.001,
                               3, 40, int(g["seeds"][1]))
    np.testing.assert_array_equal(sem["losses"], g["f64/losses"])
    np.testing.assert_allclose(sem["losses"], g["losses"], rtol=1e-6)         # the fp32 reference, a few ulps
    np.testing.assert_allclose(sem["tgt_out"], g["tgt_out"], atol=1e-5)
    np.testing.assert_array_equal(sem["accs"], g["accs"])


def test_fixture_keeps_fp32_near_ties_out_of_the_argmax():
    """The generator's condition, re-read from the file: top-2 gap of every float64 row > 100 x the fp32 error."""
    g = load_golden("dmgnn_fit3")
    for k in ("epoch_src_out", "src_out", "tgt_out"):
        f64, ref32 = g["f64/" + k], g[k].astype(np.float64)
        f64, ref32 = f64.reshape(-1, *f64.shape[-2:]), ref32.reshape(-1, *ref32.shape[-2:])
        for e in range(f64.shape[0]):
            top = np.sort(f64[e], axis=1)
            assert (top[:, -1] - top[:, -2]).min() > 100 * np.abs(ref32[e] - f64[e]).max(), (k, e)


def test_host_fit_matches_the_reference_fixture():
    check_fit_against_fixture(run_fit("cpu"), load_golden("dmgnn_fit3"))


def test_host_step_ops_match_the_reference_step():
    """``step/`` of the fixture: the reference's own batch_ppmi blocks, nei_prox_loss values and propagated logits of
    one batch (node 7, whose PPMI row is all zero, is not in it; the next test has it)."""
    g = load_golden("dmgnn_fit3")
    ppmi_s, _ = ops.acdne_process_graph(torch.tensor(g["src_ei"]), torch.tensor(g["src_x"]), 160, 3)
    ppmi_t, _ = ops.acdne_process_graph(torch.tensor(g["tgt_ei"]), torch.tensor(g["tgt_x"]), 130, 3)
    pidx = torch.tensor(np.concatenate([g["step/idx_s"], g["step/idx_t"]]))
    emb = torch.tensor(g["step/emb"])
    prox, gprox, a = ops.dmgnn_prox(ppmi_s, ppmi_t, pidx, emb, 20, 0.1)       # relu(emb) = emb
    np.testing.assert_allclose(a[0].numpy(), g["step/a_s"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(a[1].numpy(), g["step/a_t"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(prox.numpy(), g["step/prox"], rtol=1e-5)
    assert prox.dtype == torch.float64 and gprox.dtype == torch.float32 and gprox.shape == emb.shape
    wc, bc = torch.tensor(g["final/node_classifier.layer.weight"]), torch.tensor(g["final/node_classifier.layer.bias"])
    logit = F.linear(emb, wc, bc)
    prop = logit + torch.cat([a[0] @ logit[:20], a[1] @ logit[20:]])
    np.testing.assert_allclose(prop.numpy(), g["step/logits"], atol=1e-5)


def _step64(ppmi_s, ppmi_t, pidx, rows, z, y, params, alpha, pw):
    """The float64 restatement of one step: loss and gradients in z and the eight head parameters by autograd."""
    from tests.golden._acdne_semantics import batch_block
    h = z.size(0) // 2
    names = ["node_classifier.layer", "domain_discriminator.h_dann_1", "domain_discriminator.h_dann_2",
             "domain_discriminator.output_layer"]
    P64 = [p.double().requires_grad_(True) for p in params]
    P = {}
    for k, n in enumerate(names):
        P[n + ".weight"], P[n + ".bias"] = P64[2 * k], P64[2 * k + 1]
    z64 = z.double().requires_grad_(True)
    a_s = torch.tensor(batch_block(ppmi_s.double().numpy(), pidx[:h].numpy()))
    a_t = torch.tensor(batch_block(ppmi_t.double().numpy(), pidx[h:].numpy()))
    total, parts = _dmgnn_semantics.step_loss(torch.relu(z64), a_s, a_t, P, y[rows[:h]], alpha, pw)
    grads = torch.autograd.grad(total, [z64] + P64, allow_unused=True)
    return total.detach(), grads, parts, torch.stack([a_s, a_t])


def _check_step(got, want64):
    (loss, dz, grads), (total64, g64) = got, want64
    print(f"loss {loss.item():.9g} f64 {total64.item():.9g}")
    np.testing.assert_allclose(loss.item(), total64.item(), rtol=2e-5)
    for name, a, b in zip(["dz", "Wc", "bc", "W1", "b1", "W2", "b2", "W3", "b3"], [dz] + list(grads), g64):
        b = b.cpu().numpy()
        err = np.abs(a.cpu().double().numpy() - b).max()
        print(f"{name}: {err:.3e} (max |f64| {np.abs(b).max():.3e})")
        assert np.isfinite(a.cpu().numpy()).all(), name
        assert err <= 2e-5 * max(np.abs(b).max(), 1e-3), f"{name}: {err:.3e}"


def _head_params(c, e, gen):
    return [torch.randn(c, e, generator=gen) * 0.3, torch.randn(c, generator=gen) * 0.1,
            torch.randn(128, e, generator=gen) * 0.2, torch.randn(128, generator=gen) * 0.1,
            torch.randn(128, 128, generator=gen) * 0.1, torch.randn(128, generator=gen) * 0.1,
            torch.randn(2, 128, generator=gen) * 0.1, torch.randn(2, generator=gen) * 0.1]


def test_host_ops_against_the_float64_restatement_with_an_all_zero_ppmi_row():
    g = load_golden("dmgnn_fit3")
    ppmi_s, _ = ops.acdne_process_graph(torch.tensor(g["src_ei"]), torch.tensor(g["src_x"]), 160, 3)
    ppmi_t, _ = ops.acdne_process_graph(torch.tensor(g["tgt_ei"]), torch.tensor(g["tgt_x"]), 130, 3)
    assert not ppmi_s[7].any() and not ppmi_t[7].any()                     # the isolated node of each domain
    gen = torch.Generator().manual_seed(5)
    h, e, c = 20, 12, 3
    pidx = torch.cat([torch.randperm(160, generator=gen)[:h], torch.randperm(130, generator=gen)[:h]])
    pidx[3], pidx[h + 5] = 7, 7
    rows = torch.cat([pidx[:h], pidx[h:] + 160])
    z = torch.randn(2 * h, e, generator=gen)
    y = torch.tensor(g["src_y"])
    params = _head_params(c, e, gen)
    total64, g64, parts, a64 = _step64(ppmi_s, ppmi_t, pidx, rows, z, y, params, 0.7, 0.1)
    prox, gprox, a = ops.dmgnn_prox(ppmi_s, ppmi_t, pidx, z, h, 0.1)
    assert not a[0, 3].any() and not a[1, 5].any()                         # 0 / (0 + 1e-12): a zero row, not NaN
    np.testing.assert_allclose(a.double().numpy(), a64.numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(prox.numpy(), parts["prox"].detach().numpy(), rtol=2e-5)
    _check_step(ops.dmgnn_heads(z, gprox, a, params, y, rows, 0.7, prox, 0.1), (total64, g64))


def test_host_heads_with_zero_blocks_are_acdne_heads():
    """``L + mm(0, L)`` changes no finite logit: DMGNN's heads with all-zero blocks return ACDNE's loss, dz and eight
    gradients exactly."""
    gen = torch.Generator().manual_seed(9)
    h, e, c = 20, 12, 3
    z, gprox = torch.randn(2 * h, e, generator=gen), torch.randn(2 * h, e, generator=gen) * 0.01
    rows = torch.cat([torch.randperm(160, generator=gen)[:h], torch.randperm(130, generator=gen)[:h] + 160])
    y = torch.randint(0, c, (160,), generator=gen)
    params = _head_params(c, e, gen)
    prox = torch.tensor([0.3, 0.4], dtype=torch.float64)
    want = ops.acdne_heads(z, gprox, params, y, rows, 0.7, prox, 0.1)
    got = ops.dmgnn_heads(z, gprox, torch.zeros(2, h, h), params, y, rows, 0.7, prox, 0.1)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and len(got[2]) == len(want[2]) == 8
    for a, b in zip(got[2], want[2]):
        assert torch.equal(a, b)


def test_host_prox_with_e_equal_to_a_e_has_a_zero_finite_gradient():
    """|E - A E|_F = 0 exactly: a cyclic-shift PPMI block (every row one entry 1.0, so the scale is exactly 1) with all
    embedding rows equal, and the all-zero embedding.  torch's rule for ``norm`` at zero: the gradient is zero."""
    n, h, e = 30, 20, 12
    shift = torch.zeros(n, n)
    shift[torch.arange(n), (torch.arange(n) + 1) % n] = 1.0
    ring = torch.cat([torch.arange(h), torch.arange(h)])                      # rows 0..19: row 19 -> column 20: absent
    full = torch.zeros(h, h)
    full[torch.arange(h), (torch.arange(h) + 1) % h] = 1.0                    # a closed ring inside the batch
    row = torch.rand(1, e) + 0.5
    for z in (row.expand(2 * h, e).contiguous(), -torch.ones(2 * h, e)):
        prox, gprox, a = ops.dmgnn_prox(full, full, ring, z, h, 0.1)
        assert torch.equal(a[0], full) and prox.tolist() == [0.0, 0.0]
        assert torch.isfinite(gprox).all() and not gprox.any()
    prox, gprox, _ = ops.dmgnn_prox(shift, shift, ring, row.expand(2 * h, e).contiguous(), h, 0.1)
    assert prox[0] > 0 and torch.isfinite(gprox).all() and gprox.any()        # the open ring: row 19 has no neighbour


def test_host_predict_is_p_plus_ppmi_p():
    gen = torch.Generator().manual_seed(2)
    n, e, c = 50, 12, 3
    z, w, b = torch.randn(n, e, generator=gen), torch.randn(c, e, generator=gen), torch.randn(c, generator=gen)
    ppmi = torch.rand(n, n, generator=gen) * (torch.rand(n, n, generator=gen) < 0.2)
    p64 = torch.softmax(torch.relu(z.double()) @ w.double().T + b.double(), 1)
    want = p64 + ppmi.double() @ p64
    np.testing.assert_allclose(ops.dmgnn_predict(z, w, b, ppmi).numpy(), want.numpy(), rtol=1e-5, atol=1e-6)


def test_c_abi_argument_checks_return_errors_on_the_host():
    """Status codes for bad arguments come back before anything touches a device."""
    L = _lib.lib()
    one = ctypes.c_void_p(64)
    prox = lambda **kw: L.gda_dmgnn_prox_f32(*[kw.get(k, v) for k, v in (                    # noqa: E731
        ("ps", one), ("ld_s", 160), ("ns", 160), ("pt", one), ("ld_t", 132), ("nt", 130), ("pidx", one), ("z", one),
        ("h", 20), ("e", 12), ("pw", 0.1), ("loss", one), ("gz", one), ("a", one), ("ws", one),
        ("wsb", L.gda_dmgnn_prox_workspace_bytes(20, 12)), ("stream", None))])
    assert prox(h=0) == -2 and prox(h=129) == -2 and prox(e=0) == -2 and prox(e=4097) == -2     # h, e out of range
    assert prox(ld_s=159) == -2 and prox(ld_t=129) == -2                                        # rows shorter than n
    assert prox(ns=0) == -2
    assert prox(ps=None) == -1 and prox(a=None) == -1 and prox(loss=None) == -1 and prox(ws=None) == -1
    assert prox(h=21) == -3 and prox(e=13) == -3 and prox(wsb=0) == -3                         # shapes the workspace was not sized for
    assert L.gda_dmgnn_prox_workspace_bytes(20, 12) == 2 * 20 * 12 * 4
    P8 = (ctypes.c_void_p * 8)(*[64] * 8)
    heads = lambda **kw: L.gda_dmgnn_heads_f32(*[kw.get(k, v) for k, v in (                  # noqa: E731
        ("z", one), ("gprox", one), ("a", one), ("h", 20), ("e", 12), ("c", 3), ("w", P8), ("y", one), ("ny", 160),
        ("rows", one), ("alpha", one), ("prox", one), ("pw", 0.1), ("dz", one), ("g", P8), ("loss", one),
        ("acc", None), ("ws", one), ("wsb", L.gda_dmgnn_heads_workspace_bytes(20, 12, 3)), ("stream", None))])
    assert heads(h=0) == -2 and heads(h=129) == -2 and heads(c=0) == -2 and heads(c=4097) == -2 and heads(ny=0) == -2
    assert heads(a=None) == -1 and heads(z=None) == -1 and heads(w=None) == -1
    assert heads(w=(ctypes.c_void_p * 8)(*([64] * 7 + [None]))) == -1
    assert heads(c=4) == -3 and heads(h=21) == -3 and heads(wsb=0) == -3
    assert L.gda_dmgnn_heads_workspace_bytes(20, 12, 3) % 8 == 0                               # the double terms behind the floats
    pred = lambda **kw: L.gda_dmgnn_predict_f32(*[kw.get(k, v) for k, v in (                 # noqa: E731
        ("z", one), ("n", 130), ("e", 12), ("wc", one), ("bc", one), ("c", 3), ("ppmi", one), ("ld", 132),
        ("out", one), ("ws", one), ("wsb", L.gda_dmgnn_predict_workspace_bytes(130, 3)), ("stream", None))])
    assert pred(n=0) == -2 and pred(ld=128) == -2 and pred(c=0) == -2 and pred(e=0) == -2      # ld < n: not [n, n]
    assert pred(ppmi=None) == -1 and pred(out=None) == -1 and pred(ws=None) == -1
    assert pred(ld=131) == -4 and pred(ppmi=ctypes.c_void_p(68)) == -4                         # 16-byte loads
    assert pred(n=131, ld=132) == -3 and pred(c=4) == -3
    with pytest.raises(_lib.GdaError, match="gda_dmgnn_prox_f32 failed with status -2"):
        _lib.call("gda_dmgnn_prox_f32", one, 160, 160, one, 132, 130, one, one, 200, 12, 0.1, one, one, one, one, 0, None)


def test_dmgnn_bytes_counts_one_pass_over_the_ppmi():
    prox, heads, predict = ops.dmgnn_bytes(8935, 8936, 50, 128, 5)
    assert predict >= 4 * 8935 * 8936 and predict - 4 * 8935 * 8936 < 0.02 * predict
    assert prox > 0 and heads > ops.acdne_bytes(1, 0, 0, 0, 50, 128, 5)[3]


def test_fixture_regenerates_bit_for_bit(tmp_path):
    from tests.golden import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not available")
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "tests.golden.make_golden_dmgnn", "--out", str(tmp_path)], cwd=root,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = np.load(os.path.join(GOLDEN, "dmgnn_fit3.npz")), np.load(tmp_path / "dmgnn_fit3.npz")
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
