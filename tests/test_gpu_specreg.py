"""GPU: SpecReg's critic update, gap and spectral hinges (csrc/gda_critic3.hip) against the float64 restatements of
tests/test_specreg_host.py on that file's cases, and the trainer that runs on them.

One bound for every kernel (tests/test_gpu_gat.close): |gpu - f64| <= 8 |fp32 torch - f64| + 2e-6 max|f64|, the fp32 term
being the reference's own formulation (autograd's double backward) in float32 on the CPU; the figures are printed per
output.  Every device op runs twice and has to return the same bits."""
import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops, profiler
from pygda_amd.data import Data, to_undirected
from tests import test_specreg_host as H
from tests.conftest import load_golden
from tests.test_gpu_gat import close, same_bits
from tests.test_gpu_parity import SPECREG_KW, _no_dropout, _specreg_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0


def dev_inputs(name):
    return {k: v.to(DEV) for k, v in H.inputs(name).items()}


def run_grads(x):
    out = (torch.full((1,), SENTINEL, device=DEV),) + tuple(torch.full_like(x[k], SENTINEL) for k in H.PARAMS)
    ops.critic3_grads(x["es"], x["et"], tuple(x[k] for k in H.PARAMS), out)
    return dict(zip(H.KEYS, (out[0].reshape(()), *out[1:])))


# ---- (1) the critic update ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.CASES))
def test_critic3_grads_vs_float64(name):
    """Loss and the six gradients on every case (every tile count of the row kernel, its zero fill at h = 8 | 12 | 100,
    one-row domains, the second trip of its grid, the row without an input gradient) into sentinel-filled outputs."""
    x = dev_inputs(name)
    got, again = run_grads(x), run_grads(x)
    assert all(same_bits(got[k], again[k]) for k in H.KEYS)
    f64, f32 = H.critic3_refs(name)
    for k in H.KEYS:
        assert got[k].shape == f64[k].shape and bool(torch.isfinite(got[k]).all()), f"{name}/{k}"
        close(got[k], f32[k], f64[k], f"critic3/{name}/{k}")


def test_critic3_takes_unaligned_encodings():
    """4-byte-aligned storage runs the same path: the same bits as the 16-byte-aligned copy."""
    x = dev_inputs("full_tile_plus_row")
    want = run_grads(x)
    y = dict(x)
    for k in ("es", "et"):
        buf = torch.empty(x[k].numel() + 1, device=DEV)
        y[k] = buf[1:].view_as(x[k])
        y[k].copy_(x[k])
        assert y[k].data_ptr() % 16 == 4
    got = run_grads(y)
    assert all(same_bits(got[k], want[k]) for k in H.KEYS)


# ---- (2) the update with Adam inside --------------------------------------------------------------------------------
def _leaf_params(x):
    params = [torch.nn.Parameter(x[k].clone()) for k in H.PARAMS]
    for p in params:
        p.grad = torch.zeros_like(p)
    return params


def run_adam(name, inside):
    from pygda_amd.optim import Adam
    x = dev_inputs(name)
    params = _leaf_params(x)
    opt = Adam(params, H.ADAM_LR)
    loss = torch.zeros(1, device=DEV)
    for _ in range(H.ADAM_STEPS):
        if inside:
            assert ops.critic3_adam(x["es"], x["et"], params, opt, loss)
        else:
            ops.critic3_grads(x["es"], x["et"], params, (loss, *(p.grad for p in params)))
            opt.step()
    return params, opt


@pytest.mark.parametrize("name", ["golden_width_ragged_tile", "full_tile_plus_row", "several_tiles"])
def test_critic3_adam_vs_float64_and_vs_separate_step(name):
    params, opt = run_adam(name, inside=True)
    f64, f32, same_masks = H.adam_refs(name)
    assert same_masks
    x = H.inputs(name)
    for k, p in zip(H.PARAMS, params):
        # (gb3 = sum sigma is -1 + 1 = 0 in the float32 and float64 yardsticks alike: Adam leaves b3 where it is)
        assert k == "b3" or not torch.equal(p.detach().cpu(), x[k]), f"{k} did not move"
        close(p.detach(), f32[k], f64[k], f"critic3_adam/{name}/{k}")
    apart, opt2 = run_adam(name, inside=False)
    for p, q in zip(params, apart):
        assert same_bits(p.detach(), q.detach()) and same_bits(p.grad, q.grad)
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert same_bits(opt.state[p][key].reshape(-1), opt2.state[q][key].reshape(-1)), key
    assert float(opt.state[params[0]]["step"]) == H.ADAM_STEPS


def test_critic3_adam_refuses_other_optimisers():
    from pygda_amd.optim import Adam
    x = dev_inputs("full_tile_plus_row")
    loss = torch.full((1,), SENTINEL, device=DEV)
    for make in (lambda ps: torch.optim.Adam(ps, H.ADAM_LR),
                 lambda ps: Adam(ps + [torch.nn.Parameter(torch.zeros(3, device=DEV))], H.ADAM_LR)):
        params = _leaf_params(x)
        before = [p.detach().clone() for p in params]
        opt = make(list(params))
        calls = []
        orig = _lib.call
        try:
            _lib.call = lambda name, *a: calls.append(name) or orig(name, *a)
            assert ops.critic3_adam(x["es"], x["et"], params, opt, loss) is False
        finally:
            _lib.call = orig
        assert not calls and float(loss) == SENTINEL
        assert all(same_bits(p.detach(), b) for p, b in zip(params, before))
        assert all(bool((p.grad == 0).all()) for p in params)


# ---- (3) the gap ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["golden_width_ragged_tile", "one_row_target", "one_row_source_h100", "several_tiles"])
def test_critic3_gap_vs_float64(name):
    x = dev_inputs(name)
    gout = 1.7
    outs = []
    for _ in range(2):
        es, et = x["es"].clone().requires_grad_(), x["et"].clone().requires_grad_()
        params = [x[k].clone().requires_grad_() for k in H.PARAMS]
        value = ops.critic3_gap(es, et, *params)
        (value * gout).backward()
        assert all(p.grad is None for p in params)               # no gradient for the critic from the encoder's term
        outs.append(dict(value=value.detach(), ges=es.grad, get=et.grad))
    assert all(same_bits(outs[0][k], outs[1][k]) for k in outs[0])
    h = H.inputs(name)
    f64, f32 = (H.gap_ref(h["es"], h["et"], *(h[k] for k in H.PARAMS), gout, dt) for dt in (torch.float64, torch.float32))
    for k in ("value", "ges", "get"):
        assert outs[0][k].shape == f64[k].shape
        close(outs[0][k], f32[k], f64[k], f"critic3_gap/{name}/{k}")
    with torch.no_grad():                                         # no gradient wanted: the value alone, the same bits
        assert same_bits(ops.critic3_gap(x["es"], x["et"], *(x[k] for k in H.PARAMS)), outs[0]["value"])


# ---- (4) the spectral hinges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in H.HINGE_CASES if n != "both_off"])
def test_spectral_hinge_vs_float64(name):
    _, _, _, ts, tm, _ = H.HINGE_CASES[name]
    eivec, enc = (t.to(DEV) for t in H.hinge_inputs(name))
    outs = []
    for _ in range(2):
        e = enc.clone().requires_grad_()
        value = ops.spectral_hinge(eivec, e, ts, H.GAMMA_SMOOTH, tm, H.GAMMA_MFR)
        (value * 1.3).backward()
        outs.append((value.detach(), e.grad))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    f64, f32 = H.hinge_refs(name)
    assert float(f64["value"]) > 0
    close(outs[0][0], f32["value"], f64["value"], f"spectral_hinge/{name}/value")
    close(outs[0][1], 1.3 * f32["grad"], 1.3 * f64["grad"], f"spectral_hinge/{name}/grad")


def test_spectral_hinge_off_launches_nothing(monkeypatch):
    _, _, _, ts, tm, _ = H.HINGE_CASES["both_off"]
    eivec, enc = (t.to(DEV) for t in H.hinge_inputs("both_off"))
    enc.requires_grad_()
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name) or orig(name, *a))
    value = ops.spectral_hinge(eivec, enc, ts, H.GAMMA_SMOOTH, tm, H.GAMMA_MFR)
    assert not calls and float(value) == 0.0 and value.shape == () and not value.requires_grad


# ---- (5) the trainer is off the library ------------------------------------------------------------------------------
class _Recorder:
    """Wraps torch.autograd.grad, F.linear, torch.matmul and Tensor.__matmul__; keeps the calls that touch the critic's
    width ``h`` (any tensor argument with an extent of h: the critic's layers, the encodings, eivec's product with them)
    and every autograd.grad."""

    def __init__(self, h):
        self.h, self.calls, self.saved = h, [], []

    def _wrap(self, owner, attr, always=False):
        orig = getattr(owner, attr)
        rec = self

        def wrapped(*a, **k):
            if always or any(torch.is_tensor(t) and rec.h in t.shape for t in a):
                rec.calls.append(attr)
            return orig(*a, **k)

        self.saved.append((owner, attr, orig))
        setattr(owner, attr, wrapped)

    def __enter__(self):
        self._wrap(torch.autograd, "grad", always=True)
        self._wrap(torch.nn.functional, "linear")
        self._wrap(torch, "matmul")
        self._wrap(torch.Tensor, "__matmul__")
        return self

    def __exit__(self, *exc):
        for owner, attr, orig in reversed(self.saved):
            setattr(owner, attr, orig)
        return False


def _golden_model():
    """The model of tests/test_gpu_parity.test_specreg_forward_model_golden, built as that test builds it."""
    g = load_golden("specreg")
    s, t = _specreg_pair(g)
    m = pygda_amd.models.SpecReg(12, 8, 3, **SPECREG_KW)
    torch.manual_seed(int(g["init_seed"]))
    m.udagcn = m.init_model()
    _no_dropout(m.udagcn)
    m.critic = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8),
                                   torch.nn.ReLU(), torch.nn.Linear(8, 1)).to(DEV)
    m.optimizer_critic = torch.optim.Adam(m.critic.parameters(), m.lr)
    m.use_fused_critic = True
    return m, s.to(DEV), t.to(DEV), int(g["epoch"])


def _random_pair(ns, nt, k, seed):
    gen = torch.Generator().manual_seed(seed)

    def domain(n):
        ei = to_undirected(torch.randint(0, n, (2, 4 * n), generator=gen), n)
        d = Data(x=(torch.rand(n, 12, generator=gen) < 0.2).float(), edge_index=ei, y=torch.randint(0, 3, (n,), generator=gen))
        d.eivec = torch.randn(k, n, generator=gen) / n ** 0.5
        return d

    return domain(ns), domain(nt)


def _wide_model(h, critic=None, **kw):
    from pygda_amd.optim import Adam
    s, t = _random_pair(300, 260, 100, 5)
    m = pygda_amd.models.SpecReg(12, h, 3, num_layers=2, ppmi=False, thr_smooth=0.1, thr_mfr=0.1, device=DEV, epoch=3,
                                 verbose=0, **kw)
    torch.manual_seed(3)
    m.udagcn = m.init_model()
    _no_dropout(m.udagcn)
    m.critic = (critic if critic is not None else
                torch.nn.Sequential(torch.nn.Linear(h, h), torch.nn.ReLU(), torch.nn.Linear(h, h), torch.nn.ReLU(),
                                    torch.nn.Linear(h, 1))).to(DEV)
    m.optimizer_critic = Adam(m.critic.parameters(), m.lr)
    m.use_fused_critic = True
    return m, s.to(DEV), t.to(DEV), 1


@pytest.mark.parametrize("which", ["golden_h8", "h128"])
def test_forward_model_reaches_no_library_product(which):
    """Between the encodings and the entropy term -- the critic loop, the gap, the regulariser -- and in their backward,
    nothing calls autograd.grad, F.linear, matmul or ``@`` on anything of the critic's width."""
    m, s, t, epoch = _golden_model() if which == "golden_h8" else _wide_model(128)
    h = m.hid_dim
    before = [p.detach().clone() for p in m.critic.parameters()]
    with _Recorder(h) as rec:
        loss, _, _ = m.forward_model(s, t, 0.05, epoch)
        loss.backward()
    assert not rec.calls, rec.calls
    moved = [not torch.equal(p.detach(), b) for p, b in zip(m.critic.parameters(), before)]
    assert bool(torch.isfinite(loss)) and all(moved[:5])          # (the last bias has no gradient: sum sigma = 0)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.udagcn.parameters() if p.requires_grad and p.grad is not None)


# ---- (6) switch off against on, three steps -------------------------------------------------------------------------
def _loop_on_device(fused):
    """tests/test_specreg_host.loop_ref's loop through ``SpecReg.forward_model`` on the GPU: same data, same initial encoder
    and critic, ``torch.optim.Adam`` on the encoder, the critic optimiser ``fit()`` would build for the path."""
    from pygda_amd.optim import Adam
    L = H.LOOP
    src, tgt, state, crit = H.loop_data()
    datas = []
    for d in (src, tgt):
        g = Data(x=d["x"].clone(), edge_index=d["ei"].clone(), y=d["y"].clone())
        g.eivec = d["eivec"].clone()
        datas.append(g.to(DEV))
    m = pygda_amd.models.SpecReg(L["in_dim"], L["h"], L["classes"], num_layers=2, ppmi=False, adv_dim=6, reg_mode=True,
                                 gamma_adv=L["gamma_adv"], thr_smooth=L["thr_smooth"], gamma_smooth=L["gamma_smooth"],
                                 thr_mfr=L["thr_mfr"], gamma_mfr=L["gamma_mfr"], lr=L["lr"], weight_decay=L["weight_decay"],
                                 device=DEV, epoch=L["epochs"], verbose=0)
    m.use_fused_critic = fused
    m.udagcn = m.init_model()
    _no_dropout(m.udagcn)
    m.udagcn.load_state_dict(state)
    h = L["h"]
    m.critic = torch.nn.Sequential(torch.nn.Linear(h, h), torch.nn.ReLU(), torch.nn.Linear(h, h), torch.nn.ReLU(),
                                   torch.nn.Linear(h, 1)).to(DEV)
    with torch.no_grad():
        for p, k in zip(ops.critic3_params(m.critic), H.PARAMS):
            p.copy_(crit[k])
    m.optimizer_critic = Adam(m.critic.parameters(), m.lr) if fused else torch.optim.Adam(m.critic.parameters(), m.lr)
    opt = torch.optim.Adam(m.udagcn.parameters(), lr=L["lr"], weight_decay=L["weight_decay"], foreach=False)
    losses = []
    for epoch in range(L["steps"]):
        loss, _, _ = m.forward_model(datas[0], datas[1], 0.05, epoch)
        opt.zero_grad()
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in m.udagcn.named_parameters() if v.grad is not None}
        opt.step()
        losses.append(loss.detach())
    return dict(losses=torch.stack(losses), critic={k: p.detach().clone() for k, p in zip(H.PARAMS, ops.critic3_params(m.critic))},
                grads=grads)


def test_switch_off_vs_on_three_steps():
    """Three ``forward_model`` + encoder steps at h = 64 from one seed: the losses, the critic's parameters and the
    encoder's last gradients of the FUSED path within the project's bound of the float64 loop on the CPU, the yardstick
    being the float32 torch loop's distance from it (tests/test_specreg_host.test_loop_conditions checks that the two
    loops took the same ReLU masks).  The switch-off path on the GPU is run and printed beside it, not asserted: it is
    the parent's code."""
    f64, f32 = H.loop_ref(torch.float64), H.loop_ref(torch.float32)
    on, off = _loop_on_device(True), _loop_on_device(False)
    for name, run in (("off", off), ("on", on)):
        print(f"switch {name}: losses {run['losses'].tolist()}  (float64 {f64['losses'].tolist()})")
    shared = [k for k in f64["grads"] if k in on["grads"]]
    assert len(shared) >= 4, sorted(on["grads"])
    for k in H.PARAMS:
        print(f"(off) critic {k}: |gpu - f64| = {(off['critic'][k].double().cpu() - f64['critic'][k]).abs().max():.3e}")
    close(on["losses"], f32["losses"], f64["losses"], "specreg_loop/losses")
    for k in H.PARAMS:
        assert on["critic"][k].shape == f64["critic"][k].shape
        close(on["critic"][k], f32["critic"][k], f64["critic"][k], f"specreg_loop/critic/{k}")
    for k in shared:
        assert on["grads"][k].shape == f64["grads"][k].shape, k
        close(on["grads"][k], f32["grads"][k], f64["grads"][k], f"specreg_loop/grad/{k}")


# ---- (7) outside the envelope: the torch composition, as before ------------------------------------------------------
def test_critic3_ok_on_the_device():
    good = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8), torch.nn.ReLU(),
                               torch.nn.Linear(8, 1)).to(DEV)
    assert ops.critic3_ok(torch.zeros(5, 8, device=DEV), good)
    for what in H.REFUSALS:
        es, critic = H.refusal(what, DEV)
        assert not ops.critic3_ok(es, critic if what != "cpu" else good), what


def _four_layers():
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8), torch.nn.ReLU(),
                               torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 1))


@pytest.mark.parametrize("which", ["h132", "fourth_layer"])
def test_fallback_trains_through_the_torch_path(which):
    """A critic outside the envelope: no gda_critic3 / hinge entry point is called, and the step is bit for bit the one
    the switch-off path takes."""
    runs = []
    for fused in (True, False):
        torch.manual_seed(11)
        crit = _four_layers() if which == "fourth_layer" else None
        m, s, t, epoch = _wide_model(132 if which == "h132" else 8, critic=crit)
        m.use_fused_critic = fused
        m.optimizer_critic = torch.optim.Adam(m.critic.parameters(), m.lr)
        calls = []
        orig = _lib.call
        try:
            _lib.call = lambda name, *a: calls.append(name) or orig(name, *a)
            loss, _, _ = m.forward_model(s, t, 0.05, epoch)
            loss.backward()
        finally:
            _lib.call = orig
        assert not [c for c in calls if "critic3" in c or "spectral_hinge" in c]
        runs.append((loss.detach(), [p.detach().clone() for p in m.critic.parameters()]))
    assert same_bits(runs[0][0], runs[1][0])
    assert all(same_bits(a, b) for a, b in zip(runs[0][1], runs[1][1]))
