"""SpecReg's critic and spectral hinges without a GPU: the yardsticks, inputs and case lists of tests/test_gpu_specreg.py.

``critic3_ref`` is the reference's own formulation of one critic update (pygda/models/specreg.py:194-200,380-419): the
``Sequential`` forward, ``torch.autograd.grad(create_graph=True)`` and a second backward, in the dtype asked for;
``hinge_ref`` the same for the regulariser (:209-215) and ``gap_ref`` for the encoder-side term (:202).
``critic3_closed`` restates the update in the closed form csrc/gda_critic3.hip implements and is held to 1e-12 of
``critic3_ref`` in float64 on every case: that pins the algebra here, where it can run.

Conditions on the inputs (asserted below for the committed seeds).  The critic is piecewise linear: a ReLU unit that is
on in one precision and off in the other makes another function, not a rounding.  So the float32 and float64
restatements must agree on every ReLU mask, and no row's input-gradient norm may be below 1e-6 except the row built to
have none.  Likewise no hinge argument (|X[i] - X[i+1]| - thr, |X| - thr, the differences, X itself) may change sign
between float32 and float64, with a margin of twice the float32 projection's own error for another summation order.
Weights are ``randn / sqrt(h)``, biases ``0.1 randn``, encodings ``randn``."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pygda_amd import ops

KEYS = ("loss", "gW1", "gb1", "gW2", "gb2", "gW3", "gb3")
PARAMS = ("W1", "b1", "W2", "b2", "W3", "b3")

# name -> (h, n_s, n_t, seed): the smallest shapes at which the row kernel can go wrong
CASES = {
    "golden_width_ragged_tile": (8, 20, 17, 1),           # the goldens' width, one ragged tile
    "full_tile_plus_row": (64, 33, 31, 2),                # one full tile plus one row
    "one_row_target": (96, 70, 1, 3),                     # a one-row domain
    "one_row_source_h100": (100, 1, 45, 4),               # h not a multiple of 32
    "several_tiles": (128, 257, 130, 5),                  # several tiles per workgroup, both domains ragged
    # more rows than one trip of the row kernel's capped grid (the second trip's first workgroup gets a ragged quad)
    "second_trip": (8, 20000, ops.CRITIC3_ROWS_PER_TRIP + 100 - 20000, 17),
    "zero_gradient_row": (12, 37, 29, 7),                 # b1 = 0 and source row 5 = -W1^-1 1: a1 = -1, g = 0 exactly
}
ZERO_ROW = 5
assert sum(CASES["second_trip"][1:3]) < 70000


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32 inputs of a case: es, et and the six parameters (W3 [1, h], b3 [1] as ``nn.Linear`` holds them)."""
    h, ns, nt, seed = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    x = dict(es=torch.randn(ns, h, generator=gen), et=torch.randn(nt, h, generator=gen))
    for k, shape in (("W1", (h, h)), ("W2", (h, h)), ("W3", (1, h))):
        x[k] = torch.randn(*shape, generator=gen) / h ** 0.5
    for k, n in (("b1", h), ("b2", h), ("b3", 1)):
        x[k] = 0.1 * torch.randn(n, generator=gen)
    if name == "zero_gradient_row":
        x["b1"] = torch.zeros(h)
        x["es"][ZERO_ROW] = -torch.linalg.solve(x["W1"].double(), torch.ones(h, dtype=torch.float64)).float()
    return x


def _leaves(dtype, x):
    return [x[k].detach().to(dtype).clone().requires_grad_(True) for k in PARAMS]


def _critic(W1, b1, W2, b2, W3, b3):
    return lambda v: F.linear(torch.relu(F.linear(torch.relu(F.linear(v, W1, b1)), W2, b2)), W3, b3)


# ---- the yardsticks --------------------------------------------------------------------------------------------------
def critic3_ref(es, et, W1, b1, W2, b2, W3, b3, dtype=torch.float64):
    """One critic update in the reference's own formulation; the parameters must be leaves of ``dtype``."""
    es, et = es.to(dtype), et.to(dtype)
    D = _critic(W1, b1, W2, b2, W3, b3)
    loss_1 = D(es).mean() - D(et).mean()
    x = torch.cat([es, et]).requires_grad_(True)
    out = D(x)
    grad = torch.autograd.grad(outputs=out, inputs=x, grad_outputs=torch.ones_like(out), create_graph=True,
                               retain_graph=True, only_inputs=True)[0]
    norm = grad.view(grad.shape[0], -1).norm(2, dim=1)
    loss = -loss_1 + 10 * torch.mean((norm - 1) ** 2)
    grads = torch.autograd.grad(loss, [W1, b1, W2, b2, W3, b3], allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, (W1, b1, W2, b2, W3, b3))]
    return dict(zip(KEYS, (loss.detach(), *grads)), norm=norm.detach())


def critic3_closed(es, et, W1, b1, W2, b2, W3, b3, dtype=torch.float64):
    """The closed form of csrc/gda_critic3.hip, row by row as matrices; also the masks and the norms."""
    es, et = es.to(dtype), et.to(dtype)
    W1, b1, W2, b2, W3, b3 = (p.detach().to(dtype) for p in (W1, b1, W2, b2, W3, b3))
    ns, nt = es.size(0), et.size(0)
    M, w3 = ns + nt, W3.reshape(-1)
    x = torch.cat([es, et])
    a1 = x @ W1.t() + b1
    r1 = (a1 > 0).to(dtype)
    h1 = r1 * a1
    a2 = h1 @ W2.t() + b2
    r2 = (a2 > 0).to(dtype)
    h2 = r2 * a2
    D = h2 @ w3 + b3
    p = r2 * w3
    q = r1 * (p @ W2)
    g = q @ W1
    n = g.norm(2, dim=1)
    ghat = torch.where(n[:, None] > 0, g / n[:, None].clamp_min(torch.finfo(dtype).tiny), torch.zeros_like(g))
    c = (10 * 2 * (n - 1) / M)[:, None]
    sigma = torch.cat([torch.full((ns,), -1.0 / ns, dtype=dtype), torch.full((nt,), 1.0 / nt, dtype=dtype)])[:, None]
    t = r1 * (ghat @ W1.t())
    s = r2 * (t @ W2.t())
    loss = -(D[:ns].mean() - D[ns:].mean()) + 10 * ((n - 1) ** 2).mean()
    out = dict(loss=loss, gW1=q.t() @ (sigma * x + c * ghat), gb1=(sigma * q).sum(0), gW2=p.t() @ (sigma * h1 + c * t),
               gb2=(sigma * p).sum(0), gW3=(sigma * h2 + c * s).sum(0)[None, :], gb3=sigma.sum().reshape(1))
    return dict(out, norm=n, r1=r1.bool(), r2=r2.bool(), g=g)


@functools.lru_cache(maxsize=None)
def critic3_refs(name):
    """``(float64, float32)`` results of ``critic3_ref`` on a case: computed once, shared, never modified."""
    x = inputs(name)
    return tuple(critic3_ref(x["es"], x["et"], *_leaves(dt, x), dtype=dt) for dt in (torch.float64, torch.float32))


ADAM_LR, ADAM_STEPS = 0.01, 3


@functools.lru_cache(maxsize=None)
def adam_refs(name):
    """``ADAM_STEPS`` iterations of the critic loop with ``torch.optim.Adam`` on ``critic3_ref``'s gradients:
    ``(float64, float32)`` dicts of the final parameters, and whether every ReLU mask agreed on the way."""
    x = inputs(name)
    runs, masks = [], []
    for dt in (torch.float64, torch.float32):
        leaves = _leaves(dt, x)
        opt = torch.optim.Adam(leaves, ADAM_LR)
        seen = []
        for _ in range(ADAM_STEPS):
            c = critic3_closed(x["es"], x["et"], *leaves, dtype=dt)
            seen.append((c["r1"], c["r2"]))
            res = critic3_ref(x["es"], x["et"], *leaves, dtype=dt)
            for p, k in zip(leaves, KEYS[1:]):
                p.grad = res[k].clone()
            opt.step()
        runs.append({k: p.detach().clone() for k, p in zip(PARAMS, leaves)})
        masks.append(seen)
    same = all(torch.equal(a1, b1) and torch.equal(a2, b2) for (a1, a2), (b1, b2) in zip(*masks))
    return runs[0], runs[1], same


def gap_ref(es, et, W1, b1, W2, b2, W3, b3, gout, dtype=torch.float64):
    """``mean D(es) - mean D(et)`` and its input gradients for the incoming gradient ``gout``."""
    es, et = (v.detach().to(dtype).clone().requires_grad_(True) for v in (es, et))
    D = _critic(*(p.detach().to(dtype) for p in (W1, b1, W2, b2, W3, b3)))
    value = D(es).mean() - D(et).mean()
    ges, get = torch.autograd.grad(value * gout, [es, et])
    return dict(value=value.detach(), ges=ges, get=get)


# ---- the spectral hinges ---------------------------------------------------------------------------------------------
GAMMA_SMOOTH, GAMMA_MFR = 0.5, 0.25
# name -> (k, N, h, thr_smooth, thr_mfr, seed)
HINGE_CASES = {
    "k100_h8_both": (100, 150, 8, 0.7, 0.9, 11),
    "k1000_h128_both": (1000, 1030, 128, 0.7, 0.9, 13),
    "smooth_only": (100, 150, 8, 0.7, -1.0, 21),
    "mfr_only": (100, 150, 8, -1.0, 0.9, 14),
    "single_difference_row": (2, 40, 16, 0.3, 0.4, 15),
    "both_off": (100, 150, 8, -1.0, 0.0, 16),
}


@functools.lru_cache(maxsize=None)
def hinge_inputs(name):
    k, N, h, _, _, seed = HINGE_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(k, N, generator=gen) / N ** 0.5, torch.randn(N, h, generator=gen)


def hinge_ref(eivec, encoded, thr_smooth, gamma_smooth, thr_mfr, gamma_mfr, dtype=torch.float64):
    """The regulariser of one domain as the reference writes it; value, the encodings' gradient and the projection."""
    eivec = eivec.to(dtype)
    enc = encoded.detach().to(dtype).clone().requires_grad_(True)
    X = eivec @ enc
    value = torch.zeros((), dtype=dtype)
    if thr_smooth > 0:
        value = value + F.relu((X[:-1] - X[1:]).abs() - thr_smooth).mean() * gamma_smooth
    if thr_mfr > 0:
        value = value + F.relu(X.abs() - thr_mfr).mean() * gamma_mfr
    grad = torch.autograd.grad(value, enc)[0] if value.requires_grad else None
    return dict(value=value.detach(), grad=grad, X=X.detach())


@functools.lru_cache(maxsize=None)
def hinge_refs(name):
    _, _, _, ts, tm, _ = HINGE_CASES[name]
    e, x = hinge_inputs(name)
    return tuple(hinge_ref(e, x, ts, GAMMA_SMOOTH, tm, GAMMA_MFR, dt) for dt in (torch.float64, torch.float32))


# ---- tests -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_closed_form_is_the_double_backward(name):
    """The algebra the kernel implements against autograd's double backward, float64, 1e-12 relative."""
    x = inputs(name)
    ref = critic3_refs(name)[0]
    got = critic3_closed(x["es"], x["et"], *(x[k] for k in PARAMS))
    for k in KEYS + ("norm",):
        # gb3 = sum sigma is -1 + 1: relative to the two sums it cancels, not to its own (zero) value
        err, top = (got[k] - ref[k]).abs().max().item(), max(ref[k].abs().max().item(), 1.0 if k == "gb3" else 1e-300)
        assert err <= 1e-12 * top, f"{name}/{k}: {err:.3e} against {top:.3e}"
    assert all(torch.isfinite(ref[k]).all() for k in KEYS)


@pytest.mark.parametrize("name", list(CASES))
def test_case_conditions(name):
    """Same ReLU masks in float32 and float64; no vanishing input gradient except the constructed row."""
    x = inputs(name)
    c64, c32 = (critic3_closed(x["es"], x["et"], *(x[k] for k in PARAMS), dtype=dt) for dt in (torch.float64, torch.float32))
    assert torch.equal(c64["r1"], c32["r1"]) and torch.equal(c64["r2"], c32["r2"])
    small = (c64["norm"] < 1e-6).nonzero().flatten().tolist()
    if name == "zero_gradient_row":
        assert small == [ZERO_ROW] and c64["norm"][ZERO_ROW] == 0 and c32["norm"][ZERO_ROW] == 0
        assert not c32["r1"][ZERO_ROW].any() and bool((c32["g"][ZERO_ROW] == 0).all())
    else:
        assert small == []
    assert adam_refs(name)[2] if name != "second_trip" else True


@pytest.mark.parametrize("name", [n for n in HINGE_CASES if n != "both_off"])
def test_hinge_case_conditions(name):
    """No hinge argument changes sign between float32 and float64, nor within twice the float32 projection's error."""
    _, _, _, ts, tm, _ = HINGE_CASES[name]
    r64, r32 = hinge_refs(name)
    X64, X32 = r64["X"], r32["X"].double()
    margin = 2 * (X64 - X32).abs().max().item()
    for X in (X64, X32):
        d = X[:-1] - X[1:]
        args = [X, d] + ([d.abs() - ts] if ts > 0 else []) + ([X.abs() - tm] if tm > 0 else [])
        assert all(a.abs().min().item() > margin for a in args), name
    d64, d32 = X64[:-1] - X64[1:], X32[:-1] - X32[1:]
    assert torch.equal(X64 > 0, X32 > 0) and torch.equal(d64 > 0, d32 > 0)
    if ts > 0:
        assert torch.equal(d64.abs() > ts, d32.abs() > ts) and bool((d64.abs() > ts).any()) and not bool((d64.abs() > ts).all())
    if tm > 0:
        assert torch.equal(X64.abs() > tm, X32.abs() > tm) and bool((X64.abs() > tm).any()) and not bool((X64.abs() > tm).all())


def _seq(h, bias=True, extra=False, out=1):
    layers = [nn.Linear(h, h, bias=bias), nn.ReLU(), nn.Linear(h, h), nn.ReLU(), nn.Linear(h, out)]
    if extra:
        layers += [nn.ReLU(), nn.Linear(out, 1)]
    return nn.Sequential(*layers)


REFUSALS = ("h6", "h132", "no_bias", "fourth_layer", "float64", "cpu")


def refusal(what, device="cpu"):
    """``(es, critic)`` of a refused input; ``device`` is where everything but the "cpu" case's encodings lives."""
    h = {"h6": 6, "h132": 132}.get(what, 8)
    critic = _seq(h, bias=what != "no_bias", extra=what == "fourth_layer").to(device)
    es = torch.zeros(5, h, dtype=torch.float64 if what == "float64" else torch.float32,
                     device="cpu" if what == "cpu" else device)
    return es, critic


REASONS = dict(h6="width", h132="width", no_bias="bias", fourth_layer="module", float64="input", cpu="device")


@pytest.mark.parametrize("what", REFUSALS)
def test_critic3_ok_refuses(what):
    """A refused input takes the torch path, and it is refused for the property the case names: the predicate asks for
    the device last, so on this host -- where every tensor is a CPU tensor -- each case stops at its own question."""
    assert not ops.critic3_ok(*refusal(what))
    assert ops.critic3_refusal(*refusal(what)) == REASONS[what]
    assert ops.critic3_refusal(torch.zeros(5, 8), _seq(8)) == "device"          # nothing else to object to


def test_rows_per_trip_is_the_library_s():
    """The second-trip case is sized by the ops constant: it has to be the row kernel's."""
    from pygda_amd import _lib
    assert _lib.lib().gda_critic3_rows_per_trip() == ops.CRITIC3_ROWS_PER_TRIP
    assert sum(CASES["second_trip"][1:3]) > ops.CRITIC3_ROWS_PER_TRIP


# ---- the trainer's loop: three forward_model + encoder steps ---------------------------------------------------------
LOOP = dict(h=64, in_dim=12, classes=3, ns=90, nt=70, k=20, steps=3, lr=0.01, weight_decay=0.003, gamma_adv=0.1,
            thr_smooth=0.05, gamma_smooth=0.5, thr_mfr=0.1, gamma_mfr=0.5, epochs=3, seed=101,
            edges_per_node=0.25, xscale=6.0)     # sparse graphs, wide features: encodings that differ from row to row


@functools.lru_cache(maxsize=None)
def loop_data():
    """Two random graphs with their ``eivec``, the encoder's initial state (the oracle's, float32) and the critic's
    initial parameters (drawn as the cases' are)."""
    from oracle import pygda_cpu as O
    from pygda_amd.data import to_undirected
    L = LOOP
    gen = torch.Generator().manual_seed(L["seed"])

    def domain(n):
        ei = to_undirected(torch.randint(0, n, (2, int(L["edges_per_node"] * n)), generator=gen), n)
        return dict(x=L["xscale"] * torch.randn(n, L["in_dim"], generator=gen), ei=ei,
                    y=torch.randint(0, L["classes"], (n,), generator=gen), eivec=torch.randn(L["k"], n, generator=gen) / n ** 0.5)

    src, tgt = domain(L["ns"]), domain(L["nt"])
    torch.manual_seed(L["seed"])
    net = O.UDAGCNBase(L["in_dim"], L["h"], L["classes"], num_layers=2, ppmi=False, adv_dim=6, dropout_p=0.0)
    h = L["h"]
    crit = {}
    for k, shape in (("W1", (h, h)), ("W2", (h, h)), ("W3", (1, h))):
        crit[k] = torch.randn(*shape, generator=gen) / h ** 0.5
    for k, n in (("b1", h), ("b2", h), ("b3", 1)):
        crit[k] = 0.1 * torch.randn(n, generator=gen)
    return src, tgt, {k: v.detach().clone() for k, v in net.state_dict().items()}, crit


@functools.lru_cache(maxsize=None)
def loop_ref(dtype):
    """The loop in the reference's own formulation on the CPU in ``dtype`` (oracle encoder, ``critic3_ref`` updates with
    ``torch.optim.Adam``, the gap, the hinges, the entropy term, one encoder Adam step per ``forward_model``).  Returns
    the losses, the critic's final parameters, the encoder's gradients of the last step, and every ReLU mask the critic
    took on the way (updates and gap) with the smallest input-gradient norm."""
    from oracle import pygda_cpu as O
    L = LOOP
    src, tgt, state, crit = loop_data()
    net = O.UDAGCNBase(L["in_dim"], L["h"], L["classes"], num_layers=2, ppmi=False, adv_dim=6, dropout_p=0.0)
    net.load_state_dict(state)
    net = net.to(dtype)
    graphs = []
    for name, d in (("source", src), ("target", tgt)):
        graphs.append(O.Graph(d["x"].to(dtype), d["ei"], d["y"]))
        for conv in net.encoder.conv_layers:        # the normalisation in ``dtype`` too (the oracle's default is float32)
            conv.cache_dict[name] = O.gcn_norm(d["ei"], torch.ones(d["ei"].size(1), dtype=dtype), d["x"].size(0), False, True, "row")
    leaves = [crit[k].to(dtype).clone().requires_grad_(True) for k in PARAMS]
    c_opt = torch.optim.Adam(leaves, L["lr"])
    opt = torch.optim.Adam(net.parameters(), lr=L["lr"], weight_decay=L["weight_decay"])
    losses, masks, nmin = [], [], float("inf")
    for epoch in range(L["steps"]):
        es, et = net.encode(graphs[0], "source"), net.encode(graphs[1], "target")
        s_logits = net.cls_model(es)
        loss = net.loss_func(s_logits, src["y"])
        xs, xt = es.detach(), et.detach()
        for _ in range(5):
            c = critic3_closed(xs, xt, *leaves, dtype=dtype)
            masks.append((c["r1"], c["r2"]))
            nmin = min(nmin, float(c["norm"].min()))
            res = critic3_ref(xs, xt, *leaves, dtype=dtype)
            for p, k in zip(leaves, KEYS[1:]):
                p.grad = res[k].clone()
            c_opt.step()
        c = critic3_closed(xs, xt, *leaves, dtype=dtype)
        masks.append((c["r1"], c["r2"]))
        D = _critic(*(p.detach() for p in leaves))
        loss = loss + (D(es).mean() - D(et).mean()) * L["gamma_adv"]
        for d, e in ((src, es), (tgt, et)):
            X = d["eivec"].to(dtype) @ e
            loss = loss + F.relu((X[:-1] - X[1:]).abs() - L["thr_smooth"]).mean() * L["gamma_smooth"] \
                        + F.relu(X.abs() - L["thr_mfr"]).mean() * L["gamma_mfr"]
        p = torch.clamp(F.softmax(net.cls_model(et), dim=-1), min=1e-9, max=1.0)
        loss = loss + torch.mean(torch.sum(-p * torch.log(p), dim=-1)) * (epoch / L["epochs"] * 0.01)
        opt.zero_grad()
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in net.named_parameters() if v.grad is not None}
        opt.step()
        losses.append(loss.detach().clone())
    return dict(losses=torch.stack(losses), critic={k: p.detach().clone() for k, p in zip(PARAMS, leaves)}, grads=grads,
                masks=masks, nmin=nmin)


def test_loop_conditions():
    """Over the three steps the float32 and float64 loops take the same ReLU masks in every critic update and in the gap,
    and no input gradient vanishes.  (Second-layer units that are on for every row are common here -- GCN encodings of
    one graph resemble each other -- and their bias gradient is w3 * sum(sigma) = 0 exactly: the kernel forms it from
    the on-counts and gets 0, the float32 torch loop a residue that Adam amplifies; that residue is part of the
    yardstick's own distance from float64.)"""
    r64, r32 = loop_ref(torch.float64), loop_ref(torch.float32)
    assert len(r64["masks"]) == LOOP["steps"] * 6
    for (a1, a2), (b1, b2) in zip(r64["masks"], r32["masks"]):
        assert torch.equal(a1, b1) and torch.equal(a2, b2)
    assert min(r64["nmin"], r32["nmin"]) > 1e-6
    assert bool(torch.isfinite(r64["losses"]).all())
