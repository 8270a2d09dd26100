"""The adversarial heads without a GPU: the yardsticks, inputs and case lists of tests/test_gpu_adv_heads.py.

Four restatements, each runnable in float64 and float32 and with explicit dropout masks -- ``critic_ref`` (AdaGCN's
WGAN-GP critic update, the double backward through ``torch.autograd.grad(create_graph=True)``, NOT the closed form of
csrc/gda_critic.hip), ``mlp_head_ref`` (UDAGCN's two-layer discriminator and AdaGCN's sigmoid-mean head behind a gradient
reversal), ``lsgan_ref`` (DANE's head) and ``disc_ce_ref`` (the A2GNN / GRADE linear discriminator) -- cross-checked at
1e-12 in float64 against the project's composed CPU path, and the inputs both files share with the conditions those
inputs have to meet.

Exact inputs.  The gradients of these heads jump where a pre-activation crosses 0, so encodings are multiples of 1/8 in
[0, 4], interpolation weights multiples of 1/8 in [0, 1], W1 multiples of 1/16 in [-1/2, 1/2] and b1 odd multiples of
1/2048: every pre-activation is an odd multiple of 1/2048 below 2^20 / 2048 in magnitude (h <= 256), exact in float32 in
any summation order, so the ReLU mask is the same in every precision and never decided by a rounding."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_gpu_parity import _philox_keep

SEED, STEP, SITE = 0x5EED, 7, 1         # generator state of every masked case: the first call after ``site = 0`` draws site 1
GP_WEIGHT = 5.0
PS = (0.0, 0.3)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def exact_rows(gen, rows, h, sparse=False):
    """[rows, h] float32 multiples of 1/8 in [0, 4]; ``sparse``: about half the entries 0 (another distribution)."""
    x = torch.randint(0, 33, (rows, h), generator=gen)
    if sparse:
        x = x * torch.randint(0, 2, (rows, h), generator=gen)
    return x.float() / 8


def exact_layer(gen, a, h):
    """W1 [a, h] multiples of 1/16 in [-1/2, 1/2], b1 [a] odd multiples of 1/2048."""
    W1 = torch.randint(-8, 9, (a, h), generator=gen).float() / 16
    while not bool((W1.sum(1) > 0).any()):                 # a 1 x 1 layer included: some unit fires on positive rows
        W1 = torch.randint(-8, 9, (a, h), generator=gen).float() / 16
    b1 = (2 * torch.randint(-32, 32, (a,), generator=gen) + 1).float() / 2048
    return W1, b1


def interp_indices(ns, nt):
    """AdaGCN._interp_indices: the smaller domain twice against the head and the tail of the larger one."""
    from pygda_amd.models import AdaGCN
    i_s, i_t = AdaGCN._interp_indices(type("_NoCache", (), {})(), ns, nt, torch.device("cpu"))
    return i_s, i_t


def keep_masks(p, shapes, site=SITE, step=STEP, seed=SEED):
    """The keep-bits of consecutive call sites ``site, site + 1, ...`` for [rows, a] hidden layers (csrc/gda_dropout.h:
    element index row_in_domain * a + unit), or None at p = 0."""
    if p <= 0:
        return None
    return tuple(_philox_keep(seed, step, site + k, rows * a, p).reshape(rows, a) for k, (rows, a) in enumerate(shapes))


def _scale(p, dtype):
    """1 / (1 - p) for the float p the kernels receive."""
    return 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32).to(dtype))


class _Reverse(torch.autograd.Function):
    """pygda/nn/reverse_layer.py: identity forward, ``-alpha * g`` backward (alpha a number or a 0-dim tensor)."""

    @staticmethod
    def forward(ctx, x, alpha):
        ctx.alpha = alpha
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.neg() * ctx.alpha, None


def _leaves(dtype, *ts):
    return [t.detach().to(dtype).clone().requires_grad_(True) for t in ts]


def _hidden(x, W1, b1, keep, p):
    pre = F.linear(x, W1, b1)
    hid = torch.relu(pre)
    if keep is not None:
        hid = hid * (keep.to(x.dtype) * _scale(p, x.dtype))
    return hid, pre


# ---- the yardsticks --------------------------------------------------------------------------------------------------
def critic_ref(es, et, i_s, i_t, alpha, W1, b1, W2, b2, gp_weight=GP_WEIGHT, dtype=torch.float64, p=0.0, masks=None):
    """One critic update of AdaGCN in the reference's own formulation: ``D = Linear - ReLU - mask - Linear(a, 1) -
    Sigmoid``, ``loss = -|mean D(e_s) - mean D(e_t)| + gp_weight * mean((|dD/dx|_2 - 1)^2)`` over ``cat(e_s, e_t,
    e_t[it] + alpha (e_s[is] - e_t[it]))``.  ``masks``: keep-bits of (source gap rows, target gap rows, penalty rows).
    Returns the loss, the four parameter gradients, the gap, the penalty rows' gradient norms and every pre-activation."""
    es, et, alpha = es.to(dtype), et.to(dtype), alpha.to(dtype)
    W1, b1, W2, b2 = _leaves(dtype, W1, b1, W2, b2)
    ks, kt, kp = masks if masks is not None else (None, None, None)

    def D(x, keep):
        hid, pre = _hidden(x, W1, b1, keep, p)
        return torch.sigmoid(F.linear(hid, W2, b2)), pre

    ds, pre_s = D(es, ks)
    dt, pre_t = D(et, kt)
    gap = ds.mean() - dt.mean()
    hs, ht = es[i_s.long()], et[i_t.long()]
    x = torch.cat([es, et, ht + alpha * (hs - ht)]).requires_grad_(True)
    scores, pre_p = D(x, kp)
    grad = torch.autograd.grad(outputs=scores, inputs=x, grad_outputs=torch.ones_like(scores), create_graph=True)[0]
    norm = grad.norm(2, dim=1)
    loss = -gap.abs() + gp_weight * ((norm - 1) ** 2).mean()
    gW1, gb1, gW2, gb2 = torch.autograd.grad(loss, [W1, b1, W2, b2])
    return dict(loss=loss.detach(), gW1=gW1, gb1=gb1, gW2=gW2, gb2=gb2, gap=gap.detach(), norm=norm.detach(),
                pre=torch.cat([pre_s, pre_t, pre_p]).detach())


def mlp_head_ref(head, es, et, W1, b1, W2, b2, alpha, g, dtype=torch.float64, p=0.0, masks=None):
    """``D = Linear(h, a) - ReLU - mask - Linear(a, 2 - head)`` behind a gradient reversal: head 0 the two per-domain
    cross-entropy means (source rows against class 0, target rows against class 1), head 1 the two means of
    ``sigmoid(D)``; a domain without rows contributes 0.  Gradients of ``g[0] * l_s + g[1] * l_t``."""
    es, et, W1, b1, W2, b2 = _leaves(dtype, es, et, W1, b1, W2, b2)
    al = alpha.to(dtype) if torch.is_tensor(alpha) else alpha
    keeps = masks if masks is not None else (None, None)
    terms, pres = [], []
    for dom, (x, keep) in enumerate(zip((es, et), keeps)):
        hid, pre = _hidden(_Reverse.apply(x, al), W1, b1, keep, p)
        z = F.linear(hid, W2, b2)
        pres.append(pre.detach())
        if x.size(0) == 0:
            terms.append(z.sum() * 0)
        elif head == 0:
            terms.append(F.cross_entropy(z, torch.full((x.size(0),), dom, dtype=torch.long)))
        else:
            terms.append(torch.sigmoid(z).mean())
    (terms[0] * g[0] + terms[1] * g[1]).backward()
    return dict(ls=terms[0].detach(), lt=terms[1].detach(), ges=es.grad, get=et.grad, gW1=W1.grad, gb1=b1.grad,
                gW2=W2.grad, gb2=b2.grad, pre=torch.cat(pres))


def lsgan_ref(x, W1, b1, W2, b2, target, g, dtype=torch.float64):
    """``mean((Linear(a, 1)(relu(Linear(h, a)(x))) - target)^2)`` and the gradients of ``g`` times it."""
    x, W1, b1, W2, b2 = _leaves(dtype, x, W1, b1, W2, b2)
    hid, pre = _hidden(x, W1, b1, None, 0.0)
    loss = ((F.linear(hid, W2, b2) - target) ** 2).mean()
    (loss * g).backward()
    return dict(loss=loss.detach(), gx=x.grad, gW1=W1.grad, gb1=b1.grad, gW2=W2.grad, gb2=b2.grad, pre=pre.detach())


def disc_ce_ref(fs, ft, W, b, alpha, labels, g, dtype=torch.float64):
    """``cross_entropy(Linear(h, C)(reverse(cat(source, target))), labels)``, labels 0 | 1 by domain unless given."""
    fs, ft, W, b = _leaves(dtype, fs, ft, W, b)
    if labels is None:
        labels = torch.cat([torch.zeros(fs.size(0), dtype=torch.long), torch.ones(ft.size(0), dtype=torch.long)])
    loss = F.cross_entropy(F.linear(_Reverse.apply(torch.cat([fs, ft]), alpha), W, b), labels)
    (loss * g).backward()
    return dict(loss=loss.detach(), gfs=fs.grad, gft=ft.grad, gW=W.grad, gb=b.grad)


# ---- critic cases ----------------------------------------------------------------------------------------------------
# name -> (h, a, ns, nt, dropout rates, (seed, w2 scale, b2), kind).  Kinds: "mfma" the matrix-core path, "rows2" / "rows4"
# k_critic_rows<2> / <4>, "unaligned" the matrix-core shape from 4-byte-aligned storage (k_critic_rows<2>).  Seed, scale
# and b2 are chosen so that the conditions below hold (test_critic_cases_meet_their_conditions); w2 ~ scale * N(0, 1).
CRITIC_CASES = {
    "mfma_64x4_1+1": (64, 4, 1, 1, PS, (8, 0.15, 0.5), "mfma"),
    "mfma_64x64": (64, 64, 130, 97, PS, (6, 0.4, 9.625), "mfma"),
    "mfma_96x40": (96, 40, 65, 200, PS, (10, 0.4, -8.1875), "mfma"),
    "mfma_128x40": (128, 40, 300, 420, PS, (7, 0.4, 11.125), "mfma"),
    "mfma_128x64_equal": (128, 64, 256, 256, PS, (1, 0.4, -5.1875), "mfma"),
    "mfma_64x4_second_trip": (64, 4, 22000, 22000, PS, (6, 3.0, 6.6875), "mfma"),
    "mfma_64x4_dropped_rows": (64, 4, 300, 420, (0.9,), (7, 0.15, -1.375), "mfma"),
    "rows2_4x1": (4, 1, 9, 5, PS, (1, 0.15, 0.0), "rows2"),
    "rows2_100x33": (100, 33, 257, 33, PS, (1, 0.4, -2.0), "rows2"),
    "rows2_64x62": (64, 62, 97, 130, PS, (7, 0.4, 5.1875), "rows2"),
    "rows2_128x40_unaligned": (128, 40, 300, 420, PS, (4, 0.4, -8.375), "unaligned"),
    "rows4_132x24": (132, 24, 100, 100, PS, (7, 0.6, 8.1875), "rows4"),
    "rows4_200x17": (200, 17, 33, 257, PS, (1, 0.6, 1.6875), "rows4"),
    "rows4_256x64": (256, 64, 70, 90, PS, (2, 0.25, 4.1875), "rows4"),
}
DEGENERATE = ("mfma_64x4_1+1", "rows2_4x1")          # three and twenty-three penalty rows: no statistics asked of them
DROPPED = "mfma_64x4_dropped_rows"
CRITIC_RUNS = [(name, p) for name, c in CRITIC_CASES.items() for p in c[4]]
ADAM_CASE, ADAM_P, ADAM_LR, ADAM_WD, ADAM_ITERS = "mfma_128x64_equal", 0.3, 0.01, 0.01, 3


def build_critic(h, a, ns, nt, seed, w2_scale, b2):
    gen = _gen(1000 * h + a + 7919 * seed)
    es, et = exact_rows(gen, ns, h), exact_rows(gen, nt, h, sparse=True)
    W1, b1 = exact_layer(gen, a, h)
    W2 = torch.randn(1, a, generator=gen) * w2_scale
    i_s, i_t = interp_indices(ns, nt)
    alpha = torch.randint(0, 9, (i_s.numel(), 1), generator=gen).float() / 8
    return dict(es=es, et=et, i_s=i_s, i_t=i_t, alpha=alpha, W1=W1, b1=b1, W2=W2, b2=torch.tensor([float(b2)]))


@functools.lru_cache(maxsize=None)
def critic_inputs(name):
    h, a, ns, nt, _, tune, _ = CRITIC_CASES[name]
    return build_critic(h, a, ns, nt, *tune)


def critic_masks(name, p, site=SITE, step=STEP):
    h, a, ns, nt, _, _, _ = CRITIC_CASES[name]
    n_i = critic_inputs(name)["i_s"].numel()
    return keep_masks(p, [(ns, a), (nt, a), (ns + nt + n_i, a)], site=site, step=step)


@functools.lru_cache(maxsize=None)
def critic_refs(name, p):
    """``(float64, float32)`` restatements of a case at its documented masks: computed once, shared by both files."""
    x, masks = critic_inputs(name), critic_masks(name, p)
    return tuple(critic_ref(**x, dtype=dt, p=p, masks=masks) for dt in (torch.float64, torch.float32))


def assert_exact_pre(f64, f32, what):
    """Pre-activations bit-equal in float32 and float64 and at least 2^-11 away from the ReLU's kink."""
    assert torch.equal(f32["pre"].double(), f64["pre"]), f"{what}: float32 pre-activations are not exact"
    if f64["pre"].numel():
        assert float(f64["pre"].abs().min()) >= 2.0 ** -11, f"{what}: a pre-activation on the kink"


# ---- two-layer head cases --------------------------------------------------------------------------------------------
def _mlp_cases():
    """(head, h, a, ns, nt, pair, alpha kind): a on both sides of every AK of the backward (16 | 32 | 48 | 64), each AK with
    both heads and with one and two 64-column chunks of h; ns in {5, 257} so that the domain boundary falls inside a
    4-row group; sum and pair outputs, float and device-tensor alpha (head 0; head 1 has two outputs and no reversal)."""
    out, k = [], 0
    for a_lo, a_hi in ((1, 16), (17, 32), (33, 48), (49, 64)):
        for a, hs in ((a_lo, (1, 65)), (a_hi, (64, 128))):
            for h in hs:
                for head in (0, 1):
                    ns, nt = ((5, 130), (257, 7))[(k // 2) % 2]
                    out.append((head, h, a, ns, nt, bool((k // 4) % 2) or head == 1, ("float", "tensor")[(k // 8) % 2]))
                    k += 1
    for head in (0, 1):
        out += [(head, 65, 33, 0, 37, head == 1, "float"), (head, 64, 17, 41, 0, True, "tensor"),
                (head, 128, 64, 5000, 3300, head == 1, "float")]         # past the 8,192 rows of one trip of the grid
    return out


MLP_CASES = _mlp_cases()
MLP_G = (1.5, 0.5)                       # upstream weights of a pair output; a sum output is weighted by MLP_G[0]
MLP_ALPHA = 0.375


@functools.lru_cache(maxsize=None)
def mlp_inputs(head, h, a, ns, nt):
    gen = _gen(100003 * head + 1009 * h + 31 * a + ns + 3 * nt)
    es, et = exact_rows(gen, ns, h), exact_rows(gen, nt, h, sparse=True)
    W1, b1 = exact_layer(gen, a, h)
    nz = 2 - head
    W2 = torch.randn(nz, a, generator=gen) * (2.0 / (a * h) ** 0.5)      # logits of order 1
    b2 = torch.randn(nz, generator=gen) * 0.25
    return dict(es=es, et=et, W1=W1, b1=b1, W2=W2, b2=b2)


def mlp_masks(case, p, site=SITE, step=STEP):
    _, _, a, ns, nt, _, _ = case
    return keep_masks(p, [(ns, a), (nt, a)], site=site, step=step)


def mlp_alpha_and_g(case):
    """``(alpha of the reference, upstream weights)``: head 1 has no reversal (the ops pass alpha = -1)."""
    head, pair = case[0], case[5]
    return (-1.0 if head == 1 else MLP_ALPHA), (MLP_G if pair else (MLP_G[0], MLP_G[0]))


@functools.lru_cache(maxsize=None)
def mlp_refs(case, p):
    alpha, g = mlp_alpha_and_g(case)
    x, masks = mlp_inputs(*case[:5]), mlp_masks(case, p)
    return tuple(mlp_head_ref(case[0], **x, alpha=alpha, g=g, dtype=dt, p=p, masks=masks)
                 for dt in (torch.float64, torch.float32))


# ---- LSGAN head cases ------------------------------------------------------------------------------------------------
# (h, a, rows, target): a on both sides of every unit a lane owns (LS_UC = 4 units of 64 lanes); the last case has more
# rows than the 256 workgroups x 4 wavefronts of k_lsgan_fwd / _bwd take in one pass at their full grid (rows > 8,160)
LSGAN_CASES = [(16, 1, 1, 0.0), (100, 64, 193, 1.0), (256, 65, 193, 0.0), (16, 128, 1, 1.0), (100, 129, 193, 0.0),
               (256, 192, 193, 1.0), (16, 193, 193, 1.0), (100, 256, 193, 0.0), (256, 256, 1, 1.0), (16, 65, 9001, 0.0)]
LSGAN_G = 0.75


@functools.lru_cache(maxsize=None)
def lsgan_inputs(h, a, rows):
    gen = _gen(4001 * h + 17 * a + rows)
    x = exact_rows(gen, rows, h)
    W1, b1 = exact_layer(gen, a, h)
    return dict(x=x, W1=W1, b1=b1, W2=torch.randn(1, a, generator=gen) * (2.0 / (a * h) ** 0.5),
                b2=torch.randn(1, generator=gen) * 0.25)


@functools.lru_cache(maxsize=None)
def lsgan_refs(case):
    h, a, rows, target = case
    return tuple(lsgan_ref(**lsgan_inputs(h, a, rows), target=target, g=LSGAN_G, dtype=dt)
                 for dt in (torch.float64, torch.float32))


# ---- linear discriminator cases --------------------------------------------------------------------------------------
def _disc_cases():
    """(h, C, ns, nt, explicit labels): h on both sides of every CPL (1 | 2 | 4 | 8 | 16 columns per lane), every C with
    C h (1 + 4) 4 bytes within the backward's 60 KB of LDS, (768, 4) exactly at it; 16 b rows for b in {1, 28, 29, 33}
    workgroups (the edges of the fold's eight-deep unroll), one count above the 8,192 rows of a full grid's trip, an
    empty source and an empty target."""
    shapes = [(h, C) for h in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024) for C in (2, 3, 4) if C * h <= 3072]
    shapes.append((768, 4))
    rows = [16 * b for b in (1, 28, 29, 33)]
    out = []
    for k, (h, C) in enumerate(shapes):
        n = rows[k % 4]
        ns = n // 3 + 1
        out.append((h, C, ns, n - ns, k % 2 == 1))
    out += [(65, 3, 5000, 3301, True), (129, 2, 6000, 2500, False), (64, 2, 0, 37, False), (257, 4, 41, 0, True)]
    return out


DISC_CASES = _disc_cases()
DISC_ALPHA, DISC_G = 0.625, 1.75


@functools.lru_cache(maxsize=None)
def disc_inputs(h, C, ns, nt, explicit):
    gen = _gen(7001 * h + 13 * C + ns + 5 * nt)
    fs, ft = torch.randn(ns, h, generator=gen), torch.randn(nt, h, generator=gen) * 1.2 + 0.25
    W, b = torch.randn(C, h, generator=gen) * (1.0 / h ** 0.5), torch.randn(C, generator=gen) * 0.25
    labels = torch.randint(0, C, (ns + nt,), generator=gen) if explicit else None
    return dict(fs=fs, ft=ft, W=W, b=b, labels=labels)


@functools.lru_cache(maxsize=None)
def disc_refs(case):
    return tuple(disc_ce_ref(**disc_inputs(*case), alpha=DISC_ALPHA, g=DISC_G, dtype=dt)
                 for dt in (torch.float64, torch.float32))


# ---- Adam on the critic's gradients ----------------------------------------------------------------------------------
def critic_adam_ref(name, p, iters, lr, wd, dtype):
    """``iters`` critic updates with torch.optim.Adam on the restatement's gradients in ``dtype``: iteration k draws its
    masks at the sites 1 + 3 k .. 3 + 3 k of one step, as consecutive calls of the op do.  Returns the parameters and the
    smallest |pre-activation| met on the way."""
    x = dict(critic_inputs(name))
    params = [nn.Parameter(x[k].to(dtype).clone()) for k in ("W1", "b1", "W2", "b2")]
    opt = torch.optim.Adam(params, lr=lr, weight_decay=wd)
    margin, signs = float("inf"), []
    for k in range(iters):
        r = critic_ref(x["es"], x["et"], x["i_s"], x["i_t"], x["alpha"], *[q.detach() for q in params], dtype=dtype, p=p,
                       masks=critic_masks(name, p, site=SITE + 3 * k))
        for q, key in zip(params, ("gW1", "gb1", "gW2", "gb2")):
            q.grad = r[key].clone()
        opt.step()
        margin = min(margin, float(r["pre"].abs().min()))
        signs.append(r["pre"] > 0)
    return [q.detach().clone() for q in params], margin, signs


@functools.lru_cache(maxsize=None)
def critic_adam_refs():
    return tuple(critic_adam_ref(ADAM_CASE, ADAM_P, ADAM_ITERS, ADAM_LR, ADAM_WD, dt) for dt in (torch.float64, torch.float32))


# ---- tests: the restatements against the project's composed CPU path -------------------------------------------------
def _rel(a, b):
    assert a.shape == b.shape
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name", ["mfma_128x40", "rows2_100x33", "mfma_128x64_equal"])      # the three size rules
def test_critic_ref_is_the_composed_critic_update(name, monkeypatch):
    """critic_ref in float64, dropout off, against AdaGCN.gradient_penalty + _critic_gap on the CPU with the same
    interpolation weights: loss and all four parameter gradients at 1e-12."""
    import pygda_amd.hipgraph as hipgraph
    from pygda_amd.models import AdaGCN
    h, a, ns, nt = CRITIC_CASES[name][:4]
    x = critic_inputs(name)
    m = AdaGCN(16, h, 3, num_layers=2, adv_dim=a, gp_weight=GP_WEIGHT, domain_weight=1, device="cpu", epoch=1, verbose=0)
    d = m.discriminator = nn.Sequential(nn.Linear(h, a), nn.ReLU(), nn.Dropout(0.0), nn.Linear(a, 1), nn.Sigmoid()).double()
    with torch.no_grad():
        for q, key in zip(d.parameters(), ("W1", "b1", "W2", "b2")):
            q.copy_(x[key].double())
    monkeypatch.setattr(hipgraph, "host_rand_provider", lambda shape: x["alpha"].double().reshape(shape))
    es, et = x["es"].double(), x["et"].double()
    loss = -torch.abs(m._critic_gap(es, et)) + m.gp_weight * m.gradient_penalty(es, et)
    loss.backward()
    ref = critic_ref(**x)
    assert _rel(ref["loss"], loss.detach()) <= 1e-12
    for q, key in zip(d.parameters(), ("gW1", "gb1", "gW2", "gb2")):
        assert _rel(ref[key], q.grad) <= 1e-12, key


@pytest.mark.parametrize("head", [0, 1])
def test_mlp_head_ref_is_the_composed_discriminator(head):
    """mlp_head_ref in float64, dropout off, against torch.nn.Sequential + CrossEntropyLoss (head 0; the project's
    GradReverse in front) and Sequential(..., Sigmoid) means (head 1) at 1e-12."""
    from pygda_amd.nn import GradReverse
    case = next(c for c in MLP_CASES if c[0] == head and c[1] == 128 and c[3] > 0 and c[4] > 0)
    _, h, a, ns, nt, _, _ = case
    x = mlp_inputs(*case[:5])
    layers = [nn.Linear(h, a), nn.ReLU(), nn.Dropout(0.0), nn.Linear(a, 2 - head)] + ([nn.Sigmoid()] if head else [])
    d = nn.Sequential(*layers).double()
    with torch.no_grad():
        for q, key in zip(d.parameters(), ("W1", "b1", "W2", "b2")):
            q.copy_(x[key].double())
    es, et = x["es"].double().requires_grad_(), x["et"].double().requires_grad_()
    if head == 0:
        ce = nn.CrossEntropyLoss()
        ls = ce(d(GradReverse.apply(es, MLP_ALPHA)), torch.zeros(ns, dtype=torch.long))
        lt = ce(d(GradReverse.apply(et, MLP_ALPHA)), torch.ones(nt, dtype=torch.long))
    else:
        ls, lt = d(es).mean(), d(et).mean()
    (ls * MLP_G[0] + lt * MLP_G[1]).backward()
    ref = mlp_head_ref(head, **x, alpha=MLP_ALPHA if head == 0 else -1.0, g=MLP_G)
    assert _rel(ref["ls"], ls.detach()) <= 1e-12 and _rel(ref["lt"], lt.detach()) <= 1e-12
    for got, want in zip((ref["ges"], ref["get"], ref["gW1"], ref["gb1"], ref["gW2"], ref["gb2"]),
                         (es.grad, et.grad, *(q.grad for q in d.parameters()))):
        assert _rel(got, want) <= 1e-12


def test_lsgan_ref_is_the_composed_head():
    h, a, rows, target = LSGAN_CASES[5]
    x = lsgan_inputs(h, a, rows)
    d = nn.Sequential(nn.Linear(h, a), nn.ReLU(), nn.Linear(a, 1)).double()
    with torch.no_grad():
        for q, key in zip(d.parameters(), ("W1", "b1", "W2", "b2")):
            q.copy_(x[key].double())
    xin = x["x"].double().requires_grad_()
    loss = ((d(xin) - target) ** 2).mean()
    (loss * LSGAN_G).backward()
    ref = lsgan_ref(**x, target=target, g=LSGAN_G)
    assert _rel(ref["loss"], loss.detach()) <= 1e-12
    for got, want in zip((ref["gx"], ref["gW1"], ref["gb1"], ref["gW2"], ref["gb2"]), (xin.grad, *(q.grad for q in d.parameters()))):
        assert _rel(got, want) <= 1e-12


@pytest.mark.parametrize("case", [c for c in DISC_CASES if c[:2] in ((129, 3), (64, 2))][:3])
def test_disc_ce_ref_is_the_composed_discriminator(case):
    from pygda_amd.nn import GradReverse
    x = disc_inputs(*case)
    lin = nn.Linear(case[0], case[1]).double()
    with torch.no_grad():
        lin.weight.copy_(x["W"].double()); lin.bias.copy_(x["b"].double())
    fs, ft = x["fs"].double().requires_grad_(), x["ft"].double().requires_grad_()
    lab = x["labels"] if x["labels"] is not None else torch.cat([torch.zeros(case[2], dtype=torch.long), torch.ones(case[3], dtype=torch.long)])
    loss = nn.CrossEntropyLoss()(lin(GradReverse.apply(torch.cat([fs, ft]), DISC_ALPHA)), lab)
    (loss * DISC_G).backward()
    ref = disc_ce_ref(**x, alpha=DISC_ALPHA, g=DISC_G)
    assert _rel(ref["loss"], loss.detach()) <= 1e-12
    for got, want in zip((ref["gfs"], ref["gft"], ref["gW"], ref["gb"]), (fs.grad, ft.grad, lin.weight.grad, lin.bias.grad)):
        assert _rel(got, want) <= 1e-12


# ---- tests: the conditions on the inputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,p", CRITIC_RUNS)
def test_critic_cases_meet_their_conditions(name, p):
    """Exact pre-activations; a gap away from 0; gradient norms on both sides of 1 (at least 5 % of the penalty rows
    each) in every case that has rows enough; in the dropped-rows case at least 20 % of the penalty rows with a
    gradient norm of exactly 0 (every unit dropped or inactive; the norm's derivative there is 0, as torch's is) and at
    least 20 % with another."""
    f64, f32 = critic_refs(name, p)
    assert_exact_pre(f64, f32, name)
    assert abs(float(f64["gap"])) > 1e-4
    for key in ("loss", "gW1", "gb1", "gW2", "gb2"):
        assert bool(torch.isfinite(f64[key]).all())
    norm = f64["norm"]
    above, below, zero = (float(v.double().mean()) for v in (norm > 1, norm < 1, norm == 0))
    print(f"{name} p={p}: gap {float(f64['gap']):+.4f}, norm > 1: {above:.3f}, < 1: {below:.3f}, == 0: {zero:.3f}")
    if name == DROPPED:
        assert zero >= 0.2 and 1 - zero >= 0.2
    elif name not in DEGENERATE:
        assert above >= 0.05 and below >= 0.05


def test_critic_cases_have_gaps_of_both_signs():
    signs = {float(torch.sign(critic_refs(name, p)[0]["gap"])) for name, p in CRITIC_RUNS if CRITIC_CASES[name][2] < 1000}
    assert signs == {-1.0, 1.0}


def test_critic_cases_reach_the_kernels_they_name():
    """The dispatch of gda_wgan_critic_f32 restated: matrix cores for h in {64, 96, 128} with a % 4 == 0, else
    k_critic_rows<2> up to h = 128 and <4> above; the second-trip case has more penalty rows than 512 workgroups x 4
    wavefronts x 32 rows, and all three size rules of the interpolates occur."""
    rules = set()
    for name, (h, a, ns, nt, _, _, kind) in CRITIC_CASES.items():
        mfma = h in (64, 96, 128) and a % 4 == 0
        assert h % 4 == 0 and h <= 256 and a <= 64
        assert kind == ("mfma" if mfma else "rows2" if h <= 128 else "rows4") or (kind == "unaligned" and mfma)
        rules.add((ns > nt) - (ns < nt))
    assert rules == {-1, 0, 1}
    h, a, ns, nt = CRITIC_CASES["mfma_64x4_second_trip"][:4]
    assert ns + nt + critic_inputs("mfma_64x4_second_trip")["i_s"].numel() == 66000 > 512 * 4 * 32


def test_critic_adam_trajectory_keeps_its_relu_pattern():
    """Three Adam steps leave the exact grid of W1.  A float32 pre-activation of this case (a sum of 128 products of
    magnitude up to 2, |pre| of order 10) is off by about 10 * 2^-24 * sqrt(128) = 7e-6: the float64 trajectory keeps every
    pre-activation at least 4e-5 away from 0 and the float32 trajectory has the same ReLU pattern, so the comparison on
    the GPU is not a lottery."""
    (p64, margin, s64), (p32, _, s32) = critic_adam_refs()
    print(f"smallest |pre| on the float64 trajectory: {margin:.3e}")
    assert margin >= 4e-5
    assert all(torch.equal(u, v) for u, v in zip(s64, s32))
    assert all(float((u - v.double()).abs().max()) < 1e-4 for u, v in zip(p64, p32))


@pytest.mark.parametrize("case", MLP_CASES)
@pytest.mark.parametrize("p", PS)
def test_mlp_head_cases_are_exact_and_alive(case, p):
    f64, f32 = mlp_refs(case, p)
    assert_exact_pre(f64, f32, str(case))
    for key in ("gW1", "gb1", "gW2", "gb2"):
        assert bool(torch.isfinite(f64[key]).all())
    assert float(f64["gW2"].abs().max()) > 1e-4          # not saturated: the head's gradients are there to be compared


def test_mlp_head_cases_cover_the_dispatch():
    """Every AK of k_mlp_ce_bwd with both heads and with one and two chunks of h; both outputs and alpha kinds; both
    empty domains; a boundary inside a 4-row group; more than 8,192 rows."""
    ak = lambda a: 16 * ((a + 15) // 16)
    assert {(ak(c[2]), c[0], c[1] > 64) for c in MLP_CASES} == {(k, hd, w) for k in (16, 32, 48, 64) for hd in (0, 1) for w in (False, True)}
    assert {c[2] for c in MLP_CASES} >= {1, 16, 17, 32, 33, 48, 49, 64} and {c[1] for c in MLP_CASES} >= {1, 64, 65, 128}
    for head in (0, 1):
        mine = [c for c in MLP_CASES if c[0] == head]
        assert any(c[3] == 0 for c in mine) and any(c[4] == 0 for c in mine) and any(c[3] + c[4] > 8192 for c in mine)
        assert {c[3] for c in mine} >= {5, 257}                          # neither a multiple of the 4 rows of a group
    assert {(c[5], c[6]) for c in MLP_CASES if c[0] == 0} == {(pr, al) for pr in (False, True) for al in ("float", "tensor")}


@pytest.mark.parametrize("case", LSGAN_CASES)
def test_lsgan_cases_are_exact(case):
    f64, f32 = lsgan_refs(case)
    assert_exact_pre(f64, f32, str(case))
    assert float(f64["gW2"].abs().max()) > 1e-6


def test_lsgan_and_disc_cases_cover_the_dispatch():
    assert {c[1] for c in LSGAN_CASES} == {1, 64, 65, 128, 129, 192, 193, 256} and {c[0] for c in LSGAN_CASES} == {16, 100, 256}
    assert {c[2] for c in LSGAN_CASES} >= {1, 193} and {c[3] for c in LSGAN_CASES} == {0.0, 1.0}
    assert any(c[2] > 256 * 4 * 8 for c in LSGAN_CASES)                  # ls_blocks: the full grid, then a second pass
    cpl = lambda h: next(c for c in (1, 2, 4, 8, 16) if (h + 63) // 64 <= c)
    assert {(cpl(c[0]), c[1]) for c in DISC_CASES} >= {(k, C) for k in (1, 2, 4, 8) for C in (2, 3, 4)} | {(16, 2), (16, 3)}
    assert all(c[0] * c[1] * 5 * 4 <= 60 * 1024 for c in DISC_CASES) and (768, 4) in {c[:2] for c in DISC_CASES}
    assert {c[2] + c[3] for c in DISC_CASES} >= {16, 448, 464, 528} and any(c[2] + c[3] > 8192 for c in DISC_CASES)
    assert any(c[2] == 0 for c in DISC_CASES) and any(c[3] == 0 for c in DISC_CASES)
    assert {c[4] for c in DISC_CASES if c[1] == 2} == {False, True}
    for case in DISC_CASES:
        assert all(bool(torch.isfinite(v).all()) for v in disc_refs(case)[0].values())
