"""GPU: the adversarial heads -- csrc/gda_critic.hip (AdaGCN's WGAN-GP critic update), csrc/gda_disc_mlp.hip (UDAGCN's
two-layer discriminator, AdaGCN's sigmoid-mean head, DANE's LSGAN head) and csrc/gda_disc.hip (the A2GNN / GRADE linear
discriminator) -- against the float64 restatements of tests/test_adv_heads_host.py on that file's cases, dropout on
included: the masks are the documented Philox stream (csrc/gda_dropout.h) at the sites the kernels document.

One bound for everything (tests/test_gpu_cwgcn._close): |gpu - f64| <= 8 |fp32 torch - f64| + 2e-6 max|f64|, the fp32
term being the same restatement in float32 on the CPU; the figures are printed per output.  Every device op runs twice
and has to return the same bits.

Largest |gpu - f64| / bound when the file was written: critic loss 0.03, gW1 0.14, gb1 0.21, gW2 0.21, gb2 0.80 (h = 96,
a = 40, p = 0: a scalar whose gap and penalty parts cancel to 8e-4; next 0.33), parameters after three Adam steps 0.09;
two-layer head 0.25 (head 0) and 0.08 (head 1); LSGAN head 0.11; linear discriminator 0.19."""
import numpy as np
import pytest
import torch

from pygda_amd import _lib, ops
from pygda_amd.ops import dropout_state
from tests import test_adv_heads_host as H
from tests.test_gpu_gat import close, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0


@pytest.fixture(autouse=True)
def _documented_seed(monkeypatch):
    """The masks the host file checked its conditions on: its seed for the length of a test."""
    monkeypatch.setattr(dropout_state, "seed", H.SEED)


def arm(step=H.STEP):
    dropout_state.counter(torch.device(DEV)).fill_(step)
    dropout_state.site = 0


def dev(t):
    return None if t is None else t.to(DEV)


def ratio(gpu, f32, f64):
    """|gpu - f64| over the project's bound."""
    a, b, c = (np.asarray(v.detach().double().cpu(), dtype=np.float64) for v in (gpu, f32, f64))
    return np.abs(a - c).max() / (8 * np.abs(b - c).max() + 2e-6 * max(np.abs(c).max(), 1e-30))


def compare(got, refs, keys, name):
    """Every output in ``keys`` of the device result ``got`` against the (float64, float32) restatements."""
    f64, f32 = refs
    for key in keys:
        if f64[key].numel() == 0:                       # the input gradient of a domain without rows
            assert got[key] is None or got[key].numel() == 0
            continue
        assert got[key].shape == f64[key].shape, f"{name}/{key}: shape"
        close(got[key], f32[key], f64[key], f"{name}/{key}")


def same(a, b, keys):
    return all((a[k] is None and b[k] is None) or same_bits(a[k], b[k]) for k in keys)


# ---- the critic update -----------------------------------------------------------------------------------------------
CRITIC_KEYS = ("loss", "gW1", "gb1", "gW2", "gb2")


def unaligned(t):
    """The same values in 4-byte-aligned storage: the matrix-core path asks for 16."""
    buf = torch.empty(t.numel() + 1, device=DEV)
    v = buf[1:].view_as(t)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def critic_device_inputs(name):
    x = {k: dev(v) for k, v in H.critic_inputs(name).items()}
    if H.CRITIC_CASES[name][6] == "unaligned":
        x["es"], x["et"] = unaligned(x["es"]), unaligned(x["et"])
    return x


def run_critic(x, p, step=H.STEP):
    arm(step)
    out = (torch.full((1,), SENTINEL, device=DEV),) + tuple(torch.full_like(x[k], SENTINEL) for k in ("W1", "b1", "W2", "b2"))
    ops.wgan_critic_grads(x["es"], x["et"], x["i_s"], x["i_t"], x["alpha"], x["W1"], x["b1"], x["W2"], x["b2"], p,
                          H.GP_WEIGHT, out)
    return dict(zip(CRITIC_KEYS, (out[0].reshape(()), *out[1:])))


@pytest.mark.parametrize("name,p", H.CRITIC_RUNS)
def test_critic_update_vs_float64(name, p):
    """ops.wgan_critic_grads on every instantiation of the row kernels (matrix cores at h = 64 | 96 | 128, their second
    trip of the grid, k_critic_rows<2> and <4>, 4-byte-aligned storage) against the reference's own formulation
    differentiated twice by autograd in float64, with and without dropout: loss and all four parameter gradients."""
    x = critic_device_inputs(name)
    got = run_critic(x, p)
    assert same(got, run_critic(x, p), CRITIC_KEYS)
    compare(got, H.critic_refs(name, p), CRITIC_KEYS, f"critic/{name}/p={p}")
    if p > 0:
        assert not same(got, run_critic(x, p, step=H.STEP + 1), ("gW1",))          # another step, other masks


@pytest.mark.parametrize("name", ["mfma_96x40", "rows2_100x33", "rows4_200x17"])
def test_critic_masks_sit_at_their_documented_sites(name):
    """The three mask sets are the sites site (source gap rows), site + 1 (target gap rows) and site + 2 (penalty rows):
    the restatement with any other assignment is outside the bound of what the kernel returns."""
    h, a, ns, nt = H.CRITIC_CASES[name][:4]
    x, p = H.critic_inputs(name), 0.3
    got = run_critic(critic_device_inputs(name), p)
    n_i = x["i_s"].numel()
    shapes = [(ns, a), (nt, a), (ns + nt + n_i, a)]
    for sites in ((1, 2, 2), (2, 1, 3), (1, 2, 4), (1, 1, 3)):
        masks = tuple(H.keep_masks(p, [shape], site=s)[0] for shape, s in zip(shapes, sites))
        f64, f32 = (H.critic_ref(**x, dtype=dt, p=p, masks=masks) for dt in (torch.float64, torch.float32))
        worst = max(ratio(got[k], f32[k], f64[k]) for k in CRITIC_KEYS)
        print(f"critic/{name}: sites {sites}: worst ratio {worst:.1f}")
        assert worst > 1.0, f"sites {sites} fit as well as the documented ones"


def test_critic_update_with_adam_inside_vs_float64_adam():
    """ops.wgan_critic_adam for three iterations (masks at consecutive sites of one step) against torch.optim.Adam in
    float64 on the float64 gradients of the restatement: the four parameters under the project's bound."""
    from pygda_amd.optim import Adam
    x = critic_device_inputs(H.ADAM_CASE)

    def run():
        params = [torch.nn.Parameter(x[k].clone()) for k in ("W1", "b1", "W2", "b2")]
        for q in params:
            q.grad = torch.zeros_like(q)
        opt = Adam(params, lr=H.ADAM_LR, weight_decay=H.ADAM_WD)
        loss = torch.zeros(1, device=DEV)
        arm()
        for _ in range(H.ADAM_ITERS):
            assert ops.wgan_critic_adam(x["es"], x["et"], x["i_s"], x["i_t"], x["alpha"], params, opt, H.ADAM_P, H.GP_WEIGHT, loss)
        return [q.detach() for q in params]

    got, again = run(), run()
    assert all(same_bits(u, v) for u, v in zip(got, again))
    (p64, _, _), (p32, _, _) = H.critic_adam_refs()
    for key, g, r32, r64 in zip(("W1", "b1", "W2", "b2"), got, p32, p64):
        assert not torch.equal(g, x[key])
        close(g, r32, r64, f"critic_adam/{H.ADAM_CASE}/{key}")


# ---- the two-layer head ----------------------------------------------------------------------------------------------
MLP_KEYS = ("ls", "lt", "ges", "get", "gW1", "gb1", "gW2", "gb2")


def run_mlp(case, p, step=H.STEP):
    head, h, a, ns, nt, pair, alpha_kind = case
    x = {k: dev(v).requires_grad_() for k, v in H.mlp_inputs(*case[:5]).items()}
    args = (x["es"], x["et"], x["W1"], x["b1"], x["W2"], x["b2"])
    arm(step)
    if head == 1:
        ls, lt = ops.critic_means(*args, p)
    else:
        alpha = H.MLP_ALPHA if alpha_kind == "float" else torch.tensor(H.MLP_ALPHA, device=DEV)
        out = ops.grl_mlp_ce(*args, alpha, p, pair=pair)
        ls, lt = out if pair else (out, None)
    g = H.mlp_alpha_and_g(case)[1]
    (ls * g[0] + (lt * g[1] if lt is not None else 0.0)).backward()
    got = dict(ls=ls.detach(), lt=None if lt is None else lt.detach())
    got.update({"g" + k: v.grad for k, v in x.items()})
    return got


@pytest.mark.parametrize("case", H.MLP_CASES)
@pytest.mark.parametrize("p", H.PS)
def test_mlp_head_vs_float64(case, p):
    """ops.grl_mlp_ce (head 0: sum and pair outputs, float and device-tensor alpha) and ops.critic_means (head 1) at every
    AK of the backward, both chunk counts of h, a domain boundary inside a 4-row group, an empty source, an empty
    target and a second trip of the grid: the domain means, both input gradients behind the reversal and the four
    parameter gradients, with and without dropout."""
    got = run_mlp(case, p)
    again = run_mlp(case, p)
    f64, f32 = refs = H.mlp_refs(case, p)
    keys = MLP_KEYS
    if got["lt"] is None:                                # the sum output: one scalar
        keys = MLP_KEYS[2:]
        assert same_bits(got["ls"], again["ls"])
        close(got["ls"], f32["ls"] + f32["lt"], f64["ls"] + f64["lt"], f"mlp_head/{case}/p={p}/sum")
    assert same(got, again, keys)
    compare(got, refs, keys, f"mlp_head/{case}/p={p}")
    if p > 0:
        assert not same(got, run_mlp(case, p, step=H.STEP + 1), ("gW1",))


@pytest.mark.parametrize("case", [c for c in H.MLP_CASES if c[1:5] == (128, 48, 257, 7)])
def test_mlp_head_masks_sit_at_their_documented_sites(case):
    """Source rows at site, target rows at site + 1, rows numbered inside their domain."""
    p = 0.3
    got = run_mlp(case, p)
    alpha, g = H.mlp_alpha_and_g(case)
    x = H.mlp_inputs(*case[:5])
    for sites in ((2, 1), (1, 1), (1, 3), (2, 3)):
        masks = tuple(H.keep_masks(p, [(rows, case[2])], site=s)[0] for rows, s in zip(case[3:5], sites))
        f64, f32 = (H.mlp_head_ref(case[0], **x, alpha=alpha, g=g, dtype=dt, p=p, masks=masks) for dt in (torch.float64, torch.float32))
        worst = max(ratio(got[k], f32[k], f64[k]) for k in MLP_KEYS[2:])
        print(f"mlp_head/{case}: sites {sites}: worst ratio {worst:.1f}")
        assert worst > 1.0, f"sites {sites} fit as well as the documented ones"


# ---- the LSGAN head --------------------------------------------------------------------------------------------------
LSGAN_KEYS = ("loss", "gx", "gW1", "gb1", "gW2", "gb2")


def run_lsgan(case):
    h, a, rows, target = case
    x = {k: dev(v).requires_grad_() for k, v in H.lsgan_inputs(h, a, rows).items()}
    loss = ops.lsgan_head(x["x"], x["W1"], x["b1"], x["W2"], x["b2"], target)
    (loss * H.LSGAN_G).backward()
    got = dict(loss=loss.detach())
    got.update({"g" + k: v.grad for k, v in x.items()})
    return got


@pytest.mark.parametrize("case", H.LSGAN_CASES)
def test_lsgan_head_vs_float64(case):
    """ops.lsgan_head with a on both sides of each of the four units a lane owns, one row, a ragged row count and more
    rows than one pass of the full grid, both targets: loss, input gradient and the four parameter gradients."""
    got = run_lsgan(case)
    assert same(got, run_lsgan(case), LSGAN_KEYS)
    compare(got, H.lsgan_refs(case), LSGAN_KEYS, f"lsgan/{case}")


# ---- the linear discriminator ----------------------------------------------------------------------------------------
DISC_KEYS = ("loss", "gfs", "gft", "gW", "gb")


def run_disc(case):
    x = H.disc_inputs(*case)
    t = {k: dev(x[k]).requires_grad_() for k in ("fs", "ft", "W", "b")}
    loss = ops.grl_disc_ce(t["fs"], t["ft"], t["W"], t["b"], H.DISC_ALPHA, labels=dev(x["labels"]))
    (loss * H.DISC_G).backward()
    got = dict(loss=loss.detach())
    got.update({"g" + k: v.grad for k, v in t.items()})
    return got


@pytest.mark.parametrize("case", H.DISC_CASES)
def test_grl_disc_ce_vs_float64(case):
    """ops.grl_disc_ce at every CPL (h up to 1,024) with C = 2, 3, 4 up to the backward's LDS limit, default and explicit
    labels, the fold's unroll edges, a second trip of the grid and an empty domain on either side."""
    got = run_disc(case)
    assert same(got, run_disc(case), DISC_KEYS)
    compare(got, H.disc_refs(case), DISC_KEYS, f"disc/{case}")


# ---- refusals --------------------------------------------------------------------------------------------------------
def untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in ts)


@pytest.mark.parametrize("h,a", [(6, 4), (260, 8), (64, 65)])
def test_critic_refuses_shapes_outside_its_kernels(h, a):
    """h not a multiple of 4, h > 256, a > 64: an error, nothing written."""
    x = {k: dev(v) for k, v in H.build_critic(h, a, 9, 5, 0, 0.5, 0.0).items()}
    out = (torch.full((1,), SENTINEL, device=DEV),) + tuple(torch.full_like(x[k], SENTINEL) for k in ("W1", "b1", "W2", "b2"))
    with pytest.raises(_lib.GdaError):
        ops.wgan_critic_grads(x["es"], x["et"], x["i_s"], x["i_t"], x["alpha"], x["W1"], x["b1"], x["W2"], x["b2"], 0.0,
                              H.GP_WEIGHT, out)
    assert untouched(*out)


@pytest.mark.parametrize("head", [0, 1])
@pytest.mark.parametrize("h,a", [(64, 65), (132, 16)])
def test_mlp_head_refuses_shapes_outside_its_kernels(head, h, a):
    x = {k: dev(v) for k, v in H.mlp_inputs(head, h, a, 9, 5).items()}
    args = (x["es"], x["et"], x["W1"], x["b1"], x["W2"], x["b2"])
    with pytest.raises(_lib.GdaError):
        ops.critic_means(*args, 0.0) if head else ops.grl_mlp_ce(*args, 0.5, 0.0)
    losses = torch.full((3,), SENTINEL, device=DEV)
    ws, _ = _lib.scratch("gda_grl_mlp_ce_workspace_bytes", torch.device(DEV), "disc_mlp", h, a)
    with pytest.raises(_lib.GdaError):
        _lib.call("gda_mlp_head_fwd_f32", head, x["es"], h, 9, x["et"], h, 5, h, a, x["W1"], x["b1"], x["W2"], x["b2"], 0.0,
                  H.SEED, dropout_state.counter(torch.device(DEV)), 1, losses, ws, ws.numel(), _lib.stream())
    assert untouched(losses)


def test_lsgan_head_refuses_more_than_256_units():
    a, rows = 257, 9
    x = {k: dev(v) for k, v in H.lsgan_inputs(16, a, rows).items()}
    with pytest.raises(_lib.GdaError):
        ops.lsgan_head(x["x"], x["W1"], x["b1"], x["W2"], x["b2"], 1.0)
    Z = torch.ones(rows, a, device=DEV)
    pre, loss, gZ = (torch.full(s, SENTINEL, device=DEV) for s in ((rows,), (1,), (rows, a)))
    gw2, gb2 = torch.full((a,), SENTINEL, device=DEV), torch.full((1,), SENTINEL, device=DEV)
    ws, _ = _lib.scratch("gda_lsgan_head_workspace_bytes", torch.device(DEV), "lsgan", a)
    w2, b2 = x["W2"].reshape(-1).contiguous(), x["b2"]
    with pytest.raises(_lib.GdaError):
        _lib.call("gda_lsgan_head_fwd_f32", Z, a, rows, a, w2, b2, 1.0, pre, loss, ws, ws.numel(), _lib.stream())
    with pytest.raises(_lib.GdaError):
        _lib.call("gda_lsgan_head_bwd_f32", Z, a, rows, a, w2, torch.zeros(rows, device=DEV), 1.0, torch.ones(1, device=DEV),
                  gZ, a, gw2, gb2, ws, ws.numel(), _lib.stream())
    assert untouched(pre, loss, gZ, gw2, gb2)


@pytest.mark.parametrize("h,C", [(1024, 4), (800, 4)])
def test_grl_disc_ce_refuses_in_the_forward_what_its_backward_cannot_run(h, C):
    """C h (1 + 4) floats of LDS in k_bwd: past 60 KB the FORWARD call is refused (it used to compute a loss whose
    backward() then failed), with nothing launched."""
    x = H.disc_inputs(h, C, 9, 5, False)
    t = {k: dev(x[k]).requires_grad_() for k in ("fs", "ft", "W", "b")}
    with pytest.raises(_lib.GdaError):
        ops.grl_disc_ce(t["fs"], t["ft"], t["W"], t["b"], 0.5)
    probs, loss = torch.full((14, C), SENTINEL, device=DEV), torch.full((1,), SENTINEL, device=DEV)
    ws, _ = _lib.scratch("gda_grl_disc_workspace_bytes", torch.device(DEV), "disc", 14, h, C)
    with pytest.raises(_lib.GdaError):
        _lib.call("gda_grl_disc_ce_fwd_f32", t["fs"].detach(), h, 9, t["ft"].detach(), h, 5, h, C, t["W"].detach(), t["b"].detach(),
                  None, probs, loss, ws, ws.numel(), _lib.stream())
    assert untouched(probs, loss)
