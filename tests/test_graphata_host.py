"""GraphATA without a GPU: the host compositions of ``ops.sparsemax`` / ``ata_gate`` / ``ata_mix`` / ``ata_head_loss`` /
``ata_vote`` / ``ata_memory_update`` against float64 brute-force restatements of the reference's expressions written
here (the yardsticks of tests/test_gpu_graphata.py, with the inputs and shape lists both files share), the sparsemax
known answers and the fits recorded from the reference's own graphata.py (tests/golden/make_golden_graphata.py), the
two identities the device layer rests on against a literal restatement of ``NodeCentricConv.forward``, the state-dict
names, the refusals, the signature, and the argument checks of gda_graphata.hip's C ABI."""
import ctypes
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pygda_amd import _lib, ops
from pygda_amd.data import Data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ("graphata_fit_a.npz", "graphata_fit_b.npz", "graphata_fit_c.npz")     # c: live dropout
MIX_SHAPES = [(1, 4, 1), (67, 5, 2), (67, 20, 3), (130, 128, 2), (65, 256, 8)]                      # (N, h, S)
HEAD_SHAPES = [(1, 2, 1), (67, 3, 2), (300, 5, 3), (130, 64, 8), (1030, 7, 2)]                      # (N, C, S)
VOTE_SHAPES = [(1, 2, 2, 2), (67, 53, 3, 6), (300, 260, 5, 11), (130, 130, 64, 16)]                 # (N, Nm, C, K1)
MEMORY_SHAPES = [(1, 2, 4), (67, 3, 20), (1030, 5, 128)]                                            # (N, C, d)
GAP = 1e-5          # tests/test_kbl_host.py's constant: the float64 gap asked of a discrete choice


# ---- the float64 yardsticks: the reference's expressions, spelled out ------------------------------------------------------
class RefSparsemax(torch.autograd.Function):
    """node_centric_conv.py:42-71, :102-107 and :128-136 over dim 1."""

    @staticmethod
    def forward(ctx, a):
        z = a - a.max(dim=1, keepdim=True).values
        srt, _ = torch.sort(z, descending=True, dim=1)
        cumsum = srt.cumsum(1) - 1
        rhos = torch.arange(1, a.size(1) + 1, dtype=a.dtype).view(1, -1)
        support = rhos * srt > cumsum
        supp = support.sum(dim=1).unsqueeze(1)
        tau = cumsum.gather(1, supp - 1)
        tau = tau / supp.to(a.dtype)
        out = torch.clamp(z - tau, min=0)
        ctx.save_for_backward(supp, out)
        ctx.gap = (z - tau).abs().min(dim=1).values
        return out

    @staticmethod
    def backward(ctx, grad_output):
        supp, out = ctx.saved_tensors
        grad_input = grad_output.clone()
        grad_input[out == 0] = 0
        v_hat = grad_input.sum(dim=1) / supp.to(out.dtype).squeeze(1)
        return torch.where(out != 0, grad_input - v_hat.unsqueeze(1), grad_input)


def sparsemax_gap(a):
    """Per row of ``a`` the smallest ``|z_s - tau|``: how far the support is from changing."""
    z = a - a.max(dim=1, keepdim=True).values
    srt, _ = torch.sort(z, descending=True, dim=1)
    cumsum = srt.cumsum(1) - 1
    supp = (torch.arange(1, a.size(1) + 1, dtype=a.dtype).view(1, -1) * srt > cumsum).sum(dim=1, keepdim=True)
    return (z - cumsum.gather(1, supp - 1) / supp.to(a.dtype)).abs().min(dim=1).values


def brute_gate(nr, dg):
    x = nr.detach().clone().requires_grad_(True)
    g = torch.sigmoid(x) * x
    g.backward(dg)
    return g.detach(), x.grad


def brute_mix(P, Q, a, lamb, gy):
    """``(y, w, dP, dQ, da)`` of NodeCentricConv's last lines on the ``S`` projections ``P [N, S h]``."""
    P, Q, a = (v.detach().clone().requires_grad_(True) for v in (P, Q, a))
    n, h = Q.shape
    w = RefSparsemax.apply(a)
    gamma = torch.stack([P[:, s * h:(s + 1) * h] for s in range(a.size(1))])
    y = torch.sum(w.t().unsqueeze(-1) * gamma, dim=0) + Q * lamb
    y.backward(gy)
    return y.detach(), w.detach(), P.grad, Q.grad, a.grad


def brute_head(Z, att, pred):
    """``(out [4], logits, dZ, datt)``: NodeCentricMLP's blend and graphata.py:423-437."""
    Z, att = Z.detach().clone().requires_grad_(True), att.detach().clone().requires_grad_(True)
    weights = torch.cat([torch.matmul(Z[s], att.view(-1, 1)) for s in range(Z.size(0))], dim=1)
    w = RefSparsemax.apply(weights)
    logits = torch.sum(w.t().unsqueeze(-1) * Z, dim=0)
    if pred is None:
        return None, logits.detach(), None, None
    softmax_out = F.softmax(logits, dim=1)
    ent = torch.mean(torch.sum(-softmax_out * torch.log(softmax_out + 1e-8), dim=1))
    mean_softmax = softmax_out.mean(dim=0)
    div = torch.sum(mean_softmax * torch.log(mean_softmax + 1e-5))
    ce = F.cross_entropy(logits, pred)
    loss = ent + div + ce
    loss.backward()
    return torch.stack([loss, ent, div, ce]).detach(), logits.detach(), Z.grad, att.grad


def brute_vote(nn_idx, mem_cls):
    """``(pred, gap)``: graphata.py:433-435 with the FIRST arg-max, and the top-2 gap of the voted means."""
    pred_near = torch.mean(mem_cls[nn_idx[:, 1:]], dim=1)
    top = torch.sort(pred_near, dim=1, descending=True).values
    first = torch.tensor([int(torch.nonzero(r == r.max())[0]) for r in pred_near])
    return first, top[:, 0] - top[:, 1]


def brute_memory(logits, feat, mem_cls, mem_fea, momentum):
    softmax_out = F.softmax(logits, dim=1)
    outputs_target = softmax_out ** 2 / ((softmax_out ** 2).sum(dim=0))
    return (1.0 - momentum) * mem_cls + momentum * outputs_target, (1.0 - momentum) * mem_fea + momentum * feat


# ---- the inputs both test files use ----------------------------------------------------------------------------------------
def _f32_exact(x):
    return x.float().double()


def _decided_scores(g, n, s, scale=1.0):
    """``[n, s]`` scores whose sparsemax support is decided in float64 by ``GAP``: a row that is not is redrawn."""
    a = _f32_exact(torch.randn(n, s, generator=g, dtype=torch.float64) * scale)
    for _ in range(100):
        bad = sparsemax_gap(a) < GAP
        if s == 1 or not bool(bad.any()):
            break
        a[bad] = _f32_exact(torch.randn(int(bad.sum()), s, generator=g, dtype=torch.float64) * scale)
    return a


def mix_inputs(n, h, s):
    """``(P, Q, a, gy)`` in float64 on float32 values.  Planted where there is room: row 0 exactly equal scores (weights
    exactly ``1 / S``), row 1 a top score that leads by more than 1 (a support of one), row 2 a zero ``gy``."""
    g = torch.Generator().manual_seed(10000 * n + 10 * h + s)
    P, Q, gy = (_f32_exact(torch.randn(n, w, generator=g, dtype=torch.float64)) for w in (s * h, h, h))
    a = _decided_scores(g, n, s)
    if n >= 3 and s >= 2:
        a[0] = 0.375
        a[1] = torch.linspace(-2.0, -1.25, s, dtype=torch.float64)
        a[1, s // 2] = 0.5
        gy[2] = 0
    return P, Q, a, gy


def head_inputs(n, c, s):
    """``(Z [S, N, C], att [C], pred [N])``.  The scores ``<Z_si, att>`` are decided by ``GAP``; the last class is
    predicted by no row (``C >= 3``); row 1 has logits spread over 60 in every source, so some ``p`` vanishes
    under the ``+ 1e-8`` of the entropy."""
    g = torch.Generator().manual_seed(20000 * n + 10 * c + s)
    att = _f32_exact(torch.randn(c, generator=g, dtype=torch.float64))
    Z = _f32_exact(torch.randn(s, n, c, generator=g, dtype=torch.float64))
    if n >= 2:
        Z[:, 1, :] = _f32_exact(torch.linspace(-35.0, 35.0, c, dtype=torch.float64))
    for _ in range(100):
        bad = sparsemax_gap(torch.einsum("snc,c->ns", Z, att)) < GAP
        if s == 1 or not bool(bad.any()):
            break
        Z[:, bad] = _f32_exact(torch.randn(s, int(bad.sum()), c, generator=g, dtype=torch.float64))
    pred = torch.randint(0, c - 1 if c >= 3 else c, (n,), generator=g)
    return Z, att, pred


def vote_inputs(n, nm, c, k1, variant=""):
    """``(nn_idx [N, K1], mem_cls [Nm, C])``: random neighbour rows and a memory of softmax rows whose votes are decided
    by ``GAP`` (an undecided row's neighbours are redrawn).  ``variant='uniform'``: the memory holds exactly ``1 / C``;
    ``variant='tie'``: the rows that row 0 votes with all hold ``[0, 0.5, 0.5, 0, ..]`` (``[0.5, 0.5]`` for two classes),
    an exact two-class tie that goes to the lower class."""
    g = torch.Generator().manual_seed(30000 * n + 100 * nm + 10 * c + k1)
    mem_cls = _f32_exact(torch.softmax(torch.randn(nm, c, generator=g, dtype=torch.float64), dim=1))
    nn_idx = torch.randint(0, nm, (n, k1), generator=g)
    for _ in range(100):
        bad = brute_vote(nn_idx, mem_cls)[1] < GAP
        if not bool(bad.any()):
            break
        nn_idx[bad] = torch.randint(0, nm, (int(bad.sum()), k1), generator=g)
    if variant == "uniform":
        mem_cls = torch.ones(nm, c, dtype=torch.float64) / c
    if variant == "tie":
        row = torch.zeros(c, dtype=torch.float64)
        row[-2:] = 0.5
        if c >= 3:
            row = torch.zeros(c, dtype=torch.float64)
            row[1:3] = 0.5
        mem_cls[nn_idx[0, 1:]] = row
    return nn_idx, mem_cls


def memory_inputs(n, c, d):
    g = torch.Generator().manual_seed(40000 * n + 100 * c + d)
    logits = _f32_exact(torch.randn(n, c, generator=g, dtype=torch.float64) * 2)
    feat, mem_fea = (_f32_exact(torch.randn(n, d, generator=g, dtype=torch.float64)) for _ in range(2))
    mem_cls = _f32_exact(torch.softmax(torch.randn(n, c, generator=g, dtype=torch.float64), dim=1))
    return logits, feat, mem_cls, mem_fea


def close(ours, f32, f64, name, slack=2e-6):
    """The project's bound (tests/test_gpu_cwgcn._close), each figure printed before it is asserted."""
    ours, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                      for v in (ours, f32, f64))
    e_ours, e_ref = np.abs(ours - f64).max(), np.abs(f32 - f64).max()
    lim = 8 * e_ref + slack * max(np.abs(f64).max(), 1e-30)
    print(f"{name}: |ours - f64| = {e_ours:.3e}, |fp32 torch - f64| = {e_ref:.3e}, bound {lim:.3e}")
    assert e_ours <= lim, f"{name}: |ours - f64| = {e_ours:.3e} > {lim:.3e} (fp32 torch {e_ref:.3e})"


def mix_yardstick(P, Q, a, gy, dtype, lamb=0.2):
    """``ops.ata_mix``'s host composition with its gradients, in ``dtype``."""
    P, Q, a = (v.detach().to(dtype).clone().requires_grad_(True) for v in (P, Q, a))
    y, w = ops.ata_mix(P, Q, a, lamb)
    y.backward(gy.to(dtype))
    return y.detach(), w, P.grad, Q.grad, a.grad


def head_yardstick(Z, att, pred, dtype):
    Z, att = (v.detach().to(dtype).clone().requires_grad_(True) for v in (Z, att))
    loss, parts, logits = ops.ata_head_loss(Z, att, pred)
    loss.backward()
    return parts, logits, Z.grad, att.grad


# ---- the op compositions against the brute force ------------------------------------------------------------------------------
def test_sparsemax_known_answers_of_the_reference():
    from pygda_amd import nn as gnn
    f = np.load(os.path.join(HERE, FIXTURES[0]))
    names = sorted({k.split("/")[1] for k in f.files if k.startswith("spx/")})
    assert names == ["dominant", "generic3", "generic8", "single", "tie"]
    for name in names:
        a, want, cot, gwant = (torch.from_numpy(f[f"spx/{name}/{k}"]) for k in ("in", "out", "cot", "grad"))
        for fn in (ops.sparsemax, RefSparsemax.apply, lambda v: gnn.sparsemax(v, 1), gnn.Sparsemax(dim=1)):
            x = a.clone().requires_grad_(True)
            y = fn(x)
            y.backward(cot)
            assert torch.equal(y.detach(), want) and torch.equal(x.grad, gwant), name
        close(ops.sparsemax(a.float()), RefSparsemax.apply(a.float()), want, f"sparsemax {name} in float32")
        assert torch.allclose(want.sum(dim=1), torch.ones(a.size(0), dtype=torch.float64), atol=1e-14)
    assert bool((torch.from_numpy(f["spx/single/out"]) == 1).all())
    assert bool((torch.from_numpy(f["spx/tie/out"]) == 0.25).all())
    dom = torch.from_numpy(f["spx/dominant/out"])
    assert bool(((dom == 0) | (dom == 1)).all()) and bool((dom.sum(dim=1) == 1).all())
    # along another dimension: the transposed problem
    a = torch.from_numpy(f["spx/generic3/in"])
    assert torch.equal(gnn.sparsemax(a.t().contiguous(), 0), torch.from_numpy(f["spx/generic3/out"]).t())


@pytest.mark.parametrize("shape", MIX_SHAPES)
def test_gate_and_mix_compositions_are_the_brute_force(shape):
    n, h, s = shape
    P, Q, a, gy = mix_inputs(n, h, s)
    g, dnr = brute_gate(Q, gy)
    x = Q.clone().requires_grad_(True)
    got = ops.ata_gate(x)
    got.backward(gy)
    assert float((got.detach() - g).abs().max()) <= 1e-12 and float((x.grad - dnr).abs().max()) <= 1e-12
    # the gate's gradient as the header spells it
    sg = torch.sigmoid(Q)
    assert float((dnr - gy * (sg + Q * sg * (1 - sg))).abs().max()) <= 1e-12
    want = brute_mix(P, Q, a, 0.2, gy)
    have = mix_yardstick(P, Q, a, gy, torch.float64)
    for w_, h_, name in zip(want, have, ("y", "w", "dP", "dQ", "da")):
        assert float((w_ - h_).abs().max()) <= 1e-12, name
    y, w, dP, dQ, da = want
    assert torch.allclose(w.sum(dim=1), torch.ones(n, dtype=torch.float64), atol=1e-12)
    # dP_s = w_s gy, dQ = lamb gy, dw_s = <gy, P_s>, da = dw - mean over the support, 0 off it
    dw = torch.stack([(gy * P[:, k * h:(k + 1) * h]).sum(dim=1) for k in range(s)], dim=1)
    on = w != 0
    mean = (dw * on).sum(dim=1, keepdim=True) / on.sum(dim=1, keepdim=True)
    assert float((da - torch.where(on, dw - mean, torch.zeros_like(dw))).abs().max()) <= 1e-12
    assert float((dQ - 0.2 * gy).abs().max()) <= 1e-15
    if n >= 3 and s >= 2:
        assert bool((w[0] == 1.0 / s).all()) and sorted(w[1].tolist()) == [0.0] * (s - 1) + [1.0]
        assert bool((dP[2] == 0).all()) and bool((da[2] == 0).all())
    if s == 1:
        assert bool((w == 1).all()) and bool((da == 0).all())


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_composition_is_the_brute_force(shape):
    n, c, s = shape
    Z, att, pred = head_inputs(n, c, s)
    out, logits, dZ, datt = brute_head(Z, att, pred)
    parts, lg, gZ, gatt = head_yardstick(Z, att, pred, torch.float64)
    assert float((parts - out).abs().max()) <= 1e-12 and float((lg - logits).abs().max()) <= 1e-12
    assert float((gZ - dZ).abs().max()) <= 1e-12 and float((gatt - datt).abs().max()) <= 1e-12
    assert abs(float(out[0] - (out[1] + out[2] + out[3]))) <= 1e-12 and bool(torch.isfinite(out).all())
    assert float((ops.ata_head_loss(Z, att) - logits).abs().max()) <= 1e-12                     # pred=None: the logits
    assert float((ops.ata_head_loss(Z, att.view(-1, 1)) - logits).abs().max()) <= 1e-12         # att as the [C, 1] parameter
    blocks = Z.transpose(0, 1).reshape(n, s * c).view(n, s, c).transpose(0, 1)                   # the column-block view
    assert float((ops.ata_head_loss(blocks, att) - logits).abs().max()) == 0
    if n >= 2:
        p32 = torch.softmax(logits[1].float(), dim=0)
        assert c < 3 or float(p32.min() + 1e-8) == float(torch.tensor(1e-8))                   # spread over 60: p + 1e-8 is 1e-8
    if c >= 3:
        assert int(pred.max()) < c - 1                                                          # a class no row predicts


@pytest.mark.parametrize("variant", ["", "uniform", "tie"])
@pytest.mark.parametrize("shape", VOTE_SHAPES)
def test_vote_composition_is_the_brute_force(shape, variant):
    nn_idx, mem_cls = vote_inputs(*shape, variant=variant)
    want, gap = brute_vote(nn_idx, mem_cls)
    got = ops.ata_vote(nn_idx, mem_cls)
    assert torch.equal(got, want)
    if variant == "uniform":
        assert bool((got == 0).all())
    elif variant == "tie":
        assert int(got[0]) == (1 if shape[2] >= 3 else 0) and float(gap[0]) == 0
    else:
        assert float(gap.min()) >= GAP
    # rank 1 is dropped whichever row it is
    other = nn_idx.clone()
    other[:, 0] = (other[:, 0] + 1) % shape[1]
    assert torch.equal(ops.ata_vote(other, mem_cls), want)


@pytest.mark.parametrize("shape", MEMORY_SHAPES)
def test_memory_composition_is_the_brute_force(shape):
    logits, feat, mem_cls, mem_fea = memory_inputs(*shape)
    for mu in (0.9, 0.5):
        wc, wf = brute_memory(logits, feat, mem_cls, mem_fea, mu)
        c, f_ = mem_cls.clone(), mem_fea.clone()
        ops.ata_memory_update(logits, feat, c, f_, mu)
        assert float((c - wc).abs().max()) <= 1e-12 and float((f_ - wf).abs().max()) <= 1e-12


def test_ops_check_their_shapes():
    P, Q, a, gy = mix_inputs(5, 4, 2)
    for bad in (lambda: ops.ata_mix(P[:, :7], Q, a), lambda: ops.ata_mix(P, Q[:4], a), lambda: ops.sparsemax(a[0]),
                lambda: ops.ata_head_loss(P, a[0]), lambda: ops.ata_head_loss(torch.zeros(2, 5, 3), torch.zeros(4)),
                lambda: ops.ata_head_loss(torch.zeros(2, 5, 3), torch.zeros(3), torch.zeros(4, dtype=torch.long)),
                lambda: ops.ata_vote(torch.zeros(5, 1, dtype=torch.long), torch.zeros(5, 3)),
                lambda: ops.ata_memory_update(torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5, 2), torch.zeros(5, 4)),
                lambda: ops.ata_gate(torch.zeros(0, 3))):
        with pytest.raises(_lib.GdaError, match="expected"):
            bad()


# ---- the two identities the device layer rests on ---------------------------------------------------------------------------
def quirky_graph(n=40, f=12, seed=3):
    """A graph with a duplicate edge, an explicit self loop (twice), a directed-only edge and an isolated node."""
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n - 1, (2, 3 * n), generator=g)                  # node n - 1 is isolated
    ei = torch.cat([ei, ei[:, :1], torch.tensor([[4, 4, 7], [4, 4, 9]])], dim=1)
    x = _f32_exact(torch.randn(n, f, generator=g, dtype=torch.float64))
    return x, ei


def literal_layer(x, edge_index, weights, att, weight, lamb):
    """``NodeCentricConv.forward`` (:246-298) line by line: ``add_remaining_self_loops``, the mean aggregation, the
    EDGE-WISE ``gamma_i * x_j`` and its mean, ``2 S + 1`` projections, the sparsemax blend.  ``weights``: the source
    models' ``lin.weight`` ``[h, F_in]``.  Returns ``(out, w)``."""
    n = x.size(0)
    keep = edge_index[0] != edge_index[1]
    loop = torch.arange(n)
    src, dst = torch.cat([edge_index[0][keep], loop]), torch.cat([edge_index[1][keep], loop])
    cnt = torch.zeros(n, dtype=x.dtype).index_add_(0, dst, torch.ones(dst.numel(), dtype=x.dtype)).clamp(min=1)
    neigh_rep = torch.zeros_like(x).index_add_(0, dst, x[src]) / cnt.unsqueeze(-1)
    gamma = torch.sigmoid(neigh_rep)
    out = torch.zeros_like(x).index_add_(0, dst, gamma[dst] * x[src]) / cnt.view(-1, 1)
    atts, reps = [], []
    for w_s in weights:
        rep = torch.matmul(neigh_rep, w_s.t())
        atts.append(torch.matmul(rep, att))
        reps.append(torch.matmul(out, w_s.t()))
    w = RefSparsemax.apply(torch.cat(atts, dim=1))
    wg = torch.matmul(neigh_rep, weight)
    return torch.sum(w.t().unsqueeze(-1) * torch.stack(reps), dim=0) + wg * lamb, w


def restated_layer(x, edge_index, weights, att, weight, lamb):
    """The device path's arithmetic in torch: ONE aggregation, ``g = sigmoid(nr) nr``, the folded score vectors ``u_s =
    W_s^T att`` (no ``[N, h]`` score projection), one stacked product, ``ops.ata_mix``."""
    from pygda_amd.nn.node_centric_conv import _host_mean, remaining_self_loops
    nr = _host_mean(x, remaining_self_loops(edge_index, x.size(0)))
    g = ops.ata_gate(nr)
    U = torch.cat([w_s.t() @ att for w_s in weights], dim=1)              # [F_in, S]
    P = g @ torch.cat(list(weights), dim=0).t()
    return ops.ata_mix(P, nr @ weight, nr @ U, lamb)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_the_two_identities_against_the_literal_layer(s):
    x, ei = quirky_graph()
    assert int((ei[0] == ei[1]).sum()) >= 2 and not bool((ei == x.size(0) - 1).any())
    g = torch.Generator().manual_seed(11 + s)
    h = 8
    weights = [_f32_exact(torch.randn(h, x.size(1), generator=g, dtype=torch.float64)) * 0.5 for _ in range(s)]
    att, weight = (_f32_exact(torch.randn(*shape, generator=g, dtype=torch.float64)) for shape in ((h, 1), (x.size(1), h)))
    want, w = literal_layer(x, ei, weights, att, weight, 0.2)
    got, gw = restated_layer(x, ei, weights, att, weight, 0.2)
    assert float((got - want).abs().max()) <= 1e-12 and float((gw - w).abs().max()) <= 1e-12
    f32 = lambda v: [t.float() for t in v] if isinstance(v, list) else v.float()                # noqa: E731
    lit32, _ = literal_layer(f32(x), ei, f32(weights), f32(att), f32(weight), 0.2)
    res32, w32 = restated_layer(f32(x), ei, f32(weights), f32(att), f32(weight), 0.2)
    assert torch.equal(w32 != 0, w != 0)
    close(res32, lit32, want, f"S={s} restated layer in float32")
    # the module on host tensors is the literal layer
    from pygda_amd.nn import NodeCentricConv
    conv = NodeCentricConv(x.size(1), h, tuple(torch.nn.Parameter(w_s) for w_s in weights)).double()
    with torch.no_grad():
        conv.att.copy_(att)
        conv.weight.copy_(weight)
    assert float((conv(x, ei).detach() - want).abs().max()) <= 1e-12
    # and the gradients of the folded route are the literal ones
    leaves = [t.clone().requires_grad_(True) for t in weights + [att, weight, x]]
    literal_layer(leaves[-1], ei, leaves[:s], leaves[s], leaves[s + 1], 0.2)[0].square().sum().backward()
    twins = [t.clone().requires_grad_(True) for t in weights + [att, weight, x]]
    restated_layer(twins[-1], ei, twins[:s], twins[s], twins[s + 1], 0.2)[0].square().sum().backward()
    for a_, b_ in zip(leaves, twins):
        assert float((a_.grad - b_.grad).abs().max()) <= 1e-10 * max(float(a_.grad.abs().max()), 1.0)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
def fixture(name):
    f = np.load(os.path.join(HERE, name))
    graph = lambda p: Data(x=torch.from_numpy(f[p + "_x"]), edge_index=torch.from_numpy(f[p + "_ei"].astype(np.int64)),   # noqa: E731
                           y=torch.from_numpy(f[p + "_y"].astype(np.int64)))
    return f, [graph(f"src{i}") for i in range(int(f["S"]))], graph("tgt")


def initial_state(f, prefix):
    grid = float(f["grid"])
    return {k[len("init/" + prefix):]: torch.from_numpy(f[k].astype(np.float32) / grid) for k in f.files
            if k.startswith("init/" + prefix)}


def run_fit(f, sources, t, device, **kw):
    """A fit of the port from the fixture's initial state under its seeds: ``(trainer, what the fixture records)``."""
    from pygda_amd.models import GraphATA
    seeds = [int(v) for v in f["seeds"]]

    def load(stage, obj):
        if stage == "sources":
            for i, net in enumerate(obj):
                net.load_state_dict(initial_state(f, f"src{i}/"))
            torch.manual_seed(seeds[3])
        else:
            obj.load_state_dict(initial_state(f, "ata/"))
            torch.manual_seed(seeds[4])

    m = GraphATA(16, 16, int(f["tgt_y"].max()) + 1, int(f["S"]), K=int(f["K"]), momentum=float(f["momentum"]),
                 num_layers=int(f["num_layers"]), dropout=float(f["dropout"]), lr=float(f["lr"]), epoch=int(f["epochs"]),
                 device=device, verbose=0, record=True, init_hook=load, **kw)
    torch.manual_seed(seeds[0])
    random.seed(seeds[1])
    np.random.seed(seeds[2])
    m.fit(sources, t)
    cpu = lambda v: v.detach().double().cpu().numpy()                       # noqa: E731
    parts = np.array(m.parts_log, dtype=np.float64)
    got = dict(src_losses=np.array([[l for l, _ in log] for log in m.source_log]),
               src_accs=np.array([[a for _, a in log] for log in m.source_log]),
               losses=np.array([l for l, _ in m.target_log]), accs=np.array([a for _, a in m.target_log]),
               total=parts[:, 0], parts=parts[:, 1:], pred=np.stack([p.cpu().numpy() for p in m.pred_log]),
               near=np.stack([p.cpu().numpy() for p in m.near_log]), supp=np.stack([p.cpu().numpy() for p in m.supp_log]),
               mem_cls=cpu(m.mem_cls), mem_fea=cpu(m.mem_fea), logits=cpu(m.predict(t)[0]))
    return m, got


def check_fit_against_fixture(got, f):
    """Every recorded float figure -- the pretraining losses per source, the adaptation losses with ``ent`` / ``div`` /
    ``ce``, the final memory banks and ``predict``'s output -- is held against the fixture's own float32-versus-float64
    distance by the project's bound

        |ours - f64| <= 8 |reference fp32 - f64| + 2e-6 max|f64|            (max norm per figure)

    and printed before it is asserted.  The accuracies, the pseudo labels, the neighbour sets and the layers' support
    sizes are discrete: equal."""
    bad = []
    for k in ("src_losses", "losses", "parts", "mem_cls", "mem_fea", "logits"):
        f64, ref32, ours = f["f64/" + k].astype(np.float64), f[k].astype(np.float64), got[k]
        assert ours.shape == f64.shape, (k, ours.shape, f64.shape)
        e_ours, e_ref = np.abs(ours - f64).max(), np.abs(ref32 - f64).max()
        lim = 8 * e_ref + 2e-6 * max(np.abs(f64).max(), 1e-30)
        print(f"{k}: |ours - f64| = {e_ours:.3e}, |reference fp32 - f64| = {e_ref:.3e}, bound {lim:.3e}")
        if not e_ours <= lim:
            bad.append(k)
    layers = got["supp"].shape[1]
    want = dict(src_accs=f["src_accs"], accs=f["accs"], pred=f["pred"], near=f["near"], supp=f["supp"][:, :layers])
    for k, w in want.items():
        same = got[k].shape == w.shape and np.array_equal(got[k], w)
        print(f"{k}: {'equal' if same else 'DIFFERS'}")
        if not same:
            bad.append(k)
    assert np.abs(got["total"] - got["losses"]).max() <= 1e-6              # the log's loss is parts[0]
    assert not bad, bad


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_what_the_generator_describes(name):
    f, sources, t = fixture(name)
    e, n, k, layers = int(f["epochs"]), t.x.shape[0], int(f["K"]), int(f["num_layers"])
    assert len(sources) == int(f["S"]) and f["pred"].shape == (e, n) and f["near"].shape == (e, n, k)
    assert f["supp"].shape == (e, layers + 1, n) and int(f["supp"].min()) >= 1 and int(f["supp"].max()) <= int(f["S"])
    assert np.all(f["pred"][0] == 0)                        # the class memory starts at exactly 1 / C: every vote a tie
    assert f["mem0"].shape == (n, 16) and f["mem0"].dtype == np.float32
    assert np.abs(f["parts"].sum(axis=1) - f["losses"]).max() <= 1e-5
    keep = (1.0 - float(f["momentum"])) ** e                             # what is left of the initial 1 / C rows
    assert np.abs(f["f64/mem_cls"].sum(axis=0) - (keep * n / 3 + 1 - keep)).max() < 1e-9     # column-normalised updates
    assert os.path.getsize(os.path.join(HERE, name)) < 200 * 1024
    if name.endswith("_c.npz"):
        a = np.load(os.path.join(HERE, FIXTURES[0]))
        assert float(f["dropout"]) == 0.5 and np.abs(f["losses"] - a["losses"]).max() > 1e-3


def test_state_dict_names_are_the_reference_s():
    from pygda_amd.nn import GNNBase, GraphATABase
    f, sources, t = fixture(FIXTURES[0])
    models = [GNNBase(16, 16, 3, num_layers=2, dropout=0.0) for _ in sources]
    for i, net in enumerate(models):
        net.load_state_dict(initial_state(f, f"src{i}/"))                 # strict: shapes and names
    weights = list(zip(*[[p for k, p in net.named_parameters() if k.endswith("lin.weight")] for net in models]))
    ata = GraphATABase(16, 16, 3, weights, models, num_layers=2)
    state = initial_state(f, "ata/")
    assert set(ata.state_dict()) == set(state) == {"convs.0.att", "convs.0.weight", "convs.1.att", "convs.1.weight", "cls.att"}
    ata.load_state_dict(state)
    assert tuple(ata.convs[0].weight.shape) == (16, 16) and tuple(ata.cls.att.shape) == (3, 1)
    assert ata.convs[0].lamb == 0.2 and len(ata.convs[1].weights_list) == 2 and len(list(ata.parameters())) == 5
    out = ata(t.x, t.edge_index)
    assert out.shape == (t.x.shape[0], 3) and torch.allclose(out.exp().sum(dim=1), torch.ones(t.x.shape[0]), atol=1e-5)
    # the classifier entry of the collected lin.weight lists is used by no layer
    assert len(weights) == 3 and all(w is not weights[2][0].t() for w in ata.convs[1].weights_list)


@pytest.mark.parametrize("name", FIXTURES)
def test_host_fit_agrees_with_the_fixture_recorded_from_the_reference(name):
    f, sources, t = fixture(name)
    m, got = run_fit(f, sources, t, "cpu")
    check_fit_against_fixture(got, f)
    assert got["supp"].shape[1] == int(f["num_layers"])


def test_parameters_without_a_gradient_stay_untouched():
    """The source convolutions' biases (and nothing else of the source models' layers) receive no gradient during
    adaptation: with weight decay on, they still end where pretraining left them."""
    f, sources, t = fixture(FIXTURES[1])
    m, _ = run_fit(f, sources, t, "cpu", weight_decay=0.1)
    for net in m.source_model_list:
        assert all(conv.bias.grad is None for conv in net.convs) and net.cls.bias.grad is not None
        assert all(conv.lin.weight.grad is not None for conv in net.convs)
    opt_state = m.optimizer.state
    assert all(conv.bias not in opt_state for net in m.source_model_list for conv in net.convs)


def test_signature_is_the_reference_s_and_the_alias_resolves():
    from pygda_amd.models import GraphATA
    import pygda.models
    import pygda.nn
    assert pygda.models.GraphATA is GraphATA and pygda.nn.GraphATABase is not None
    sig = inspect.signature(GraphATA.__init__)
    want = [("in_dim", inspect._empty), ("hid_dim", inspect._empty), ("num_classes", inspect._empty),
            ("num_src_domains", inspect._empty), ("K", 10), ("momentum", 0.9), ("num_layers", 3), ("dropout", 0.),
            ("act", F.relu), ("weight_decay", 0.), ("lr", 1e-4), ("epoch", 200), ("gnn", 'gcn'), ("mode", 'node'),
            ("device", 'cuda:0'), ("batch_size", 0), ("num_neigh", -1), ("verbose", 2)]
    assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "kwargs")] == want
    from pygda_amd.nn import NodeCentricConv, NodeCentricMLP
    assert list(inspect.signature(NodeCentricConv.__init__).parameters)[1:6] == ["in_channels", "out_channels",
                                                                                  "model_weights", "lamb", "aggr"]
    assert list(inspect.signature(NodeCentricMLP.__init__).parameters)[1:] == ["num_classes", "model_list"]


def test_refusals_name_their_argument():
    from pygda_amd.models import GraphATA
    for key, value in (("mode", "graph"), ("batch_size", 32), ("gnn", "sage")):
        with pytest.raises(NotImplementedError, match=key):
            GraphATA(16, 16, 3, 2, device="cpu", **{key: value})
    f, sources, t = fixture(FIXTURES[0])
    with pytest.raises(ValueError, match="num_src_domains"):
        GraphATA(16, 16, 3, 3, device="cpu").fit(sources, t)
    with pytest.raises(ValueError, match="num_src_domains"):
        GraphATA(16, 16, 3, 1, device="cpu").fit(sources[0], t)
    broken = Data(x=t.x, edge_index=t.edge_index.clone(), y=t.y)
    broken.edge_index[1, 0] = t.x.shape[0]
    with pytest.raises(ValueError, match="edge_index"):
        GraphATA(16, 16, 3, 2, device="cpu").fit(sources, broken)
    with pytest.raises(ValueError, match="neighbours"):
        GraphATA(16, 16, 3, 2, K=t.x.shape[0], device="cpu").fit(sources, t)
    # too many classes or sources for the kernels: refused before anything is built (no device is touched)
    with pytest.raises(ValueError, match="classes"):
        GraphATA(16, 16, ops.ATA_MAX_CLASSES + 1, 2, device="cuda:0").fit(sources, t)
    with pytest.raises(ValueError, match="sources"):
        GraphATA(16, 16, 3, ops.ATA_MAX_SOURCES + 1, device="cuda:0").fit((sources * 5)[:9], t)
    from pygda_amd import distributed
    old = distributed.active
    distributed.active = lambda: True
    try:
        with pytest.raises(NotImplementedError, match="data-parallel"):
            GraphATA(16, 16, 3, 2, device="cpu").fit(sources, t)
    finally:
        distributed.active = old


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def _declared():
    src = open(os.path.join(ROOT, "include", "gda_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): len([p for p in m.group(2).split(",") if p.strip()])
            for m in re.finditer(r"\b(gda_ata_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_every_graphata_entry_is_bound_with_the_declared_argument_count():
    decl = _declared()
    assert len(decl) == 11, sorted(decl)
    L = _lib.lib()
    for name, nargs in decl.items():
        assert name in _lib.EXPORTED_SYMBOLS and len(getattr(L, name).argtypes) == nargs, name
    src = open(os.path.join(ROOT, "include", "gda_hip.h")).read()
    assert "#define GDA_ATA_MAX_SOURCES 8" in src and "#define GDA_ATA_MAX_CLASSES 64" in src
    assert (ops.ATA_MAX_SOURCES, ops.ATA_MAX_CLASSES) == (8, 64)
    from pygda_amd import _build
    assert "gda_graphata.hip" in _build.SOURCES


def test_entry_points_refuse_bad_arguments_with_nothing_launched():
    L = _lib.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)                      # never dereferenced
    big = 1 << 30
    assert L.gda_ata_gate_f32(p, p, 0, None) == -2 and L.gda_ata_gate_f32(None, p, 8, None) == -1
    assert L.gda_ata_gate_f32(odd, p, 8, None) == -4 and L.gda_ata_gate_bwd_f32(p, p, None, None, 8, None) == -1
    assert L.gda_ata_sparsemax_f32(p, 4, 9, p, None) == -4 and L.gda_ata_sparsemax_f32(p, 0, 2, p, None) == -2
    assert L.gda_ata_sparsemax_bwd_f32(p, None, 4, 2, p, None) == -1

    def mix(n=10, h=16, s=2, P=p):
        return L.gda_ata_mix_f32(P, p, p, n, h, s, 0.2, p, p, None)

    assert mix(s=9) == -4 and mix(h=257) == -4 and mix(n=0) == -2 and mix(P=None) == -1 and mix(P=odd) == -4
    assert mix(n=1 << 25) == -2
    assert L.gda_ata_mix_bwd_f32(p, p, p, 10, 16, 9, 0.2, p, p, p, None) == -4
    assert L.gda_ata_mix_bwd_f32(p, p, p, 10, 16, 2, 0.2, p, None, p, None) == -1

    def head(n=10, c=3, s=2, zs=None, zr=None, Z=p, pred=p, out=p, wsb=big):
        return L.gda_ata_head_f32(Z, n * c if zs is None else zs, c if zr is None else zr, p, pred, n, c, s, p, out, p, p,
                                  p, wsb, None)

    assert head(c=65) == -4 and head(s=9) == -4 and head(n=0) == -2 and head(Z=None) == -1 and head(Z=odd) == -4
    assert head(zs=7) == -2 and head(zs=3, zr=5) == -2 and head(out=None) == -1 and head(wsb=16) == -3
    assert L.gda_ata_head_workspace_bytes(10, 3) >= 4 * (10 * 8 + 10 * 4) and L.gda_ata_head_workspace_bytes(10, 65) == 256

    def vote(n=10, nm=10, c=3, k1=6, idx=p):
        return L.gda_ata_vote_f32(idx, p, n, nm, c, k1, p, None)

    assert vote(k1=1) == -2 and vote(k1=17) == -4 and vote(c=65) == -4 and vote(idx=None) == -1 and vote(nm=0) == -2

    def memory(n=10, c=3, d=16, mem=p, wsb=big):
        return L.gda_ata_memory_f32(p, p, n, c, d, 0.1, 0.9, mem, p, p, wsb, None)

    assert memory(c=65) == -4 and memory(d=257) == -4 and memory(n=0) == -2 and memory(mem=None) == -1
    assert memory(wsb=16) == -3 and L.gda_ata_memory_workspace_bytes(10, 3) >= 4 * 10 * 4
    with pytest.raises(_lib.GdaError, match="gda_ata_mix_f32"):
        _lib.call("gda_ata_mix_f32", p, p, p, 10, 16, 9, 0.2, p, p, None)
