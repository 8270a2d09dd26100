"""GraphATA on the GPU: the kernels of csrc/gda_graphata.hip against the float64 yardsticks of
tests/test_graphata_host.py under the project's bound (tests/test_gpu_cwgcn._close), two runs bit-identical, the
refusals, the device layer against the literal host layer, device fits against the fixtures recorded from the
reference's graphata.py, eager fits against fits replayed from hipGraphs, and one epoch of each phase at the ACMv9 /
DBLPv7 stand-in shapes."""
import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from pygda_amd.data import Data
from tests.test_gpu_cwgcn import _close
from tests.test_graphata_host import (FIXTURES, GAP, HEAD_SHAPES, MEMORY_SHAPES, MIX_SHAPES, VOTE_SHAPES, brute_gate,
                                      brute_head, brute_memory, brute_mix, brute_vote, check_fit_against_fixture,
                                      fixture, head_inputs, head_yardstick, literal_layer, memory_inputs, mix_inputs,
                                      mix_yardstick, quirky_graph, run_fit, vote_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(gpu, f32, f64, name, slack=2e-6):
    """|gpu - f64| <= 8 |fp32 torch - f64| + 2e-6 max|f64|, the figures printed first."""
    a, b, c = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64) for v in (gpu, f32, f64))
    print(f"{name}: |gpu - f64| = {np.abs(a - c).max():.3e}, |fp32 torch - f64| = {np.abs(b - c).max():.3e}, "
          f"max|f64| = {np.abs(c).max():.3e}")
    _close(gpu, f32, f64, name, slack)


def same_bits(a, b):
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def dev32(*tensors):
    return [t.to(DEV, torch.float32) if t.is_floating_point() else t.to(DEV) for t in tensors]


def mix_run(P, Q, a, gy, lamb=0.2):
    P, Q, a, gy = dev32(P, Q, a, gy)
    nr = Q.clone().requires_grad_(True)
    g = ops.ata_gate(nr)
    g.backward(gy)
    P, Q, a = (v.requires_grad_(True) for v in (P, Q, a))
    y, w = ops.ata_mix(P, Q, a, lamb)
    y.backward(gy)
    sp = a.detach().clone().requires_grad_(True)
    ws = ops.sparsemax(sp)
    ws.backward(a.detach())
    return dict(g=g.detach(), dnr=nr.grad, y=y.detach(), w=w, dP=P.grad, dQ=Q.grad, da=a.grad, sparsemax=ws.detach(),
                dsparsemax=sp.grad)


@pytest.mark.parametrize("shape", MIX_SHAPES)
def test_gate_and_mix_against_float64(shape):
    n, h, s = shape
    P, Q, a, gy = mix_inputs(n, h, s)
    f64 = dict(zip(("y", "w", "dP", "dQ", "da"), brute_mix(P, Q, a, 0.2, gy)))
    f64["g"], f64["dnr"] = brute_gate(Q, gy)
    f32 = dict(zip(("y", "w", "dP", "dQ", "da"), mix_yardstick(P, Q, a, gy, torch.float32)))
    f32["g"], f32["dnr"] = brute_gate(Q.float(), gy.float())
    gpu, again = mix_run(P, Q, a, gy), mix_run(P, Q, a, gy)
    tag = f"N={n} h={h} S={s}"
    for k in gpu:
        assert same_bits(gpu[k], again[k]), f"{tag} {k}: two runs differ"
    assert torch.equal(gpu["w"].cpu() != 0, f64["w"] != 0), f"{tag}: support"
    for k in f64:
        close(gpu[k], f32[k], f64[k], f"{tag} {k}")
    assert same_bits(gpu["sparsemax"], gpu["w"])                            # the plain op is the blend's sparsemax
    sp = f64["w"].clone()
    on = sp != 0
    want = torch.where(on, a - (a * on).sum(1, keepdim=True) / on.sum(1, keepdim=True), torch.zeros_like(a))
    close(gpu["dsparsemax"], want.float(), want, f"{tag} sparsemax backward")
    w = gpu["w"].cpu()
    if n >= 3 and s >= 2:
        assert bool((w[0] == 1.0 / s).all()), f"{tag}: equal scores"                        # exactly 1 / S
        assert sorted(w[1].tolist()) == [0.0] * (s - 1) + [1.0], f"{tag}: a support of one"  # exact zeros elsewhere
        assert bool((gpu["dP"][2] == 0).all()) and bool((gpu["da"][2] == 0).all())          # a zero gy row
    if s == 1:
        assert bool((w == 1).all()) and bool((gpu["da"] == 0).all())


def head_run(Z, att, pred, blocks=False):
    Z, att = dev32(Z, att)
    s, n, c = Z.shape
    if blocks:                                                              # the column blocks of an [N, S C] array
        base = Z.transpose(0, 1).reshape(n, s * c).contiguous().requires_grad_(True)
        Zin = base.view(n, s, c).transpose(0, 1)
    else:
        base = Z.requires_grad_(True)
        Zin = base
    att = att.requires_grad_(True)
    loss, parts, logits = ops.ata_head_loss(Zin, att, pred.to(DEV))
    loss.backward()
    dZ = base.grad.view(n, s, c).transpose(0, 1) if blocks else base.grad
    return dict(parts=parts, logits=logits, dZ=dZ.contiguous(), datt=att.grad)


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_against_float64(shape):
    n, c, s = shape
    Z, att, pred = head_inputs(n, c, s)
    f64 = dict(zip(("parts", "logits", "dZ", "datt"), brute_head(Z, att, pred)))
    f32 = dict(zip(("parts", "logits", "dZ", "datt"), head_yardstick(Z, att, pred, torch.float32)))
    gpu, again, blk = head_run(Z, att, pred), head_run(Z, att, pred), head_run(Z, att, pred, blocks=True)
    tag = f"N={n} C={c} S={s}"
    for k in gpu:
        assert same_bits(gpu[k], again[k]), f"{tag} {k}: two runs differ"
        assert same_bits(gpu[k], blk[k]), f"{tag} {k}: the two layouts differ"
        assert bool(torch.isfinite(gpu[k]).all()), f"{tag} {k}: not finite"
        close(gpu[k], f32[k], f64[k], f"{tag} {k}")
    Zd, attd = dev32(Z, att)
    only = ops.ata_head_loss(Zd, attd)                                      # pred = NULL: forward only
    assert same_bits(only, gpu["logits"]) and not only.requires_grad
    if c >= 3:
        assert int(pred.max()) < c - 1                                      # a class no row predicts


@pytest.mark.parametrize("variant", ["", "uniform", "tie"])
@pytest.mark.parametrize("shape", VOTE_SHAPES)
def test_vote_against_float64(shape, variant):
    nn_idx, mem_cls = vote_inputs(*shape, variant=variant)
    want, gap = brute_vote(nn_idx, mem_cls)
    got = ops.ata_vote(nn_idx.to(DEV, torch.int32), mem_cls.to(DEV, torch.float32))
    again = ops.ata_vote(nn_idx.to(DEV), mem_cls.to(DEV, torch.float32))
    assert got.dtype == torch.int32 and torch.equal(got, again)
    if variant == "":
        assert float(gap.min()) >= GAP
    assert torch.equal(got.cpu().long(), want), f"{shape} {variant}"
    if variant == "uniform":
        assert bool((got == 0).all())
    # an index outside [0, Nm) adds nothing: the vote of the rows that remain
    if shape[3] >= 3 and variant == "uniform":
        out = nn_idx.clone()
        out[:, 1] = shape[1] + 5
        out[0, 2] = -1
        assert bool((ops.ata_vote(out.to(DEV), mem_cls.to(DEV, torch.float32)) == 0).all())


@pytest.mark.parametrize("shape", MEMORY_SHAPES)
def test_memory_update_against_float64(shape):
    logits, feat, mem_cls, mem_fea = memory_inputs(*shape)
    for mu in (0.9, 0.5):
        f64 = brute_memory(logits, feat, mem_cls, mem_fea, mu)
        f32 = brute_memory(*(v.float() for v in (logits, feat, mem_cls, mem_fea)), mu)
        runs = []
        for _ in range(2):
            lg, ft, c, f_ = dev32(logits, feat, mem_cls, mem_fea)
            ops.ata_memory_update(lg, ft, c, f_, mu)
            runs.append((c, f_))
        assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), "two runs differ"
        close(runs[0][0], f32[0], f64[0], f"{shape} mu={mu} mem_cls")
        close(runs[0][1], f32[1], f64[1], f"{shape} mu={mu} mem_fea")


def test_ops_refuse_what_the_kernels_do_not_cover():
    P, Q, a, gy = dev32(*mix_inputs(67, 5, 2))
    with pytest.raises(_lib.GdaError, match="fp32"):
        ops.ata_mix(P.double(), Q.double(), a.double())
    with pytest.raises(_lib.GdaError, match="sources"):
        ops.sparsemax(torch.zeros(4, ops.ATA_MAX_SOURCES + 1, device=DEV))
    with pytest.raises(_lib.GdaError, match="sources"):
        ops.ata_mix(torch.zeros(4, 9 * 4, device=DEV), torch.zeros(4, 4, device=DEV), torch.zeros(4, 9, device=DEV))
    with pytest.raises(_lib.GdaError, match="widths"):
        ops.ata_mix(torch.zeros(4, 2 * 257, device=DEV), torch.zeros(4, 257, device=DEV), torch.zeros(4, 2, device=DEV))
    with pytest.raises(_lib.GdaError, match="classes"):
        ops.ata_head_loss(torch.zeros(2, 4, 65, device=DEV), torch.zeros(65, device=DEV))
    with pytest.raises(_lib.GdaError, match="neighbours"):
        ops.ata_vote(torch.zeros(4, 17, dtype=torch.int32, device=DEV), torch.ones(4, 3, device=DEV))
    with pytest.raises(_lib.GdaError, match="classes"):
        ops.ata_memory_update(torch.zeros(4, 65, device=DEV), torch.zeros(4, 8, device=DEV), torch.zeros(4, 65, device=DEV),
                              torch.zeros(4, 8, device=DEV))
    with pytest.raises(_lib.GdaError, match="expected"):
        ops.ata_mix(P, Q[:5], a)
    L = _lib.lib()
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    assert L.gda_ata_mix_f32(P, Q, a, 67, 5, 9, 0.2, Q, a, None) == -4              # GDA_E_UNSUPPORTED, nothing launched
    assert L.gda_ata_head_f32(P, 7, 3, a, None, 67, 3, 2, Q, None, None, None, ws, ws.numel(), None) == -2    # strides


@pytest.mark.parametrize("s", [1, 3])
def test_device_layer_is_the_literal_layer(s):
    """NodeCentricConv on the device -- one aggregation, the gate, folded score vectors, the stacked product, the mix
    kernel -- against the reference's lines on a graph with a duplicate edge, self loops and an isolated node, forward
    and the gradients of every parameter and of the input."""
    from pygda_amd.nn import NodeCentricConv
    x, ei = quirky_graph()
    g = torch.Generator().manual_seed(11 + s)
    h = 8
    weights = [(torch.randn(h, x.size(1), generator=g, dtype=torch.float64) * 0.5).float().double() for _ in range(s)]
    att, weight = (torch.randn(*shape, generator=g, dtype=torch.float64).float().double()
                   for shape in ((h, 1), (x.size(1), h)))

    def lit(dtype):
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in weights + [att, weight, x]]
        out, w = literal_layer(leaves[-1], ei, leaves[:s], leaves[s], leaves[s + 1], 0.2)
        out.square().sum().backward()
        return [out.detach()] + [t.grad for t in leaves], w.detach()

    f64, w64 = lit(torch.float64)
    f32, _ = lit(torch.float32)
    params = [torch.nn.Parameter(w_.to(DEV, torch.float32)) for w_ in weights]
    conv = NodeCentricConv(x.size(1), h, tuple(params)).to(DEV)
    with torch.no_grad():
        conv.att.copy_(att)
        conv.weight.copy_(weight)
    xd = x.to(DEV, torch.float32).requires_grad_(True)
    out = conv(xd, ei.to(DEV))
    out.square().sum().backward()
    gpu = [out.detach()] + [p.grad for p in params] + [conv.att.grad, conv.weight.grad, xd.grad]
    assert torch.equal(conv.last_w.cpu() != 0, w64 != 0)
    for name, a_, b_, c_ in zip(["out"] + [f"dW{k}" for k in range(s)] + ["datt", "dweight", "dx"], gpu, f32, f64):
        close(a_, b_, c_, f"S={s} {name}")


@pytest.mark.parametrize("name", FIXTURES[:2])
def test_device_fit_agrees_with_the_fixture_recorded_from_the_reference(name):
    f, sources, t = fixture(name)
    m, got = run_fit(f, sources, t, DEV)
    check_fit_against_fixture(got, f)


@pytest.mark.parametrize("name", FIXTURES)                                  # c: with the dropout of both phases live
def test_eager_and_captured_fits_are_bit_identical(name, monkeypatch):
    """Both phases replayed from hipGraphs (two epochs per replay: three replays per phase) against eager epochs: every
    recorded figure, the memory banks and every parameter have the same bits."""
    from pygda_amd import epoch_graph
    f, sources, t = fixture(name)
    fits, captures = [], []
    rolled_back = epoch_graph.capture_rolled_back

    def counted(*args, **kw):
        captures.append(len(kw.get("also", args[4] if len(args) > 4 else ())))
        return rolled_back(*args, **kw)

    monkeypatch.setattr(epoch_graph, "capture_rolled_back", counted)
    for graph in (False, True):
        ops.dropout_state.counter(torch.device(DEV)).zero_()               # the keep-bit stream restarts: the same masks
        fits.append(run_fit(f, sources, t, DEV, use_hip_graph=graph, epochs_per_graph=2))
        # eager: no capture; captured: one per source, then the adaptation's with its memory banks and the counter
        assert captures == ([1] * int(f["S"]) + [3] if graph else []), captures
    (m1, eager), (m2, captured) = fits
    for k in eager:
        assert np.array_equal(eager[k], captured[k]), k
    for a, b in zip(m1.source_model_list + [m1.graphata], m2.source_model_list + [m2.graphata]):
        for (k, v), w in zip(a.state_dict().items(), b.state_dict().values()):
            assert torch.equal(v, w), k
    assert np.isfinite(eager["logits"]).all() and np.isfinite(eager["losses"]).all()
    if float(f["dropout"]) > 0:                                             # the masks are drawn
        g, _, _ = fixture(FIXTURES[0])
        assert np.abs(eager["losses"] - g["losses"]).max() > 1e-3
        assert np.abs(eager["src_losses"] - g["src_losses"]).max() > 1e-3


def test_one_epoch_of_each_phase_at_the_acm_dblp_shapes():
    from bench import make_cfg_a
    src, tgt = make_cfg_a(ns=7410, nt=5578)
    other = Data(x=src.x, edge_index=src.edge_index,
                 y=torch.randint(0, 5, (7410,), generator=torch.Generator().manual_seed(1)).to(src.y.device))
    m = pygda_amd.models.GraphATA(src.x.size(1), 128, 5, 2, K=10, num_layers=2, device=DEV, epoch=1, verbose=0,
                                  record=True, use_hip_graph=False)
    torch.manual_seed(0)
    m.fit([src, other], tgt)
    logits, _ = m.predict(tgt)
    assert len(m.target_log) == 1 and np.isfinite(m.target_log[0][0]) and np.isfinite(m.parts_log).all()
    assert all(len(log) == 1 and np.isfinite(log[0][0]) for log in m.source_log)
    assert logits.shape == (5578, 5) and bool(torch.isfinite(logits).all())
    pred = m.pred_log[0]
    assert pred.shape == (5578,) and int(pred.min()) >= 0 and int(pred.max()) < 5
    assert bool((pred == 0).all())                                          # the class memory starts at exactly 1 / C
    near = m.near_log[0]
    assert near.shape == (5578, 10) and int(near.min()) >= 0 and int(near.max()) < 5578
