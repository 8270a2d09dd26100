"""GPU: the activation between two conv layers applied by the CONSUMING projection (gda_gemm_act_cm_f32,
gda_gemm_skinny_act_cm_f32; ops.ACT_IN_CONSUMER) against the composition it replaces -- the activation launch
(gda_relu_dropout_fwd_cm_f32) followed by the projection.  Both kernels reproduce their compositions' arithmetic, so every
comparison here is ``torch.equal``.

Two row thresholds decide which kernels the COMPOSITION takes: ``nn.linear.TALL_MIN_ROWS`` (1024: the column-major
projection + LDS K-step route of a hidden layer) and ``ops.SKINNY_ROWS`` (2048: the classifier's vector kernel).  The small
graphs of the layer and trainer tests (and n = 203 of the classifier test) sit below them; those tests lower the thresholds
for BOTH sides, so the 203-node cases compare the new kernels with the kernels they reproduce."""
import gc

import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from pygda_amd.data import Data
from pygda_amd.graph import as_graph
from pygda_amd.nn import A2GNNBase
from pygda_amd.nn import linear as linear_mod

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _state(step=7):
    ops.dropout_state.counter(torch.device(DEV)).fill_(step)
    ops.dropout_state.site = 0


def _colmajor(n, K, gen):
    """A pre-activation as the K-step kernel leaves it; the padding columns hold NaN (no result may depend on them)."""
    n_pad = (n + 3) // 4 * 4
    xT = torch.full((K, n_pad), float("nan"))
    xT[:, :n] = torch.randn(K, n, generator=gen)
    return xT.to(DEV)


def _graph(n, edges, gen):
    e = torch.randint(0, n, (2, edges), generator=gen)
    e = e[:, e[0] != e[1]]
    ei = torch.cat([e, e.flip(0)], dim=1)
    return ei


SHAPES = [(1, 128, 128), (63, 128, 128), (64, 128, 128), (203, 128, 128), (257, 64, 128), (203, 128, 64)]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("n,K,M", SHAPES)
def test_projection_with_the_activation_on_its_operand_load_equals_the_composition(n, K, M, p, training):
    """Kernel 1 against ``relu_dropout(ColMajor)`` then ``tall_linear_colmajor`` at the same step and site: the activation
    ``y``, the product ``hT[:, :n]``, the column-major input gradient and the weight gradient; and ``hT`` again with
    ``y = NULL`` under ``no_grad``.  203 nodes: ``n_pad = 204 != n`` and ragged tiles; 257: one row past a tile."""
    gen = torch.Generator().manual_seed(1000 * n + K + M)
    xT0 = _colmajor(n, K, gen)
    W0 = (torch.randn(M, K, generator=gen) / K ** 0.5).to(DEV)
    g = torch.randn(M, n, generator=gen).to(DEV)

    def run(fused):
        xT, W = xT0.clone().requires_grad_(), W0.clone().requires_grad_()
        x = ops.ColMajor(xT, n)
        _state()
        if fused:
            assert ops.act_tall_linear_ok(x, W)
            h = ops.act_tall_linear_colmajor(x, W, p, training)
            y = h.t.grad_fn.saved_tensors[0]
        else:
            y = ops.relu_dropout(x, p, training)
            h = ops.tall_linear_colmajor(y, W)
        assert ops.dropout_state.site == 1
        (h.t[:, :n] * g).sum().backward()
        return y.detach(), h.t.detach()[:, :n], xT.grad, W.grad

    a, b = run(True), run(False)
    for name, u, v in zip(("y", "hT", "grad xT", "grad W"), a, b):
        assert u.shape == v.shape and torch.equal(u, v), name
    assert not torch.isnan(a[2]).any()                       # the padding columns of the gradient are zeros
    with torch.no_grad():                                    # y = NULL: a pass that is not differentiated
        _state()
        h = ops.act_tall_linear_colmajor(ops.ColMajor(xT0, n), W0, p, training)
    assert torch.equal(h.t[:, :n], b[1])


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("classes", [5, 8])
@pytest.mark.parametrize("n", [203, 2053, 4100])
def test_classifier_projection_reading_the_colmajor_preactivation(monkeypatch, n, classes, K, p):
    """Kernel 2 against ``relu_dropout(ColMajor)`` then the classifier's ``Linear`` (k_skinny_fwd: the kernel whose eight
    chains and addition tree it reproduces; at n = 203 the threshold is lowered so that the composition takes it)."""
    monkeypatch.setattr(ops, "SKINNY_ROWS", 128)
    gen = torch.Generator().manual_seed(77 * n + classes + K)
    xT = _colmajor(n, K, gen)
    torch.manual_seed(n + classes)
    lin = linear_mod.Linear(K, classes, bias=False).to(DEV)
    x = ops.ColMajor(xT, n)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with torch.no_grad():
        _state()
        ref = lin(ops.relu_dropout(x, p, True))
        assert calls == ["gda_relu_dropout_fwd_cm_f32", "gda_gemm_skinny_f32"]
        _state()
        assert ops.act_skinny_ok(x, lin.weight)
        got = ops.act_skinny_linear(x, lin.weight, p, True)
    assert calls[2:] == ["gda_gemm_skinny_act_cm_f32"]
    assert got.shape == (n, classes) and torch.equal(got, ref)


def test_a2gnn_layers_hand_the_preactivation_to_the_consuming_projection(monkeypatch):
    """Two hidden layers over a static 203-node graph on the LDS K-step: ``ACT_IN_CONSUMER`` on against off.  The feature
    pass with gradients (output, input gradient, every parameter gradient) and the ``no_grad`` logits pass through
    ``feat_classifier`` are equal; the feature pass launches the activation kernel ONCE (its last activation feeds the MMD
    and stays), the logits pass not at all."""
    monkeypatch.setattr(linear_mod, "TALL_MIN_ROWS", 128)
    monkeypatch.setattr(ops, "SKINNY_ROWS", 128)
    gen = torch.Generator().manual_seed(5)
    n = 203
    ei = _graph(n, 400, gen).to(DEV)
    ei._gda_static = True
    G = as_graph(ei, n)
    assert G.static and ops.lds_kstep_plan(G, 10, False) is not None and ops.lds_kstep_plan(G, 10, True) is not None
    x0 = torch.randn(n, 128, generator=gen).to(DEV)
    gy = torch.randn(n, 128, generator=gen).to(DEV)
    torch.manual_seed(3)
    net = A2GNNBase(128, 128, 5, num_layers=2, dropout=0.5).to(DEV).train()
    with torch.no_grad():
        for conv in (*net.convs, net.cls):
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen))
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])

    def run(flag):
        monkeypatch.setattr(ops, "ACT_IN_CONSUMER", flag)
        net.zero_grad()
        x = x0.clone().requires_grad_()
        _state()
        del calls[:]
        h0 = net.first_conv(x, ei, 10)
        assert isinstance(h0, ops.ColMajor)
        feats = net.feat_bottleneck_from(h0, ei, None, 10)
        feat_calls = list(calls)
        (feats * gy).sum().backward()
        grads = [p.grad.clone() for c in net.convs for p in c.parameters()]
        del calls[:]
        with torch.no_grad():
            h0 = net.first_conv(x0, ei, 10)
            del calls[:]
            logits = net.feat_classifier(net.feat_bottleneck_from(h0.detach(), ei, None, 10, draw=1, preact_out=True),
                                         ei, None, 1)
        return feats.detach(), x.grad, grads, logits, feat_calls, list(calls)

    on, off = run(True), run(False)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and torch.equal(on[3], off[3])
    assert len(on[2]) == len(off[2]) == 4
    for u, v in zip(on[2], off[2]):
        assert torch.equal(u, v)
    assert on[4].count("gda_relu_dropout_fwd_cm_f32") == 1 and on[4].count("gda_gemm_act_cm_f32") == 1
    assert on[5].count("gda_relu_dropout_fwd_cm_f32") == 0
    assert on[5].count("gda_gemm_act_cm_f32") == 1 and on[5].count("gda_gemm_skinny_act_cm_f32") == 1
    assert off[4].count("gda_relu_dropout_fwd_cm_f32") == 2 and off[5].count("gda_relu_dropout_fwd_cm_f32") == 2
    assert "gda_gemm_act_cm_f32" not in off[4] + off[5] and "gda_gemm_skinny_act_cm_f32" not in off[5]
    assert off[5].count("gda_gemm_skinny_f32") == 1          # the kernel the fused classifier projection reproduces


def test_a2gnn_captured_fit_is_the_same_trajectory(monkeypatch):
    """Three captured epochs of ``A2GNN.fit`` on two small static graphs (203 and 157 nodes, 128 dense features, 10 target
    propagation steps, dropout 0.5), ``ACT_IN_CONSUMER`` on against off: per-epoch losses, the final ``state_dict`` and the
    target logits ``forward_model`` returns, bit for bit."""
    monkeypatch.setattr(linear_mod, "TALL_MIN_ROWS", 128)
    monkeypatch.setattr(ops, "SKINNY_ROWS", 128)
    gen = torch.Generator().manual_seed(9)

    def domain(n, edges):
        return Data(x=torch.randn(n, 128, generator=gen), edge_index=_graph(n, edges, gen),
                    y=torch.randint(0, 5, (n,), generator=gen))

    s, t = domain(203, 400), domain(157, 300)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    runs = {}
    for flag in (True, False):
        monkeypatch.setattr(ops, "ACT_IN_CONSUMER", flag)
        m = pygda_amd.models.A2GNN(128, 128, 5, num_layers=2, dropout=0.5, s_pnums=0, t_pnums=10, adv=False, weight=10,
                                   lr=0.01, weight_decay=0.005, device=DEV, epoch=3, verbose=0, use_hip_graph=True)
        seen = []
        m.epoch_hook = lambda e, loss, acc, secs: seen.append((loss, acc))
        torch.manual_seed(11)
        torch.cuda.synchronize()
        ops.dropout_state.seed, ops.dropout_state.site = 1234, 0     # the process-wide generator state: same for both runs
        ops.dropout_state.counter(torch.device(DEV)).zero_()
        del calls[:]
        m.fit(s, t)
        assert getattr(m, "_graphed", None) is not None, "step was not captured"
        fused = calls.count("gda_gemm_act_cm_f32"), calls.count("gda_gemm_skinny_act_cm_f32")
        assert (fused[0] > 0 and fused[1] > 0) if flag else fused == (0, 0)
        state = {k: v.detach().clone() for k, v in m.a2gnn.state_dict().items()}
        src = next(iter(m.source_loader)).to(DEV)
        tgt = next(iter(m.target_loader)).to(DEV)
        m.a2gnn.train()
        torch.manual_seed(12)
        ops.dropout_state.next_step(torch.device(DEV))
        _, _, target_logits = m.forward_model(src, tgt, 1.0)
        torch.cuda.synchronize()
        runs[flag] = (seen, state, target_logits.detach().clone())
        del m
        gc.collect()
    assert len(runs[True][0]) == 3 and runs[True][0] == runs[False][0], (runs[True][0], runs[False][0])
    for k, v in runs[True][1].items():
        assert torch.equal(v, runs[False][1][k]), k
    assert torch.equal(runs[True][2], runs[False][2])
