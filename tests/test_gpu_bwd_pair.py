"""GPU: a hidden layer's data gradient and weight gradient as two block ranges of one launch, with the preceding
activation's backward in the data-gradient tiles' epilogue (gda_gemm_act_cm_bwd_f32; ops.BWD_PAIR), against the composition
it replaces.  The kernel runs its composition's MFMA chains and the same slab sum, so every comparison here is
``torch.equal`` against the run with ``ops.BWD_PAIR = False``.

The row thresholds that decide which kernels the COMPOSITION takes (``nn.linear.TALL_MIN_ROWS``, ``ops.SKINNY_ROWS``,
``ops.TALL_WGRAD_ROWS``) are lowered for BOTH sides in the trainer test, whose graphs have ~200 nodes."""
import gc

import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from pygda_amd.data import Data
from pygda_amd.nn import linear as linear_mod

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _graph(n, edges, gen):
    e = torch.randint(0, n, (2, edges), generator=gen)
    e = e[:, e[0] != e[1]]
    return torch.cat([e, e.flip(0)], dim=1)


def _record(monkeypatch):
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


# (n, K, M): one slab with a direct write; below / exactly one tile; n_pad != n with ragged tiles; one row past a tile with
# a narrower input; a narrower output.  (1300, 128, 128): from 1024 nodes on the composition's weight gradient is split over
# row slabs (11 here) and n % 4 == 0 takes the branch-free loads -- the path of the full-batch step.
SHAPES = [(1, 128, 128), (63, 128, 128), (64, 128, 128), (203, 128, 128), (257, 64, 128), (203, 128, 64), (1300, 128, 128)]


@pytest.mark.parametrize("want", ["both", "gxT", "gW"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("n,K,M", SHAPES)
def test_target_backward_in_one_launch_equals_the_composition(monkeypatch, n, K, M, p, want):
    """``act_tall_linear_t_backward`` with the flag on against off, on a gradient whose padding columns hold NaN: ``gxT``
    (padding included: exact zeros, no NaN anywhere) and ``gW``, and each output alone."""
    gen = torch.Generator().manual_seed(1000 * n + K + M)
    n_pad = (n + 3) // 4 * 4
    gT = torch.full((M, n_pad), float("nan"))
    gT[:, :n] = torch.randn(M, n, generator=gen)
    gT = gT.to(DEV)
    y = torch.randn(n, K, generator=gen)
    y = (y * (torch.rand(n, K, generator=gen) < 0.5)).clamp_(min=0).to(DEV)       # a dropout(relu(.)) output: about 3/4 zeros
    W = (torch.randn(M, K, generator=gen) / K ** 0.5).to(DEV)
    want_x, want_w = want != "gW", want != "gxT"
    calls = _record(monkeypatch)

    def run(flag):
        monkeypatch.setattr(ops, "BWD_PAIR", flag)
        del calls[:]
        out = ops.act_tall_linear_t_backward(y, W, gT, p, want_x, want_w)
        return out, list(calls)

    (gx_a, gw_a), on = run(True)
    (gx_b, gw_b), off = run(False)
    assert on == ["gda_gemm_act_cm_bwd_f32"] and "gda_gemm_act_cm_bwd_f32" not in off
    assert off.count("gda_gemm_f32") == want_x + want_w and off.count("gda_relu_dropout_bwd_cm_f32") == want_x
    if want_x:
        assert gx_a.shape == (K, n_pad) and torch.equal(gx_a, gx_b)
        assert not torch.isnan(gx_a).any() and (gx_a[:, n:] == 0).all()
    else:
        assert gx_a is None and gx_b is None
    if want_w:
        assert gw_a.shape == (M, K) and torch.equal(gw_a, gw_b) and not torch.isnan(gw_a).any()
    else:
        assert gw_a is None and gw_b is None


@pytest.mark.parametrize("n,K,M", [(203, 128, 256), (1300, 256, 256), (203, 128, 132)])
def test_target_backward_above_128_output_rows_is_the_composition(monkeypatch, n, K, M):
    """Above 128 output rows the composition's data gradient is a sum of slab partials (``split_k`` is true for every TN
    product, ``slabs_for(M) = ceil(M / 128)``), which the one-launch kernel does not reproduce: the helper composes, and
    the flag changes no bit."""
    gen = torch.Generator().manual_seed(1000 * n + K + M)
    n_pad = (n + 3) // 4 * 4
    gT = torch.full((M, n_pad), float("nan"))
    gT[:, :n] = torch.randn(M, n, generator=gen)
    gT = gT.to(DEV)
    y = (torch.randn(n, K, generator=gen) * (torch.rand(n, K, generator=gen) < 0.5)).clamp_(min=0).to(DEV)
    W = (torch.randn(M, K, generator=gen) / K ** 0.5).to(DEV)
    assert ops.BWD_PAIR and not ops.act_tall_linear_bwd_ok(y, W, gT)
    calls = _record(monkeypatch)
    gx_a, gw_a = ops.act_tall_linear_t_backward(y, W, gT, 0.5)
    assert calls == ["gda_gemm_f32", "gda_gemm_f32", "gda_relu_dropout_bwd_cm_f32"]
    monkeypatch.setattr(ops, "BWD_PAIR", False)
    gx_b, gw_b = ops.act_tall_linear_t_backward(y, W, gT, 0.5)
    assert torch.equal(gx_a, gx_b) and torch.equal(gw_a, gw_b)
    assert not torch.isnan(gx_a).any() and (gx_a[:, n:] == 0).all() and not torch.isnan(gw_a).any()


@pytest.mark.parametrize("captured", [False, True])
def test_a2gnn_fit_is_the_same_trajectory(monkeypatch, captured):
    """Three epochs of ``A2GNN.fit``, eager and captured, on two small static graphs (203 and 157 nodes, 128 dense features,
    10 target propagation steps, dropout 0.5), ``BWD_PAIR`` on against off: per-epoch losses and the final ``state_dict``,
    bit for bit.  The entry point is on the step's path when the flag is on and not when it is off."""
    monkeypatch.setattr(linear_mod, "TALL_MIN_ROWS", 128)
    monkeypatch.setattr(ops, "SKINNY_ROWS", 128)
    monkeypatch.setattr(ops, "TALL_WGRAD_ROWS", 128)
    gen = torch.Generator().manual_seed(9)

    def domain(n, edges):
        return Data(x=torch.randn(n, 128, generator=gen), edge_index=_graph(n, edges, gen),
                    y=torch.randint(0, 5, (n,), generator=gen))

    s, t = domain(203, 400), domain(157, 300)
    calls = _record(monkeypatch)
    runs = {}
    for flag in (True, False):
        monkeypatch.setattr(ops, "BWD_PAIR", flag)
        m = pygda_amd.models.A2GNN(128, 128, 5, num_layers=2, dropout=0.5, s_pnums=0, t_pnums=10, adv=False, weight=10,
                                   lr=0.01, weight_decay=0.005, device=DEV, epoch=3, verbose=0, use_hip_graph=captured)
        seen = []
        m.epoch_hook = lambda e, loss, acc, secs: seen.append((loss, acc))
        torch.manual_seed(11)
        torch.cuda.synchronize()
        ops.dropout_state.seed, ops.dropout_state.site = 1234, 0     # the process-wide generator state: same for both runs
        ops.dropout_state.counter(torch.device(DEV)).zero_()
        del calls[:]
        m.fit(s, t)
        torch.cuda.synchronize()
        assert (getattr(m, "_graphed", None) is not None) == captured
        assert (calls.count("gda_gemm_act_cm_bwd_f32") > 0) == flag
        runs[flag] = (seen, {k: v.detach().clone() for k, v in m.a2gnn.state_dict().items()})
        del m
        gc.collect()
    assert len(runs[True][0]) == 3 and runs[True][0] == runs[False][0], (runs[True][0], runs[False][0])
    for k, v in runs[True][1].items():
        assert torch.equal(v, runs[False][1][k]), k
