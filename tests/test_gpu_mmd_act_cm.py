"""GPU: the one-pass MMD whose target operand is the K-step kernel's column-major pre-activation
(gda_mmd_fused_fwd_act_cm_f32 / gda_mmd_fused_bwd_act_cm_f32; ops.MMD_ACT_CM) against the composition it replaces --
``_ReluDropoutT`` forward, the one-pass MMD on the row-major activation, its scatter, ``_ReluDropoutT`` backward.  The new
kernels apply the same select to the same values and fold the same partials in the same order, so every comparison here is
``torch.equal`` against the run with ``ops.MMD_ACT_CM = False``; one case pins the kept set against the documented Philox
stream itself.

The row thresholds that decide which kernels the composition takes (``nn.linear.TALL_MIN_ROWS``, ``ops.SKINNY_ROWS``,
``ops.TALL_WGRAD_ROWS``) are lowered for BOTH arms in the trainer test, whose graphs have ~200 nodes."""
import gc

import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from pygda_amd.data import Data
from pygda_amd.nn import linear as linear_mod

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, SITE = 1234, 3

# (times, n, d, nseg, target rows nt, how the target rows are drawn)
#   (1, 16, 32)    m = 32: ONE tile holding both domains; nt = n, every row sampled exactly once
#   (1, 20, 32)    n % 32 != 0: a tile straddling the domains, a ragged last tile; nt % 4 != 0 (n_pad != nt)
#   (1, 40, 64)    nt = 257: one past a 64-row tile of the composition, one past sixteen 16-row blocks of the scatter
#   (5, 64, 128)   n % 32 == 0; nt = 50 < n: every row drawn in several resamples (and several times in one)
#   (2, 70, 128)   nt = 1000 >> times * n: most rows never sampled
#   (2, 90, 96), (3, 100, 64)   the remaining width block counts and segment counts
#   (1, 130, 32)   nt = n again, with replacement
CASES = [(1, 16, 32, 1, 16, "perm"), (1, 20, 32, 2, 23, "rand"), (1, 40, 64, 3, 257, "rand"), (5, 64, 128, 4, 50, "rand"),
         (2, 70, 128, 5, 1000, "rand"), (2, 90, 96, 6, 257, "rand"), (3, 100, 64, 7, 301, "rand"), (1, 130, 32, 8, 130, "rand")]


def _record(monkeypatch, keep_args=False):
    """The names of the C-ABI calls, in order.  ``keep_args``: their arguments too (the op-level cases read the gathered
    rows and the partials out of them and drop the list at once).  The trainer test keeps NAMES ONLY: an argument tuple
    holds tensors of the captured step, i.e. blocks of the graph's private memory pool, and a list that outlives the
    trainer keeps that pool from being released with its graph -- it would be torn down whenever the list is cleared, in
    the middle of the next trainer's capture or replays (profiles/HISTORY.md 4.7, "Lifetime")."""
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a if keep_args else None)), real(name, *a))[1])
    return calls


def _philox_keep(seed, step, site, n, p):
    """The kept set of row-major elements 0..n-1 in the format of pygda_amd/csrc/gda_dropout.h, in numpy: Philox-4x32-10
    keyed on the seed, counter {lo(quad), hi(quad), lo(hi), hi(hi)}, hi = (step << 20) ^ site, quad = element >> 2; element
    e is kept when word e & 3 of its quad is >= floor(min(p * 2^32, 2^32 - 1))."""
    u, lo32 = np.uint64, np.uint64(0xFFFFFFFF)
    quad = np.arange((n + 3) // 4, dtype=np.uint64)
    hi = ((step << 20) ^ site) & (2 ** 64 - 1)
    c = [quad & lo32, quad >> u(32), np.full_like(quad, hi & 0xFFFFFFFF), np.full_like(quad, hi >> 32)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c[0], u(0xCD9E8D57) * c[2]
        c = [(p1 >> u(32)) ^ c[1] ^ u(k0), p1 & lo32, (p0 >> u(32)) ^ c[3] ^ u(k1), p0 & lo32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    thresh = int(min(float(np.float32(p)) * 2.0 ** 32, 2.0 ** 32 - 1))
    return torch.from_numpy(np.stack(c, axis=1).reshape(-1)[:n] >= u(thresh))


def _inputs(times, n, d, nt, draw, gen, positive=False):
    ns = n + 7
    n_pad = (nt + 3) // 4 * 4
    src = torch.randn(ns, d, generator=gen)
    x = torch.randn(nt, d, generator=gen)                      # negative, zero and positive entries
    x[torch.rand(nt, d, generator=gen) < 0.1] = 0.0
    if positive:
        x = 1.0 + torch.rand(nt, d, generator=gen)
    xT = torch.full((d, n_pad), float("nan"))                  # NaN in the padding columns: never read as values
    xT[:, :nt] = x.t()
    s_cpu = torch.randint(ns, (times, n), generator=gen)
    t_cpu = torch.randperm(nt, generator=gen)[:n].view(1, n) if draw == "perm" else torch.randint(nt, (times, n), generator=gen)
    return src.to(DEV), xT.to(DEV), s_cpu, t_cpu, ns, n_pad


def _run(flag, monkeypatch, calls, src0, xT0, idx_s, idx_t, sel, nt, p):
    """Loss, gathered target rows, row-gradient partials, source gradient and the pre-activation's column-major gradient
    of one arm; the generator triple is the same explicit one in both."""
    monkeypatch.setattr(ops, "MMD_ACT_CM", flag)
    src, xT = src0.clone().requires_grad_(), xT0.clone().requires_grad_()
    step = ops.dropout_state.counter(torch.device(DEV))
    feat = ops.PreActCM(ops.ColMajor(xT, nt), p, (SEED, step, SITE))
    del calls[:]
    loss = ops.mmd_loss(src, feat, idx_s, idx_t, sel=sel, scale=2.5)
    gs, gxT = torch.autograd.grad(loss, [src, xT], torch.tensor(0.75, device=DEV))     # a non-unit upstream gradient
    torch.cuda.synchronize()
    names = [c[0] for c in calls]
    if flag:
        assert "gda_mmd_fused_fwd_act_cm_f32" in names and "gda_mmd_fused_bwd_act_cm_f32" in names
        assert "gda_relu_dropout_fwd_cm_f32" not in names and "gda_relu_dropout_bwd_cm_f32" not in names
        fwd = next(a for k, a in calls if k == "gda_mmd_fused_fwd_act_cm_f32")
        rows_t, part = fwd[16], fwd[19]
    else:
        assert "gda_mmd_fused_fwd_act_cm_f32" not in names and "gda_mmd_fused_bwd_act_cm_f32" not in names
        assert "gda_relu_dropout_fwd_cm_f32" in names and "gda_relu_dropout_bwd_cm_f32" in names
        fwd = next(a for k, a in calls if k == "gda_mmd_fused_fwd_f32")
        rows_t, part = fwd[15], fwd[18]
    out = loss.detach().clone(), rows_t.clone(), part.clone(), gs.clone(), gxT.clone()
    del calls[:], fwd
    return out


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("times,n,d,nseg,nt,draw", CASES)
def test_op_equals_the_composition(monkeypatch, times, n, d, nseg, nt, draw, p):
    assert ops.mmd_one_pass_ok(torch.device(DEV))
    assert ops.mmd_one_pass_segments(times, n, d) == nseg
    gen = torch.Generator().manual_seed(1000 * n + d)
    src, xT, s_cpu, t_cpu, ns, n_pad = _inputs(times, n, d, nt, draw, gen)
    idx_s, idx_t, sel = ops.mmd_samples_to_device(s_cpu, t_cpu, ns, nt, torch.device(DEV))
    ops.dropout_state.next_step(torch.device(DEV))
    calls = _record(monkeypatch, keep_args=True)
    new = _run(True, monkeypatch, calls, src, xT, idx_s, idx_t, sel, nt, p)
    again = _run(True, monkeypatch, calls, src, xT, idx_s, idx_t, sel, nt, p)
    ref = _run(False, monkeypatch, calls, src, xT, idx_s, idx_t, sel, nt, p)
    for name, a, b, c in zip(("loss", "rows_tgt", "partials", "source gradient", "gxT"), new, again, ref):
        assert not torch.isnan(a).any(), name
        assert torch.equal(a, b), name + ": two runs of the new path differ"
        assert torch.equal(a, c), name
    gxT = new[4]
    assert gxT.shape == (d, n_pad) and (gxT[:, nt:] == 0).all()                 # the padding columns: exact zeros
    never = torch.ones(nt, dtype=torch.bool)
    never[t_cpu.reshape(-1)] = False
    assert (gxT[:, :nt][:, never.to(DEV)] == 0).all()                            # rows nobody sampled: exact zeros
    if draw == "perm":
        assert not never.any()
    if nt == 1000:
        assert never.sum() > nt // 2
    if nt == 50:
        assert torch.bincount(t_cpu.reshape(-1), minlength=nt).max() > times     # a row drawn more often than once per resample
    assert gxT.abs().sum() > 0 and new[3].abs().sum() > 0


def test_kept_set_is_the_documented_philox_stream(monkeypatch):
    """Strictly positive pre-activations (the relu hides nothing), every target row sampled once: a gathered row's positive
    entries are exactly the kept elements ``g * d + c`` of the documented stream, and the gradient's non-zero pattern is
    drawn from the same key in the backward launch."""
    times, n, d, nt, p = 1, 40, 64, 40, 0.5
    gen = torch.Generator().manual_seed(5)
    src, xT, s_cpu, t_cpu, ns, n_pad = _inputs(times, n, d, nt, "perm", gen, positive=True)
    idx_s, idx_t, sel = ops.mmd_samples_to_device(s_cpu, t_cpu, ns, nt, torch.device(DEV))
    ops.dropout_state.next_step(torch.device(DEV))
    calls = _record(monkeypatch, keep_args=True)
    _, rows_t, _, _, gxT = _run(True, monkeypatch, calls, src, xT, idx_s, idx_t, sel, nt, p)
    step = int(ops.dropout_state.counter(torch.device(DEV)).item())
    keep = _philox_keep(SEED, step, SITE, nt * d, p).view(nt, d)
    assert 0.4 < keep.float().mean() < 0.6
    assert torch.equal((rows_t > 0).cpu(), keep[t_cpu.reshape(-1)])
    x = xT[:, :nt].t().cpu()
    assert torch.equal(rows_t.cpu(), torch.where(keep, x * np.float32(1.0 / (1.0 - p)), torch.zeros(()))[t_cpu.reshape(-1)])
    assert not ((gxT[:, :nt].t().cpu() != 0) & ~keep).any()                      # nothing flows through a dropped element


def _graph(n, edges, gen):
    e = torch.randint(0, n, (2, edges), generator=gen)
    e = e[:, e[0] != e[1]]
    return torch.cat([e, e.flip(0)], dim=1)


@pytest.mark.parametrize("captured", [False, True])
def test_a2gnn_fit_is_the_same_trajectory(monkeypatch, captured):
    """Three epochs of ``A2GNN.fit``, eager and captured, on two small static graphs (203 and 157 nodes, 128 dense features,
    10 target propagation steps, dropout 0.5), ``MMD_ACT_CM`` on against off: per-epoch losses, the target predictions and
    the final ``state_dict``, bit for bit.  With the flag on the step issues the new entry points and neither of the
    column-major activation launches; with it off the other way round."""
    monkeypatch.setattr(linear_mod, "TALL_MIN_ROWS", 128)
    monkeypatch.setattr(ops, "SKINNY_ROWS", 128)
    monkeypatch.setattr(ops, "TALL_WGRAD_ROWS", 128)
    gen = torch.Generator().manual_seed(9)

    def domain(n, edges):
        return Data(x=torch.randn(n, 128, generator=gen), edge_index=_graph(n, edges, gen),
                    y=torch.randint(0, 5, (n,), generator=gen))

    s, t = domain(203, 400), domain(157, 300)
    assert ops.mmd_one_pass_ok(torch.device(DEV))
    calls = _record(monkeypatch)
    runs = {}
    for flag in (True, False):
        monkeypatch.setattr(ops, "MMD_ACT_CM", flag)
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
        names = [c[0] for c in calls]
        new = names.count("gda_mmd_fused_fwd_act_cm_f32"), names.count("gda_mmd_fused_bwd_act_cm_f32")
        old = names.count("gda_relu_dropout_fwd_cm_f32"), names.count("gda_relu_dropout_bwd_cm_f32")
        if flag:
            assert new[0] > 0 and new[0] == new[1] and old == (0, 0), (new, old)
        else:
            assert new == (0, 0) and old[0] > 0 and old[1] > 0, (new, old)
        logits, labels = m.predict(t)
        runs[flag] = (seen, logits.detach().clone(), {k: v.detach().clone() for k, v in m.a2gnn.state_dict().items()})
        del m, logits, labels
        torch.cuda.synchronize()
        gc.collect()                  # the trainer's graphs and their pool go here, with the device idle
    assert len(runs[True][0]) == 3 and runs[True][0] == runs[False][0], (runs[True][0], runs[False][0])
    assert torch.equal(runs[True][1], runs[False][1])
    for k, v in runs[True][2].items():
        assert torch.equal(v, runs[False][2][k]), k
