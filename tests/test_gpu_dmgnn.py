"""DMGNN on the MI355X: its kernels (csrc/gda_dmgnn.hip, the heads shared with ACDNE in csrc/gda_acdne.hip) against
float64 (the proximity loss and the heads at several batch sizes, an odd one among them, the heads with all-zero blocks
against ACDNE's heads; predict's ``P + M P`` up to N = 9,360 with garbage in the padding columns), two
runs bit-identical, the normalised blocks against the float64 block and against the ones ACDNE's kernel uses, the
3-epoch fit against the reference's fixture with the bound taken from the float64 restatement, eager and captured fits
bit-identical, one full-size epoch at the DBLPv7 -> Citationv1 shapes, and no BLAS product on the path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import _lib, ops
from tests.conftest import load_golden
from tests.test_dmgnn_host import _check_step, _step64, check_fit_against_fixture, run_fit
from tests.test_gpu_acdne import _close, _step_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("h,e,c", [(20, 12, 3), (37, 128, 5), (50, 128, 5), (128, 64, 7)])
def test_prox_and_heads_against_float64(h, e, c):
    ps, pt, pidx, rows, z, y, params = _step_inputs(h, e, c, h * 31 + c)
    alpha, pw = 0.7, 0.1
    total64, g64, parts, a64 = _step64(ps, pt, pidx, rows, z, y, params, alpha, pw)
    d = [t.to(DEV) for t in (ps, pt, pidx, rows, z, y)]
    dp = [p.to(DEV) for p in params]
    al = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)

    def run():
        prox, gprox, a = ops.dmgnn_prox(d[0], d[1], d[2], d[4], h, pw)
        return prox, gprox, a, ops.dmgnn_heads(d[4], gprox, a, dp, d[5], d[3], al, prox, pw, loss_acc=acc)

    prox, gprox, a, got = run()
    a32 = torch.stack([(1.0 / (b.sum(1) + 1e-12))[:, None] * b for b in
                       (M[ix][:, ix].clone().fill_diagonal_(0) for M, ix in ((ps, pidx[:h]), (pt, pidx[h:])))])
    _close(a, a32, a64, "a_blocks")
    np.testing.assert_allclose(prox.cpu().numpy(), parts["prox"].detach().numpy(), rtol=2e-5)
    _check_step(got, (total64, g64))
    assert acc.item() == got[0].item()
    prox2, gprox2, a2, (loss2, dz2, grads2) = run()
    assert torch.equal(prox, prox2) and torch.equal(gprox, gprox2) and torch.equal(a, a2) and torch.equal(got[0], loss2)
    assert torch.equal(got[1], dz2) and all(torch.equal(x, y_) for x, y_ in zip(got[2], grads2))


@pytest.mark.parametrize("h,e,c", [(20, 12, 3), (37, 128, 5)])
def test_heads_with_zero_blocks_are_acdne_heads(h, e, c):
    """The one kernel's two paths stay in step: with all-zero blocks the propagation adds zeros, so DMGNN's heads return
    ACDNE's loss, dz and eight gradients exactly and advance ``loss_acc`` by the same value."""
    ps, pt, pidx, rows, z, y, params = _step_inputs(h, e, c, h * 31 + c)
    d = [t.to(DEV) for t in (ps, pt, pidx, rows, z, y)]
    dp = [p.to(DEV) for p in params]
    al = torch.tensor(0.7, dtype=torch.float32, device=DEV)
    prox, gprox = ops.acdne_prox(d[0], d[1], d[2], d[4], h, 0.1)
    acc = torch.full((2,), 1.5, dtype=torch.float64, device=DEV)
    want = ops.acdne_heads(d[4], gprox, dp, d[5], d[3], al, prox, 0.1, loss_acc=acc[:1])
    got = ops.dmgnn_heads(d[4], gprox, torch.zeros(2, h, h, device=DEV), dp, d[5], d[3], al, prox, 0.1,
                          loss_acc=acc[1:])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and len(got[2]) == len(want[2]) == 8
    for a, b in zip(got[2], want[2]):
        assert torch.equal(a, b)
    assert acc[0].item() == acc[1].item() == 1.5 + want[0].item()


def test_blocks_are_the_ones_acdne_prox_uses():
    """For embeddings with |e_i|^2 = 1 and e_i . e_j = 0 (distinct unit vectors) ACDNE's loss is mean_i sum_j a_ij * 2 =
    2 mean_i rowsum_i(A): computed from ``a_blocks`` in the kernel's order it equals gda_acdne_prox_f32's loss to the
    rounding of A's entries to fp32 (the ACDNE kernel keeps the product of scale and entry in double)."""
    h, e = 50, 128
    ps, pt, pidx, rows, _, _, _ = _step_inputs(h, e, 5, 77)
    z = torch.zeros(2 * h, e)
    z[torch.arange(2 * h), torch.arange(2 * h) % h] = 1.0
    d = [t.to(DEV) for t in (ps, pt, pidx, z)]
    acdne_loss, _ = ops.acdne_prox(d[0], d[1], d[2], d[3], h, 0.1)
    _, _, a = ops.dmgnn_prox(d[0], d[1], d[2], d[3], h, 0.1)
    mine = 2.0 * a.double().sum(2).mean(1)
    np.testing.assert_allclose(mine.cpu().numpy(), acdne_loss.cpu().numpy(), rtol=1e-7)


def test_prox_with_a_zero_norm_has_a_zero_finite_gradient_and_checks_its_arguments():
    h, e = 20, 12
    full = torch.zeros(h, h)
    full[torch.arange(h), (torch.arange(h) + 1) % h] = 1.0
    ring = torch.cat([torch.arange(h), torch.arange(h)]).to(DEV)
    row = torch.rand(1, e) + 0.5
    for z in (row.expand(2 * h, e).contiguous(), -torch.ones(2 * h, e)):
        prox, gprox, a = ops.dmgnn_prox(full.to(DEV), full.to(DEV), ring, z.to(DEV), h, 0.1)
        assert torch.equal(a[0].cpu(), full) and prox.tolist() == [0.0, 0.0]
        assert torch.isfinite(gprox).all() and not gprox.any()
    # an index outside the domain reads zero
    far = ring.clone()
    far[0] = 10_000
    prox, gprox, a = ops.dmgnn_prox(full.to(DEV), full.to(DEV), far, row.expand(2 * h, e).contiguous().to(DEV), h, 0.1)
    assert not a[0, 0].any() and not a[0, :, 0].any() and prox[0] > 0 and torch.isfinite(gprox).all()
    z = torch.zeros(2 * h, e, device=DEV)
    with pytest.raises(_lib.GdaError, match="square"):
        ops.dmgnn_prox(torch.zeros(h, h + 4, device=DEV), full.to(DEV), ring, z, h, 0.1)
    with pytest.raises(_lib.GdaError, match="rows"):
        ops.dmgnn_prox(full.to(DEV), full.to(DEV), ring[:-1], z, h, 0.1)
    with pytest.raises(_lib.GdaError, match="a_blocks"):
        ops.dmgnn_heads(z, z, torch.zeros(2, h, h + 1, device=DEV), [torch.zeros(3, e, device=DEV)] * 2 +
                        [torch.zeros(128, e, device=DEV)] + [None] * 5, ring, ring, z[0, 0], z[0, :2].double(), 0.1)
    with pytest.raises(_lib.GdaError, match="16-byte"):
        ops.dmgnn_predict(torch.zeros(7, e, device=DEV), torch.zeros(3, e, device=DEV), torch.zeros(3, device=DEV),
                          torch.zeros(7, 7, device=DEV))


@pytest.mark.parametrize("n,c", [(n, c) for n in (160, 1001, 9360) for c in (3, 5, 7)] + [(1001, 11)])
def test_predict_against_float64(n, c):
    """``P + M P`` with M a non-negative matrix of PPMI-like density in a [n, round_up(n, 4)] buffer whose padding
    columns hold NaN on purpose (n = 1001): the kernel never uses them.  c = 11 takes the wide-head kernel."""
    g = torch.Generator().manual_seed(n + c)
    e, ld = 128, (n + 3) // 4 * 4
    buf = torch.full((n, ld), float("nan"))
    buf[:, :n] = torch.rand(n, n, generator=g) * 6 * (torch.rand(n, n, generator=g) < 0.05)
    z, w, b = torch.randn(n, e, generator=g), torch.randn(c, e, generator=g) * 0.2, torch.randn(c, generator=g) * 0.1
    buf, z, w, b = (t.to(DEV) for t in (buf, z, w, b))
    M = buf[:, :n]

    def torch_out(dtype):
        p = torch.softmax(torch.relu(z.to(dtype)) @ w.to(dtype).T + b.to(dtype), 1)
        return p + M.to(dtype) @ p

    out = ops.dmgnn_predict(z, w, b, M)
    assert out.shape == (n, c) and torch.isfinite(out).all()
    _close(out, torch_out(torch.float32), torch_out(torch.float64), "P + M P", 1e-5)
    assert torch.equal(out, ops.dmgnn_predict(z, w, b, M))


def test_fit3_against_the_reference_bounded_by_the_float64_restatement():
    check_fit_against_fixture(run_fit(DEV, use_hip_graph=True, steps_per_graph=4), load_golden("dmgnn_fit3"))


def test_eager_and_captured_fits_are_bit_identical():
    a = run_fit(DEV, use_hip_graph=True, steps_per_graph=4)
    b = run_fit(DEV, use_hip_graph=False, steps_per_graph=4)
    c = run_fit(DEV, use_hip_graph=True, steps_per_graph=3)     # 8 steps: two replays of 3 and two eager steps
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], c[k]), k


def test_one_full_size_epoch_at_dblp_citation_shapes():
    from bench import make_cfg_a
    src, tgt = make_cfg_a(seed=7, ns=5484, es=8117, nt=8935, et=15098)
    m = pygda_amd.models.DMGNN(src.x.size(1), 128, 5, dropout=0.5, weight_decay=1e-3, lr=1e-3, device=DEV, epoch=1,
                               verbose=0)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    np.random.seed(0)
    m.fit(src, tgt)
    assert len(log) == 1 and np.isfinite(log[0]) and log[0] > 0
    out, _ = m.predict(tgt)
    assert out.shape == (8935, 5) and torch.isfinite(out).all()
    assert m.ppmi_t.shape == (8935, 8935) and hasattr(m, "dmgnn") and not hasattr(m, "acdne")


def test_no_blas_product_on_the_dmgnn_path(monkeypatch):
    from bench import make_cfg_a
    src, tgt = make_cfg_a(seed=7, ns=1200, es=1800, nt=1000, et=1500)
    m = pygda_amd.models.DMGNN(src.x.size(1), 128, 5, device=DEV, epoch=2, verbose=0)
    calls = []

    def spy(name, fn):
        def wrapped(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapped

    for owner, attr in ((torch, "mm"), (torch, "matmul"), (torch.Tensor, "mm"), (torch.Tensor, "__matmul__"),
                        (F, "linear")):
        monkeypatch.setattr(owner, attr, spy(attr, getattr(owner, attr)))
    torch.manual_seed(0)
    m.fit(src, tgt)
    m.predict(tgt)
    torch.cuda.synchronize()
    assert calls == [], sorted(set(calls))
