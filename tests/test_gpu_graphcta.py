"""GraphCTA on the MI355X: the kernels of csrc/gda_graphcta.hip against the float64 brute force of
tests/test_graphcta_host.py -- the model loss with both gradients (a zero feature row, a zero prototype, one row, a
second row tile and a second column split), the per-row top-(K + 1) on the rows whose ranks float64 decides, the
test-time loss with float64's neighbours fed in (the selected set equal to the host's, a class whose share rounds to no
row, no selected row at all, a one-class memory) -- each held by the project's bound against torch-float32's own distance
to float64 on the same inputs, the figures printed first; two runs bit-identical; the fits against the fixtures recorded
from the reference's own graphcta.py; eager and captured fits bit-identical; one iteration at the ACMv9 -> DBLPv7
stand-in shapes."""
import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from tests.test_gpu_cwgcn import _close
from tests.test_graphcta_host import (FIXTURES, KNN_SHAPES, check_fit_against_fixture, fixture, run_fit, brute_knn, brute_model_loss, brute_test_time, grads, knn_decided,
                                      knn_inputs, model_inputs, tt_decided, tt_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(gpu, f32, f64, name, slack=2e-6):
    """|gpu - f64| <= 8 |fp32 torch - f64| + 2e-6 max|f64| (NaN where float64 has NaN), the figures printed first."""
    a, b, c = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64) for v in (gpu, f32, f64))
    with np.errstate(invalid="ignore"):
        print(f"{name}: |gpu - f64| = {np.nanmax(np.abs(a - c), initial=0):.3e}, |fp32 torch - f64| = "
              f"{np.nanmax(np.abs(b - c), initial=0):.3e}, max|f64| = {np.nanmax(np.abs(c), initial=0):.3e}")
    _close(gpu, f32, f64, name, slack)


def same_bits(a, b):
    """Equal bit for bit, a NaN against the same NaN included."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def model_run(inputs, dtype, dev, tau, lamb, fn=ops.cta_model_loss):
    feat, logits, proto, pred = inputs
    x, y = feat.to(dev, dtype).requires_grad_(True), logits.to(dev, dtype).requires_grad_(True)
    res = fn(x, y, proto.to(dev, dtype), pred.to(dev), tau, lamb)
    parts = res[1] if fn is ops.cta_model_loss else torch.stack(res)
    return [parts.detach()] + list(grads(res[0], x, y))


@pytest.mark.parametrize("n", [1, 67, 300])
@pytest.mark.parametrize("d", [4, 20, 128, 256])
def test_model_loss_and_both_gradients_against_float64(n, d):
    for c, (tau, lamb) in zip((2, 5, 64), ((0.2, 0.2), (0.5, 0.5), (0.2, 0.2))):
        inputs = model_inputs(n, d, c)
        f64 = model_run(inputs, torch.float64, "cpu", tau, lamb, brute_model_loss)
        f32 = model_run(inputs, torch.float32, "cpu", tau, lamb)
        gpu = model_run(inputs, torch.float32, DEV, tau, lamb)
        again = model_run(inputs, torch.float32, DEV, tau, lamb)
        tag = f"N={n} d={d} C={c}"
        assert all(torch.equal(a, b) for a, b in zip(gpu, again)), f"{tag}: two runs differ"
        assert all(bool(torch.isfinite(v).all()) for v in gpu), f"{tag}: not finite"
        close(gpu[0], f32[0], f64[0], f"{tag} out")
        rest = torch.ones(n, dtype=torch.bool)
        if n >= 3:                                           # the zero row's gradient is 1e12 times the others'
            rest[1] = False
            close(gpu[1][1], f32[1][1], f64[1][1], f"{tag} dfeat, zero row")
        close(gpu[1].cpu()[rest], f32[1][rest], f64[1][rest], f"{tag} dfeat")
        close(gpu[2], f32[2], f64[2], f"{tag} dlogits")


def test_model_loss_refuses_what_the_kernels_do_not_cover():
    feat, logits, proto, pred = (v.to(DEV) for v in model_inputs(67, 4, 5))
    with pytest.raises(_lib.GdaError, match="fp32"):
        ops.cta_model_loss(feat, logits, proto, pred)
    wide = torch.zeros(67, 260, device=DEV)
    with pytest.raises(_lib.GdaError, match="widths up to 256"):
        ops.cta_model_loss(wide, logits.float(), torch.zeros(5, 260, device=DEV), pred)


@pytest.mark.parametrize("n,d,k1", KNN_SHAPES)
def test_knn_on_the_rows_float64_decides(n, d, k1):
    feat, mem = knn_inputs(n, d, k1)
    decided = knn_decided(feat, mem, k1)
    assert int((~decided).sum()) <= n // 100
    bi, bv = brute_knn(feat, mem, k1)
    v32 = torch.topk(feat.float() @ mem.float().t(), k1, dim=1).values
    idx, val = ops.cta_knn(feat.to(DEV, torch.float32), mem.to(DEV, torch.float32), k1)
    idx2, val2 = ops.cta_knn(feat.to(DEV, torch.float32), mem.to(DEV, torch.float32), k1)
    assert idx.dtype == torch.int32 and torch.equal(idx, idx2) and torch.equal(val, val2)
    assert bool((val[:, :-1] >= val[:, 1:]).all()) and int(idx.min()) >= 0 and int(idx.max()) < n
    got = np.sort(idx.cpu().numpy()[:, 1:], axis=1)[decided.numpy()]
    want = np.sort(bi.numpy()[:, 1:], axis=1)[decided.numpy()]
    assert np.array_equal(got, want), f"{int((got != want).any(axis=1).sum())} decided rows differ"
    assert np.array_equal(idx.cpu().numpy()[decided.numpy(), 0], bi.numpy()[decided.numpy(), 0])
    close(val, v32, bv, f"N={n} d={d} K1={k1} values")


def test_knn_ties_go_to_the_lower_index_and_too_few_rows_raise():
    feat = torch.tensor([[1.0, 0.0], [0.0, 1.0]], device=DEV)
    mem = torch.tensor([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0]], device=DEV)
    idx, val = ops.cta_knn(feat, mem, 3)
    assert idx.tolist() == [[0, 1, 3], [2, 0, 1]] and val.tolist() == [[1, 1, 1], [1, 0, 0]]
    big = torch.ones(70, 3, device=DEV)                                  # every product equal, across two column tiles
    idx, _ = ops.cta_knn(big, torch.ones(200, 3, device=DEV), 16)
    assert torch.equal(idx.cpu(), torch.arange(16, dtype=torch.int32).expand(70, 16))
    with pytest.raises(_lib.GdaError, match="out of range"):
        ops.cta_knn(feat, mem, 5)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    out = torch.empty(64, device=DEV)
    assert _lib.lib().gda_cta_knn_f32(_lib.ptr(feat), _lib.ptr(mem), 2, 4, 2, 5, _lib.ptr(out), _lib.ptr(out),
                                      _lib.ptr(ws), ws.numel(), None) == -2          # GDA_E_SIZE: Nm < K1


def tt_run(inputs, dtype, dev, fn=ops.cta_test_time_loss):
    logits, feat, mem_fea, mem_cls, idx_near = inputs
    x, y = logits.to(dev, dtype).requires_grad_(True), feat.to(dev, dtype).requires_grad_(True)
    res = fn(x, y, mem_fea.to(dev, dtype), mem_cls.to(dev, dtype), idx_near.to(dev))
    if fn is ops.cta_test_time_loss:
        loss, parts, pred, sel = res
    else:
        loss, parts, pred, sel = res[0], torch.stack(res[:4]), res[4], res[5]
    g = grads(loss, x, y) if bool(torch.isfinite(loss)) else (torch.zeros_like(x), torch.zeros_like(y))
    return [parts.detach(), g[0], g[1], pred.cpu().long(), sel.cpu().bool()]


TT_CASES = [(n, d, k1, (2, 5, 64)[i % 3], False) for i, (n, d, k1) in enumerate(KNN_SHAPES)] + [(67, 4, 6, 5, True)]


@pytest.mark.parametrize("n,d,k1,c,rare", TT_CASES)
def test_test_time_loss_and_both_gradients_against_float64(n, d, k1, c, rare):
    inputs = tt_inputs(n, d, c, k1, rare_class=rare)
    assert tt_decided(inputs[0], inputs[3])
    f64 = tt_run(inputs, torch.float64, "cpu", brute_test_time)
    host = tt_run(inputs, torch.float64, "cpu")
    f32 = tt_run(inputs, torch.float32, "cpu")
    gpu = tt_run(inputs, torch.float32, DEV)
    again = tt_run(inputs, torch.float32, DEV)
    tag = f"N={n} d={d} K1={k1} C={c}"
    assert all(same_bits(a, b) for a, b in zip(gpu, again)), f"{tag}: two runs differ"
    assert torch.equal(gpu[3], f64[3]) and torch.equal(gpu[4], host[4]) and torch.equal(host[4], f64[4])
    if rare:
        assert int((gpu[3] == 0).sum()) == 3 and not bool(gpu[4][gpu[3] == 0].any()) and bool(gpu[4].any())
    close(gpu[0], f32[0], f64[0], f"{tag} out")
    close(gpu[1], f32[1], f64[1], f"{tag} dlogits")
    close(gpu[2], f32[2], f64[2], f"{tag} dfeat")


def test_one_class_memory_gives_nan_on_the_device_too():
    logits, feat, mem_fea, mem_cls, idx_near = tt_inputs(67, 4, 5, 6)
    mem_cls = torch.zeros_like(mem_cls)
    mem_cls[:, 2] = 1
    _, parts, pred, _ = ops.cta_test_time_loss(logits.to(DEV, torch.float32), feat.to(DEV, torch.float32),
                                               mem_fea.to(DEV, torch.float32), mem_cls.to(DEV, torch.float32),
                                               idx_near.to(DEV))
    assert bool((pred == 2).any()) and bool(torch.isnan(parts[3])) and bool(torch.isfinite(parts[1:3]).all())


@pytest.mark.parametrize("name", FIXTURES)
def test_device_fit_agrees_with_the_fixture_recorded_from_the_reference(name):
    f, s, t = fixture(name)
    m, got = run_fit(f, s, t, DEV)
    assert float(np.abs(got["p_iter"] - 1e-7).max()) < 1e-12
    check_fit_against_fixture(got, f)


@pytest.mark.parametrize("name", FIXTURES[1:])                          # make_undirected False (b) and True (c)
@pytest.mark.parametrize("stepped", [False, True])
def test_eager_and_captured_fits_are_bit_identical(stepped, name):
    f, s, t = fixture(name)
    kw = dict(step_structure=stepped, epochs_per_graph=2)
    _, eager = run_fit(f, s, t, DEV, use_hip_graph=False, **kw)
    _, captured = run_fit(f, s, t, DEV, use_hip_graph=True, **kw)
    for k in eager:
        assert np.array_equal(eager[k], captured[k]), k
    assert np.isfinite(eager["logits"]).all() and np.isfinite(eager["steps"]).all() and len(eager["steps"]) == 12 + 20
    if not stepped:
        assert str(eager["stopped"]) == str(f["stopped"])
    if stepped:
        assert (eager["p_iter"][-1] > 1e-6).sum() > 0
        k = int(0.1 * f["tgt_ei"].shape[1] // 2)
        assert np.clip(eager["p_iter"], 0, 1).sum(1).max() <= k + 1e-5 * eager["p_iter"].shape[1]


def test_one_iteration_at_the_acm_dblp_shapes():
    from bench import make_cfg_a
    src, tgt = make_cfg_a()
    m = pygda_amd.models.GraphCTA(src.x.size(1), 128, 5, device=DEV, epoch=5, verbose=0, record=True)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    np.random.seed(0)
    m.fit(src, tgt)
    logits, _ = m.predict(tgt)
    assert len(log) == 5 + 1 and all(np.isfinite(v) for v in log)
    assert len(m.model_log) == 3 and np.isfinite(m.model_log).all()
    assert len(m.parts_log) == 5 + 20 and np.isfinite(m.parts_log).all()
    assert logits.shape == (5484, 5) and torch.isfinite(logits).all()
