"""KBL on the MI355X: the kernels of csrc/gda_kbl.hip against the float64 brute force of tests/test_kbl_host.py -- the
pair loss with its gradient (repeated indices, a zero row, identical and opposite rows, one class only; one pair, a
second row tile, a second feature block), the bridge top-k (one pair, a second row tile and a second column split, two
pairs that tie exactly, a NaN row, ``k`` above the kernel's cap) -- each float figure held by the project's bound against
torch-float32's own distance to float64 on the same inputs, the figures printed first; two runs bit-identical; the
refusals; device fits against the fixtures recorded from the reference's own kbl.py; eager and captured fits
bit-identical; one bridge epoch and one bridge generation at the ACMv9 -> DBLPv7 stand-in shapes."""
import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from tests.test_gpu_cwgcn import _close
from tests.test_kbl_host import (FIXTURES, GAP, PAIR_SHAPES, TOPK_SEEDS, TOPK_SHAPES, brute_bridge_topk, brute_pair_bce,
                                 check_fit_against_fixture, check_topk, fixture, pair_inputs, pair_yardstick, run_fit,
                                 topk_inputs)

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


def pair_run(u, ia, ib, y):
    v = u.to(DEV, torch.float32).requires_grad_(True)
    loss = ops.kbl_pair_bce(v, ia.to(DEV), ib.to(DEV), y.to(DEV))
    loss.backward()
    return loss.detach(), v.grad


@pytest.mark.parametrize("one_class", [False, True])
@pytest.mark.parametrize("shape", PAIR_SHAPES)
def test_pair_loss_and_gradient_against_float64(shape, one_class):
    u, ia, ib, y = pair_inputs(*shape, one_class=one_class)
    f64 = brute_pair_bce(u, ia, ib, y)
    f32 = pair_yardstick(u, ia, ib, y, torch.float32)
    gpu, again = pair_run(u, ia, ib, y), pair_run(u, ia, ib, y)
    tag = f"n={shape[0]} d={shape[1]} ma={shape[2]} mb={shape[3]} one_class={one_class}"
    assert same_bits(gpu[0], again[0]) and same_bits(gpu[1], again[1]), f"{tag}: two runs differ"
    assert bool(torch.isfinite(gpu[0])) and bool(torch.isfinite(gpu[1]).all()), f"{tag}: not finite"
    close(gpu[0], f32[0], f64[0], f"{tag} loss")
    rest = torch.ones(shape[0], dtype=torch.bool)
    if shape[0] >= 6:                                        # the zero row's gradient is g / 1e-8: 1e8 times the others'
        rest[1] = False
        close(gpu[1][1], f32[1][1], f64[1][1], f"{tag} dU, zero row")
    close(gpu[1].cpu()[rest], f32[1][rest], f64[1][rest], f"{tag} dU")
    named = torch.zeros(shape[0], dtype=torch.bool)
    named[ia], named[ib] = True, True
    assert bool((gpu[1].cpu()[~named] == 0).all())           # a node no list names: an exact zero row


def test_pair_loss_refuses_what_the_kernel_does_not_cover():
    u, ia, ib, y = (v.to(DEV) for v in pair_inputs(67, 20, 5, 9))
    with pytest.raises(_lib.GdaError, match="fp32"):
        ops.kbl_pair_bce(u, ia, ib, y)
    u = u.float()
    big = torch.zeros(ops.KBL_MAX_PAIR_ROWS + 1, dtype=torch.long, device=DEV)
    with pytest.raises(_lib.GdaError, match="gda_kbl_pair_bce_f32"):
        ops.kbl_pair_bce(u, big, ib, y)
    wide = torch.zeros(67, ops.KBL_MAX_WIDTH + 1, device=DEV)
    with pytest.raises(_lib.GdaError, match="gda_kbl_pair_bce_f32"):
        ops.kbl_pair_bce(wide, ia, ib, y)
    with pytest.raises(_lib.GdaError, match="expected"):
        ops.kbl_pair_bce(u, ia, ib, y[:5])


def topk_run(a, b, k):
    return ops.kbl_bridge_topk(a.to(DEV, torch.float32), b.to(DEV, torch.float32), k)


def by_pair(row, col, val, nb):
    order = torch.argsort(row.long().cpu() * nb + col.long().cpu())
    return val.cpu()[order]


@pytest.mark.parametrize("seed", TOPK_SEEDS)
@pytest.mark.parametrize("shape", TOPK_SHAPES)
def test_bridge_topk_against_float64(shape, seed):
    na, nb, d, k = shape
    a, b = topk_inputs(na, nb, d, seed)
    gpu, again = topk_run(a, b, k), topk_run(a, b, k)
    assert all(same_bits(x, y) for x, y in zip(gpu, again)), "two runs differ"
    assert gpu[0].dtype == torch.int32 and gpu[1].dtype == torch.int32
    row, col, val = check_topk(gpu, a, b, k, f"{shape} seed {seed}")
    f32 = ops.kbl_bridge_topk(a.float(), b.float(), k)                       # torch-float32 on the host: the yardstick
    close(by_pair(*gpu, nb), by_pair(*f32, nb), by_pair(row, col, val, nb), f"{shape} seed {seed} val")


@pytest.mark.parametrize("shape", TOPK_SHAPES[1:])
def test_bridge_topk_keeps_ties_in_flat_order_and_ranks_nan_first(shape):
    na, nb, d, k = shape
    a, b = topk_inputs(na, nb, d, variant="dup")
    row, col, val, gap = brute_bridge_topk(a, b, k)
    assert gap >= GAP and int(row[0]) == int(row[1]) and int(col[0]) < int(col[1])
    g = topk_run(a, b, k)
    check_topk(g, a, b, k, f"{shape} dup")
    assert g[0][:2].tolist() == row[:2].tolist() and g[1][:2].tolist() == col[:2].tolist()      # both, in flat-index order
    assert float(g[2][0]) == float(g[2][1])
    a, b = topk_inputs(na, nb, d, variant="nan")
    g = topk_run(a, b, k)
    m = min(k, nb)
    assert g[0][:m].tolist() == [0] * m and g[1][:m].tolist() == list(range(m)) and bool((g[2][:m] == 1).all())
    assert bool(torch.isfinite(g[2]).all()) and bool((g[2][1:] <= g[2][:-1]).all())


def test_bridge_topk_above_the_cap_takes_the_chunked_path():
    na, nb, d, _ = TOPK_SHAPES[3]
    k = ops.KBL_MAX_K + 44
    a, b = topk_inputs(na, nb, d)
    g = topk_run(a, b, k)
    assert g[0].dtype == torch.int64 and g[0].is_cuda
    check_topk(g, a, b, k, "k above the cap")
    with pytest.raises(_lib.GdaError, match="out of range"):
        topk_run(a, b, na * nb + 1)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.empty(k, dtype=torch.int32, device=DEV)
    status = _lib.lib().gda_kbl_bridge_topk_f32(a.to(DEV, torch.float32), b.to(DEV, torch.float32), na, nb, d, k, out, out,
                                                out.float(), ws, ws.numel(), None)
    assert status == -4                                                                        # GDA_E_UNSUPPORTED


@pytest.mark.parametrize("name", FIXTURES[:2])
def test_device_fit_agrees_with_the_fixture_recorded_from_the_reference(name):
    f, s, t = fixture(name)
    m, got = run_fit(f, s, t, DEV)
    check_fit_against_fixture(got, f)


@pytest.mark.parametrize("name", FIXTURES)                              # c: with the dropout of all three stages live
def test_eager_and_captured_fits_are_bit_identical(name):
    f, s, t = fixture(name)
    fits = []
    for graph in (False, True):
        ops.dropout_state.counter(torch.device(DEV)).zero_()   # the keep-bit stream restarts: the same masks
        fits.append(run_fit(f, s, t, DEV, use_hip_graph=graph, epochs_per_graph=2))
    (m1, eager), (m2, captured) = fits
    for k in eager:
        assert np.array_equal(eager[k], captured[k]), k
    for (k, v), w in zip(m1.kbl.state_dict().items(), m2.kbl.state_dict().values()):
        assert torch.equal(v, w), k
    assert np.isfinite(eager["logits"]).all() and np.isfinite(eager["stage1"]).all()
    if bool(f["live_dropout"]):                             # the masks are drawn: neither stage repeats the fit without
        g, _, _ = fixture(FIXTURES[0])
        assert np.abs(eager["stage1"][:, 0] - g["stage1"][:, 0]).max() > 1e-3
        assert np.abs(eager["losses"] - g["losses"]).max() > 1e-3


def test_one_bridge_epoch_and_one_bridge_generation_at_the_acm_dblp_shapes():
    from bench import make_cfg_a
    src, tgt = make_cfg_a(ns=7410, nt=5578)
    src.train_mask = torch.ones(7410, dtype=torch.bool)
    m = pygda_amd.models.KBL(src.x.size(1), 128, 5, k_cross=20, k_within=10, device=DEV, epoch=1, verbose=0,
                             bridge_epochs=1, use_hip_graph=False)
    torch.manual_seed(0)
    np.random.seed(0)
    m.fit(src, tgt)
    logits, _ = m.predict(tgt)
    assert len(m.bridge_log) == 1 and np.isfinite(m.bridge_log).all()
    row, col, val = m.bridge_edges
    assert row.shape == (20,) and int(row.max()) < 7410 and int(col.max()) < 5578 and bool(torch.isfinite(val).all())
    assert bool((val[1:] <= val[:-1]).all()) and len(set(zip(row.tolist(), col.tolist()))) == 20
    assert m.stored_data.x.shape[0] == 7410 + 5578 and logits.shape == (5578, 5) and bool(torch.isfinite(logits).all())
