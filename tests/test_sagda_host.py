"""SAGDA without a GPU: the trainer's public surface (pygda/models/sagda.py), the module layout the golden state dicts
load into, argument validation of the FAConv entry points, the float64 restatement that arbitrates the GPU tests, and
the fixtures' regeneration from the reference."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pygda_amd
from pygda_amd import _lib
from tests.conftest import GOLDEN, T, load_golden


def test_sagda_signature_and_defaults():
    from pygda_amd.models import SAGDA
    sig = inspect.signature(SAGDA.__init__)
    want = dict(mode='node', beta=1.0, alpha=1.0, num_layers=2, dropout=0.0, act=F.relu, ppmi=True, adv_dim=40,
                weight_decay=3e-3, lr=4e-3, epoch=200, device='cuda:0', batch_size=0, num_neigh=-1, verbose=2)
    names = list(sig.parameters)
    assert names[:4] == ["self", "in_dim", "hid_dim", "num_classes"]
    assert names[4:-1] == list(want) and names[-1] == "kwargs"
    for k, v in want.items():
        assert sig.parameters[k].default == v, k


def test_sagda_rejects_what_it_does_not_run_without_a_device():
    from pygda_amd.models import SAGDA
    with pytest.raises(AssertionError):
        SAGDA(12, 8, 3, alpha=0.5)
    with pytest.raises(AssertionError):
        SAGDA(12, 8, 3, beta=0.5)
    with pytest.raises(NotImplementedError, match="sagda_base.py:322"):
        SAGDA(12, 8, 3, ppmi=False)
    with pytest.raises(NotImplementedError, match="mode='graph'"):
        SAGDA(12, 8, 3, mode='graph')
    with pytest.raises(NotImplementedError, match="sagda.py:264-270"):
        SAGDA(12, 8, 3, batch_size=16)
    with pytest.raises(ValueError, match="ppmi=True"):
        pygda_amd.nn.SAGDABase(12, 8, 3, ppmi=False)
    m = SAGDA(12, 8, 3)                    # the defaults build without a device
    assert (m.mode, m.ppmi, m.adv_dim, m.epoch, m.lr) == ('node', True, 40, 200, 4e-3)


def test_pygda_alias_resolves_sagda():
    import pygda
    from pygda.models import SAGDA
    from pygda.nn import SAGDABase
    assert SAGDA is pygda_amd.models.SAGDA and SAGDABase is pygda_amd.nn.SAGDABase
    assert "SAGDA" in pygda.__doc__


@pytest.mark.parametrize("layers", [1, 2])
def test_state_dict_keys_and_init_stream_match_the_reference(layers):
    """A fresh SAGDABase has the reference's state-dict keys, and from the reference's seed the same initial values:
    the init RNG stream is consumed in the same order (FAConv draws att_l, att_r, att_l, att_r before the layer's
    weight, which the source encoder shares)."""
    g = load_golden(f"sagda_fit3_l{layers}")
    init = {k[len("init/"):]: v for k, v in g.items() if k.startswith("init/")}
    torch.manual_seed(int(g["seed"]))
    net = pygda_amd.nn.SAGDABase(12, 8, 3, num_layers=layers, adv_dim=6)
    sd = net.state_dict()
    assert list(sd) == list(init)
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), init[k], err_msg=k)
    assert net.src_encoder.conv_layers[0].weight is net.encoder.conv_layers[0].weight
    assert net.src_encoder.conv_layers[-1].bias is net.ppmi_encoder.conv_layers[-1].bias
    assert net.models == [net.encoder, net.cls_model, net.domain_model, net.ppmi_encoder, net.att_model,
                          net.src_encoder]
    listed = [p for m in net.models for p in m.parameters()]
    assert sum(p is net.encoder.conv_layers[0].weight for p in listed) == 3      # three Adam rounds on the shared weight


def test_faconv_entry_points_validate_before_touching_a_device():
    L = _lib.lib()
    one = ctypes.c_void_p(1)
    fwd = lambda n, d, ldh, ldsr, ldo, p=one: L.gda_faconv_fwd_f32(p, one, one, n, d, one, ldh, one, one, ldsr,  # noqa
                                                                   0.1, None, ctypes.c_void_p(2), ldo, one, None)
    bwd = lambda n, d, ldh, ldgh, ldgsr, p=one: L.gda_faconv_bwd_f32(p, one, one, one, one, one, n, d, one, ldh,  # noqa
                                                                     one, ctypes.c_void_p(2), d, 0.1,
                                                                     ctypes.c_void_p(3), ldgh, one, one, ldgsr, one, None)
    assert fwd(10, 8, 8, 1, 8, p=None) == -1                     # NULL
    assert bwd(10, 8, 8, 8, 1, p=None) == -1
    assert fwd(-1, 8, 8, 1, 8) == -2 and fwd(10, -1, 8, 1, 8) == -2         # negative sizes
    assert bwd(-1, 8, 8, 8, 1) == -2 and bwd(10, -1, 8, 8, 1) == -2
    assert fwd(10, 8, 7, 1, 8) == -2 and fwd(10, 8, 8, 0, 8) == -2 and fwd(10, 8, 8, 1, 7) == -2   # ldh / ldsr / ldo
    assert bwd(10, 8, 7, 8, 1) == -2 and bwd(10, 8, 8, 7, 1) == -2 and bwd(10, 8, 8, 8, 0) == -2
    assert fwd(2 ** 31, 8, 8, 1, 8) == -2                        # int32 row indices
    assert L.gda_faconv_fwd_f32(one, one, one, 10, 8, one, 8, one, one, 1, 0.1, None, one, 8, one, None) == -5  # out == h
    assert fwd(0, 8, 8, 1, 8) == 0                               # nothing to do


@pytest.mark.parametrize("case", ["w12", "w8"])
def test_float64_loop_reproduces_faconv_fixture(case):
    """The per-node float64 restatement (tests/golden/_faconv_semantics.py, F1-F7) against what the reference's SAGNN
    path computed through the vectorised stand-in: output and the gradients of x, att_l and att_r."""
    from tests.golden._faconv_semantics import faconv_loop
    g = load_golden("faconv")
    ei = T(g[f"{case}/edge_index"])
    x = T(g[f"{case}/x"]).double().requires_grad_(True)
    al = T(g[f"{case}/att_l"]).double().requires_grad_(True)
    ar = T(g[f"{case}/att_r"]).double().requires_grad_(True)
    assert (ei[0] == ei[1]).any() and x.size(0) - 1 not in ei.tolist()[0] + ei.tolist()[1]   # loops; isolated last node
    out = faconv_loop(x, ei, al, ar, 0.1)
    out.backward(T(g[f"{case}/gy"]).double())
    for name, got in (("out", out), ("gx", x.grad), ("g_att_l", al.grad), ("g_att_r", ar.grad)):
        ref = g[f"{case}/{name}"].astype(np.float64)
        np.testing.assert_allclose(got.detach().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max(), err_msg=name)


def test_fixtures_regenerate_bit_for_bit(tmp_path):
    from tests.golden import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not available")
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "tests.golden.make_golden_sagda", "--out", str(tmp_path)], cwd=root,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("faconv", "sagda_fit3_l1", "sagda_fit3_l2"):
        a, b = np.load(os.path.join(GOLDEN, name + ".npz")), np.load(tmp_path / (name + ".npz"))
        assert a.files == b.files, name
        for k in a.files:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name}:{k}")
