"""CPU: the host side of the one-pass MMD that reads the target's column-major pre-activation (ops.MMD_ACT_CM): the shape
list of tests/test_gpu_mmd_act_cm.py reaches every segment count the scatter kernel is instantiated for, and the envelope
predicate refuses what the entry points refuse."""
import torch

from pygda_amd import _lib, ops

# (times, n, d) -> nseg, the op-level cases of tests/test_gpu_mmd_act_cm.py
CASES = [((1, 16, 32), 1), ((1, 20, 32), 2), ((1, 40, 64), 3), ((5, 64, 128), 4), ((2, 70, 128), 5), ((2, 90, 96), 6),
         ((3, 100, 64), 7), ((1, 130, 32), 8)]


def test_shape_list_reaches_every_segment_count():
    L = _lib.lib()
    got = [int(L.gda_mmd_fused_nseg(times, n, d, 2.0, 5)) for (times, n, d), _ in CASES]
    assert got == [nseg for _, nseg in CASES]
    assert sorted(got) == list(range(1, 9))
    # the benchmark's shape
    assert int(L.gda_mmd_fused_nseg(5, 1000, 128, 2.0, 5)) == 6


def test_envelope_predicate():
    sel = tuple(torch.zeros(4, dtype=torch.int32) for _ in range(4)) + (torch.ones(4),)
    a = torch.zeros(64)
    base = a.data_ptr()
    assert base % 16 == 0
    for (times, n, d), _ in CASES:
        assert ops.mmd_act_cm_ok(times, n, d, sel, (base, base + 16), (n + 4 - n % 4 if n % 4 else n,))
    assert ops.mmd_act_cm_ok(5, 1000, 128, sel, (base,), (5580,))
    assert not ops.mmd_act_cm_ok(5, 1000, 100, sel, (base,))                      # not a width of the register kernel
    assert not ops.mmd_act_cm_ok(5, 1000, 160, sel, (base,))
    assert not ops.mmd_act_cm_ok(5, 1000, 128, None, (base,))                     # no selection CSRs: no scatter
    assert not ops.mmd_act_cm_ok(5, 1000, 128, (sel[0], None, sel[2], sel[3], sel[4]), (base,))
    assert not ops.mmd_act_cm_ok(5, 1000, 128, sel, (base, a[1:].data_ptr()))     # an operand off the 16-byte grid
    assert not ops.mmd_act_cm_ok(5, 1000, 128, sel, (base,), (5578,))             # a leading dimension that is no quad
    assert not ops.mmd_act_cm_ok(5, 1000, 128, sel, (base,), fix_sigma=1.0)       # the fused pass has no fixed bandwidth
    assert not ops.mmd_act_cm_ok(5, 1000, 128, sel, (base,), kernel_num=3)


def test_flag_off_refuses(monkeypatch):
    sel = tuple(torch.zeros(4, dtype=torch.int32) for _ in range(4))
    monkeypatch.setattr(ops, "MMD_ACT_CM", False)
    assert not ops.mmd_act_cm_ok(5, 1000, 128, sel)
