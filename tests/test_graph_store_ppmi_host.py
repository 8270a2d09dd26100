"""CPU: the ``ppmi`` keyword of ``pygda_amd.data.GraphStore`` -- accepted, validated, ``"per_batch"`` by default,
``"per_graph"`` refused on a CPU store -- and the argument checks of the two entry points behind ``"per_graph"``
(csrc/gda_collate.hip ``gda_collate_ppmi_f32``, csrc/gda_ppmi_dev.hip ``gda_ppmi_build_ratio``), which come before
anything touches a device.  What the mode computes is tested in tests/test_gpu_graph_store_ppmi.py."""
import ctypes

import pytest
import torch

from pygda_amd import _lib
from pygda_amd.data import Data, GraphStore

NULL, SIZE, UNSUPPORTED, ALIAS = -1, -2, -4, -5


def _graphs():
    return [Data(x=torch.ones(3, 4), edge_index=torch.tensor([[0, 1], [1, 2]]), y=torch.tensor([i % 2])) for i in range(3)]


def test_the_default_is_per_batch_and_the_keyword_is_kept():
    assert GraphStore(_graphs(), "cpu").ppmi == "per_batch"
    assert GraphStore(_graphs(), "cpu", ppmi="per_batch").ppmi == "per_batch"
    assert GraphStore(_graphs(), "cpu", "per_batch").ppmi == "per_batch"
    assert GraphStore([], "cpu").ppmi == "per_batch"


@pytest.mark.parametrize("bad", ["per_layer", "", None, True, 0, "PER_GRAPH"])
def test_any_other_mode_is_refused(bad):
    with pytest.raises(ValueError, match="ppmi"):
        GraphStore(_graphs(), "cpu", ppmi=bad)


def test_per_graph_on_a_cpu_store_is_refused_and_names_the_device():
    with pytest.raises(ValueError, match="cpu"):
        GraphStore(_graphs(), "cpu", ppmi="per_graph")
    with pytest.raises(ValueError, match="cpu"):
        GraphStore(_graphs(), torch.device("cpu"), ppmi="per_graph")


def test_a_per_batch_store_has_no_stored_pairs():
    with pytest.raises(ValueError, match="per_batch"):
        GraphStore(_graphs(), "cpu").ppmi_pairs(object())


# --------------------------------------------------------------------------------------------------- ABI --
def P(addr):
    return ctypes.c_void_p(addr)


# distinct non-NULL dummies: validation comes first, nothing is dereferenced
IDS, PPTR, POFF, SEG, LS, LD, RATIO, OUT, W = (P(0x1000 * k) for k in range(1, 10))


def collate_ppmi(ids=IDS, B=4, G=9, pair_ptr=PPTR, pair_off=POFF, seg=SEG, ls=LS, ld=LD, ratio=RATIO, P_total=50,
                 targets=7, path_len=5, m=30, out=OUT, w=W):
    return _lib.lib().gda_collate_ppmi_f32(ids, B, G, pair_ptr, pair_off, seg, ls, ld, ratio, P_total, targets, path_len, m,
                                           out, w, None)


def test_the_pair_collation_validates_its_arguments():
    for missing in ("ids", "pair_ptr", "pair_off", "seg", "ls", "ld", "ratio", "out", "w"):
        assert collate_ppmi(**{missing: None}) == NULL, missing
    for bad in (dict(B=-1), dict(G=-1), dict(P_total=-1), dict(m=-1), dict(targets=-1), dict(path_len=0),
                dict(P_total=0, m=1)):
        assert collate_ppmi(**bad) == SIZE, bad
    for other in (IDS, PPTR, POFF, SEG, LS, LD, RATIO):
        assert collate_ppmi(out=other) == ALIAS
    for other in (OUT, LS, LD, RATIO):
        assert collate_ppmi(w=other) == ALIAS


def test_an_empty_pair_list_launches_nothing_and_looks_at_no_operand():
    none = dict(ids=None, pair_ptr=None, pair_off=None, seg=None, ls=None, ld=None, ratio=None, out=None, w=None)
    assert collate_ppmi(B=0, m=0, **none) == 0
    assert collate_ppmi(m=0, **none) == 0                       # a batch of graphs without a pair: no log is evaluated
    assert collate_ppmi(m=0, P_total=0, targets=0, **none) == 0


def test_the_ratio_builder_has_the_limits_and_checks_of_the_weight_builder():
    L = _lib.lib()
    one = P(1)

    def both(*args):
        got = {getattr(L, name)(*args) for name in ("gda_ppmi_build", "gda_ppmi_build_ratio")}
        assert len(got) == 1, got
        return got.pop()

    args = lambda E=10, N=5, path_len=5, passes=40, src=one, dst=one, o_src=one, o_dst=one, o_val=one, count=one, ws=one, nbytes=1 << 40: \
        (src, dst, E, N, path_len, passes, 3, o_src, o_dst, o_val, count, ws, nbytes, None)
    assert both(*args(E=-1)) == SIZE and both(*args(N=-1)) == SIZE and both(*args(path_len=0)) == SIZE and both(*args(passes=0)) == SIZE
    assert both(*args(E=2 ** 30)) == UNSUPPORTED and both(*args(N=2 ** 24, path_len=10)) == UNSUPPORTED
    assert L.gda_ppmi_workspace_bytes(2 ** 30, 5, 5, 40) == 0 and L.gda_ppmi_workspace_bytes(10, 2 ** 24, 10, 40) == 0
    for missing in ("src", "dst", "o_src", "o_dst", "o_val", "count", "ws"):
        assert both(*args(**{missing: None})) == NULL, missing
    assert both(*args(nbytes=16)) == -3                            # workspace too small
