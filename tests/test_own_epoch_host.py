"""The two refusals that ASN, JHGDA, SEPA and SOGA share (models/own_epoch.py), by exception type and full text."""
import pytest
import torch

import pygda_amd
from pygda_amd.data import Data

N, F_IN, C = 30, 8, 3
TRAINERS = {
    "ASN": lambda: pygda_amd.models.ASN(F_IN, 8, 4, C, device="cpu", epoch=1, verbose=0),
    "JHGDA": lambda: pygda_amd.models.JHGDA(F_IN, 8, C, num_layers=2, pool_ratio=0.5, device="cpu", epoch=1, verbose=0),
    "SEPA": lambda: pygda_amd.models.SEPA(F_IN, 8, C, device="cpu", epoch=1, verbose=0),
    "SOGA": lambda: pygda_amd.models.SOGA(F_IN, 8, C, device="cpu", epoch=1, verbose=0),
}


def _ring(seed, bad=False):
    g = torch.Generator().manual_seed(seed)
    src = torch.arange(N)
    ei = torch.stack([src, (src + 1) % N])
    if bad:
        ei[1, 0] = N                                          # one past the last node
    return Data(x=torch.randn(N, F_IN, generator=g), edge_index=ei, y=src % C)


@pytest.mark.parametrize("name", sorted(TRAINERS))
def test_an_edge_index_outside_the_graph_is_refused_with_the_trainers_name(name):
    m = TRAINERS[name]()
    with pytest.raises(ValueError) as err:
        m.fit(_ring(0), _ring(1, bad=True))
    assert type(err.value) is ValueError
    assert str(err.value) == f"{name}: edge_index refers to nodes outside [0, {N})"
    with pytest.raises(ValueError) as err:
        m.fit(_ring(0, bad=True), _ring(1))
    assert str(err.value) == f"{name}: edge_index refers to nodes outside [0, {N})"


@pytest.mark.parametrize("name", sorted(TRAINERS))
def test_a_data_parallel_run_is_refused_with_the_trainers_name(name, monkeypatch):
    monkeypatch.setattr(pygda_amd.distributed, "active", lambda: True)
    m = TRAINERS[name]()
    with pytest.raises(NotImplementedError) as err:
        m.fit(_ring(0), _ring(1))
    assert type(err.value) is NotImplementedError
    assert str(err.value) == f"{name}: data-parallel training is not supported"
