"""Host: tests/_sampled_padding.py::poison_tail on a hand-built block with the attributes of
pygda_amd.sampled_graph._StaticBatch -- it rewrites the padding, all of it, and nothing else; and ``differences`` sees a
changed value but not the sign of a zero."""
from types import SimpleNamespace

import pytest
import torch

from tests._sampled_padding import POISON, VARIANTS, differences, hot_features, poison_tail

N_NODES, NCAP, ECAP, HOT = 50, 12, 20, 49
LIVE = (7, 9, 16, 3)                       # live rows, edges, CSR entries, interior rows
MARK_I, MARK_F = -1, 0.5                   # what the fake block's padding holds before: nothing poison_tail ever writes


def _block():
    g = torch.Generator().manual_seed(3)
    n, e, nnz, _ = LIVE
    cap = NCAP + ECAP
    rowptr = torch.cat([torch.tensor([0, 3, 5, 8, 10, 12, 14, 16]), torch.full((NCAP - n,), nnz)]).to(torch.int32)
    graph = SimpleNamespace(rowptr=rowptr, t_rowptr=rowptr.clone().flip(0).contiguous(),
                            colidx=torch.full((cap,), MARK_I, dtype=torch.int32), val=torch.full((cap,), MARK_F),
                            t_colidx=torch.full((cap,), MARK_I, dtype=torch.int32), t_val=torch.full((cap,), MARK_F))
    graph.colidx[:nnz] = torch.randint(0, n, (nnz,), generator=g).to(torch.int32)
    graph.t_colidx[:nnz] = torch.randint(0, n, (nnz,), generator=g).to(torch.int32)
    graph.val[:nnz] = torch.rand(nnz, generator=g)
    graph.t_val[:nnz] = torch.rand(nnz, generator=g)
    nodes = torch.full((NCAP,), MARK_I, dtype=torch.int64)
    nodes[:n] = torch.randperm(N_NODES - 1, generator=g)[:n]
    ei = torch.full((2, ECAP), MARK_I, dtype=torch.int64)
    ei[:, :e] = torch.randint(0, n, (2, e), generator=g)
    loader = SimpleNamespace(data=SimpleNamespace(x=torch.zeros(N_NODES, 4)))
    return SimpleNamespace(nodes=nodes, ei=ei, graph=graph, ncap=NCAP, live=LIVE, loader=loader,
                           counts=torch.tensor([n, e, nnz, 3] + [0] * 8, dtype=torch.int64))


def _parts(b):
    g = b.graph
    return dict(nodes=b.nodes, ei=b.ei, colidx=g.colidx, val=g.val, t_colidx=g.t_colidx, t_val=g.t_val,
                rowptr=g.rowptr, t_rowptr=g.t_rowptr, counts=b.counts)


def _tails(b):
    n, e, nnz, _ = LIVE
    g = b.graph
    return dict(nodes=b.nodes[n:], ei=b.ei[:, e:], colidx=g.colidx[nnz:], val=g.val[nnz:], t_colidx=g.t_colidx[nnz:],
                t_val=g.t_val[nnz:])


@pytest.mark.parametrize("variant", VARIANTS)
def test_poison_tail_rewrites_the_padding_and_nothing_else(variant):
    before = _block()
    b = poison_tail(_block(), variant, hot=HOT, seed=5)
    n, e, nnz, _ = LIVE
    was, now = _parts(before), _parts(b)
    for name in ("rowptr", "t_rowptr", "counts"):                        # never touched
        assert torch.equal(was[name], now[name]), name
    for name, live in (("nodes", n), ("colidx", nnz), ("val", nnz), ("t_colidx", nnz), ("t_val", nnz)):
        assert torch.equal(was[name][:live], now[name][:live]), name      # live prefixes, bit for bit
    assert torch.equal(before.ei[:, :e], b.ei[:, :e])
    tails = _tails(b)
    # every padded element was written (the marks are values no variant writes) ...
    for name in ("nodes", "ei", "colidx", "t_colidx"):
        assert not bool((tails[name] == MARK_I).any()), name
    for name in ("val", "t_val"):
        assert not bool((tails[name] == MARK_F).any()), name
        assert bool(torch.isfinite(tails[name]).all()) and float(tails[name].abs().max()) <= POISON
    # ... with ids in range
    assert 0 <= int(tails["nodes"].min()) and int(tails["nodes"].max()) < N_NODES
    for name in ("ei", "colidx", "t_colidx"):
        assert 0 <= int(tails[name].min()) and int(tails[name].max()) < NCAP, name
    if variant == "zero":
        assert all(float(t.double().abs().max()) == 0.0 for t in tails.values())
    if variant == "hot":
        assert bool((tails["nodes"] == HOT).all())
        assert bool((tails["colidx"] == n).all()) and bool((tails["ei"] == n).all())     # the first padded row
        assert tails["val"].tolist()[:4] == [POISON, -POISON, POISON, -POISON]
    if variant == "random":
        assert tails["nodes"].unique().numel() > 1 and tails["val"].unique().numel() > 2


def test_the_variants_differ_from_each_other_in_the_tail():
    tails = {v: _tails(poison_tail(_block(), v, hot=HOT, seed=5)) for v in VARIANTS}
    for a, b in (("zero", "random"), ("zero", "hot"), ("random", "hot")):
        for name in tails[a]:
            assert not torch.equal(tails[a][name], tails[b][name]), (a, b, name)


def test_poison_tail_refuses_what_is_out_of_range():
    with pytest.raises(ValueError):
        poison_tail(_block(), "hot", hot=N_NODES)
    with pytest.raises(ValueError):
        poison_tail(_block(), "nan")


def test_a_block_without_padding_is_left_alone():
    b = _block()
    b.live = (NCAP, ECAP, NCAP + ECAP, 3)
    was = {k: v.clone() for k, v in _parts(b).items()}
    poison_tail(b, "hot", hot=HOT)
    for k, v in _parts(b).items():
        assert torch.equal(was[k], v), k


def test_hot_features_alternate():
    assert hot_features(5).tolist() == [POISON, -POISON, POISON, -POISON, POISON]


def test_differences_compares_values_not_bit_patterns():
    run = lambda w, m: dict(loss=[1.5], correct=[3.0], param=[{"w": torch.tensor(w)}],
                            exp_avg=[{"w": torch.tensor(m)}], exp_avg_sq=[{"w": torch.tensor([0.0, 4.0])}])
    assert differences(run([1.0, 2.0], [0.0, 1.0]), run([1.0, 2.0], [-0.0, 1.0])) == []      # a zero of either sign
    d = differences(run([1.0, 2.0], [0.0, 1.0]), run([1.0, 2.0], [1e-30, 1.0]))
    assert len(d) == 1 and "exp_avg[w]" in d[0]
    other = run([1.0, 2.0], [0.0, 1.0])
    other["loss"] = [1.5000001]
    assert any("loss" in s for s in differences(run([1.0, 2.0], [0.0, 1.0]), other))
