"""GPU: graph-mode batches collated on the device out of a ``GraphStore`` (csrc/gda_collate.hip) are, bit for bit, the
host collation moved to the device; their normalised graphs are the ones ``build_csr`` makes of the collated edge list;
every graph-mode trainer reaches the same weights from stores as from lists; drawing a batch never waits for the
device."""
import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import ops
from pygda_amd.data import Data, DataLoader, GraphStore, StoreLoader, _collate
from pygda_amd.graph import as_graph, build_csr
from tests.conftest import load_golden, sub
from tests.test_gpu_cwgcn import _check_golden, _graphs
from tests.test_gpu_graph_mode import _dataset, _gt_trainer, _zero_dropouts
from tests.test_gpu_parity import DEV, LOGIT_ATOL, REL, close, exact

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 10, 130]
VARIANTS = [(False, True, True, "col"), (False, True, True, "row"), (True, True, True, "col"),
            (False, False, False, "col"), (False, "drop", True, "row")]


def make_graph(n, e, seed, undirected=True, self_loops=0, dups=0, isolated=True):
    """The edge cases gcn_norm must handle (as the golden scripts build them): self loops, duplicate and one-directional
    edges, an isolated last node; no edge at all where the graph leaves no room for one."""
    g = torch.Generator().manual_seed(seed)
    hi = n - 1 if isolated else n
    if hi <= 0 or e == 0:
        return torch.empty(2, 0, dtype=torch.long)
    src, dst = torch.randint(0, hi, (e,), generator=g), torch.randint(0, hi, (e,), generator=g)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    if undirected:
        src, dst = torch.cat([src, dst]), torch.cat([dst, src])
    if dups:
        src, dst = torch.cat([src, src[:dups]]), torch.cat([dst, dst[:dups]])
    if self_loops:
        l = torch.randint(0, hi, (self_loops,), generator=g)
        src, dst = torch.cat([src, l]), torch.cat([dst, l])
    perm = torch.randperm(src.numel(), generator=g)
    return torch.stack([src[perm], dst[perm]]).long()


# (nodes, edges drawn, make_graph options): 0, 1, 2, 63, 64, 65 and ~300 nodes; graphs 1 and 9 are empty, 5 and 10 have
# nodes but no edge, 2 is one node with nothing but self loops
SHAPES = [(5, 6, {}), (0, 0, {}), (1, 2, dict(isolated=False, self_loops=2)), (2, 3, dict(isolated=False, dups=1)),
          (63, 90, dict(self_loops=3, dups=4)), (64, 0, {}), (65, 120, dict(undirected=False, self_loops=2)),
          (300, 700, dict(self_loops=5, dups=9)), (1, 0, {}), (0, 0, {}), (17, 0, {}), (2, 2, dict(self_loops=1)),
          (64, 100, dict(undirected=False, dups=5, isolated=False))]
ID_LISTS = {"single": [7], "identity": list(range(len(SHAPES))), "permutation": [4, 12, 0, 9, 7, 2, 11, 1, 6, 3, 10, 8, 5],
            "subset_descending": [11, 7, 6, 4, 2], "empty_first_and_last": [1, 6, 10, 3, 9]}


def _graphs_of(shapes, F, seed):
    g = torch.Generator().manual_seed(seed)
    return [Data(x=torch.randn(n, F, generator=g), edge_index=make_graph(n, e, seed + 31 * i, **kw),
                 y=torch.tensor([i % 4])) for i, (n, e, kw) in enumerate(shapes)]


_cache = {}


def _case(F, name):
    """``(store, graphs, ids, host collation on the device)``, built once per width and shared."""
    if ("data", F) not in _cache:
        small = _graphs_of(SHAPES, F, 100 + F)
        # 1,500 graphs of 1 to 3 nodes: more chosen graphs than any one workgroup scans in a single pass
        many = _graphs_of([(1 + i % 3, i % 4, dict(isolated=False, self_loops=i % 2)) for i in range(1500)], F, 200 + F)
        _cache["data", F] = {"small": (small, GraphStore(small, DEV)), "many": (many, GraphStore(many, DEV))}
    if (F, name) not in _cache:
        graphs, store = _cache["data", F]["many" if name == "many" else "small"]
        ids = torch.randperm(1500, generator=torch.Generator().manual_seed(3)).tolist() if name == "many" else ID_LISTS[name]
        ref = _collate([graphs[i] for i in ids]).to(DEV)
        _cache[F, name] = (store, graphs, ids, ref)
    return _cache[F, name]


@pytest.mark.parametrize("name", [*ID_LISTS, "many"])
@pytest.mark.parametrize("F", WIDTHS)
def test_device_collation_is_the_host_collation(F, name):
    store, graphs, ids, ref = _case(F, name)
    got = store.batch(ids)
    assert got.x.is_cuda and got.x.dtype == torch.float32 and got.edge_index.dtype == torch.long
    for k in ("x", "edge_index", "y", "batch"):
        assert getattr(got, k).shape == getattr(ref, k).shape, k
        assert torch.equal(getattr(got, k), getattr(ref, k)), k
    assert got.num_graphs == ref.num_graphs == len(ids)
    assert got.batch._gda_sorted is True and got.batch._gda_num_graphs == ref.batch._gda_num_graphs == len(ids)
    want_seg = ops.segment_ptr(ref.batch, len(ids))
    assert got.batch._gda_seg_ptr.dtype == want_seg.dtype and torch.equal(got.batch._gda_seg_ptr, want_seg)
    assert ops.segment_ptr(got.batch, len(ids)) is got.batch._gda_seg_ptr           # the readout takes it as it is
    moved = got.to(DEV)
    assert moved is got and moved.batch._gda_seg_ptr is got.batch._gda_seg_ptr


@pytest.mark.parametrize("name", [*ID_LISTS, "many"])
@pytest.mark.parametrize("F", [4, 3])
def test_batch_graphs_are_the_builds_of_the_collated_edges(F, name):
    store, graphs, ids, ref = _case(F, name)
    n = ref.x.size(0)
    for variant in VARIANTS:
        want = build_csr(ref.edge_index, n, None, *variant)
        nnz = want.nnz
        assert int(want.t_rowptr[n]) == nnz
        runs = []
        for _ in range(2):
            batch = store.batch(ids)
            g = as_graph(batch.edge_index, n, None, *variant)
            assert as_graph(batch.edge_index, n, None, *variant) is g                # one graph per (batch, variant)
            assert g.num_nodes == n and g.nnz == nnz and (g.static, g.transient) == (want.static, want.transient)
            runs.append(g)
        for g in runs:
            for a in ("rowptr", "t_rowptr"):
                assert torch.equal(getattr(g, a), getattr(want, a)), (variant, a)
            for a in ("colidx", "val", "t_colidx", "t_val"):
                assert torch.equal(getattr(g, a)[:nnz], getattr(want, a)[:nnz]), (variant, a)
        assert store.nnz_counts(*variant)[torch.tensor(ids)].sum() == nnz
    # anything the store does not hold falls through to the present build, on a correct edge list
    batch = store.batch(ids)
    w = torch.rand(batch.edge_index.size(1), device=DEV)
    weighted, want = as_graph(batch.edge_index, n, w), build_csr(ref.edge_index, n, w)
    assert torch.equal(weighted.rowptr, want.rowptr) and torch.equal(weighted.val[:want.nnz], want.val[:want.nnz])


def test_long_rows_are_laid_out_as_for_a_fresh_build():
    """A batch graph out of a store without a row beyond the long-row limit carries the no-hub layout ready-made; one
    with a hub (a 300-leaf star: a row of 301 entries) leaves it to the first aggregation, as a fresh build does.  The
    aggregations agree bit for bit either way, in both orientations."""
    hub = torch.arange(1, 301)
    star = Data(x=torch.randn(301, 8), edge_index=torch.stack([torch.cat([hub, 0 * hub]), torch.cat([0 * hub, hub])]),
                y=torch.tensor([1]))
    plain = _case(4, "identity")[1]
    for graphs, F, hubs in (([g for g in plain if g.x.size(0) < 100], 4, False),
                            ([Data(x=torch.randn(9, 8), edge_index=make_graph(9, 20, 5), y=torch.tensor([0])), star], 8, True)):
        store = GraphStore(graphs, DEV)
        ids = list(range(len(graphs)))[::-1]
        ref = _collate([graphs[i] for i in ids]).to(DEV)
        n = ref.x.size(0)
        g, want = as_graph(store.batch(ids).edge_index, n), build_csr(ref.edge_index, n)
        assert (g._split is None, g._t_split is None) == (hubs, hubs)
        x = torch.randn(n, F, device=DEV)
        for transposed in (False, True):
            assert torch.equal(ops.spmm_kstep(g, x, 2, transposed=transposed), ops.spmm_kstep(want, x, 2, transposed=transposed))
        assert (g.split().n_long, g.split(True).n_long) == (want.split().n_long, want.split(True).n_long) == (int(hubs),) * 2


# ---------------------------------------------------------------------------------------------- trainers --
def _wrap(stores, src, tgt):
    return (GraphStore(src, DEV), GraphStore(tgt, DEV)) if stores else (src, tgt)


def _fit_pair(make, net_of, seed, src, tgt):
    """The same fit from lists and from stores: ``[(trainer, per-epoch log, predict)]``, lists first."""
    runs = []
    for stores in (False, True):
        m = make()
        seen = []
        m.epoch_hook = lambda e, loss, acc, secs: seen.append((float(loss), acc))
        torch.manual_seed(seed)
        s, t = _wrap(stores, src, tgt)
        m.fit(s, t)
        runs.append((m, seen, m.predict(t)))
    (ml, logl, (pl, yl)), (ms, logs, (ps, ys)) = runs
    assert logs == logl and len(logs) >= 3
    for (k, a), b in zip(net_of(ml).state_dict().items(), net_of(ms).state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(pl, ps) and torch.equal(yl, ys)
    return runs[1]


@pytest.mark.parametrize("batch_size", [0, 6])
def test_a2gnn_from_stores_equals_lists_and_meets_the_golden(batch_size):
    g = load_golden(f"a2gnn_graph_fit3_b{batch_size}")
    make = lambda: pygda_amd.models.A2GNN(10, 16, 3, mode='graph', num_layers=2, dropout=0.0, s_pnums=0, t_pnums=5,
                                          weight=0.5, lr=0.01, weight_decay=0.001, device=DEV, epoch=3, verbose=0,
                                          batch_size=batch_size)
    m, seen, (logits, labels) = _fit_pair(make, lambda m: m.a2gnn, int(g["seed"]), _dataset(g, "src"), _dataset(g, "tgt"))
    close([x[0] for x in seen], g["losses"], rtol=REL)
    close([x[1] for x in seen], g["accs"], rtol=0, atol=1e-12)
    for k, v in sub(g, "final/").items():
        close(m.a2gnn.state_dict()[k], v, rtol=1e-3, atol=2e-4)
    if batch_size == 0:
        close(logits, g["tgt_logits"], rtol=0, atol=LOGIT_ATOL)
        exact(labels, g["tgt_labels"])
        exact(logits.argmax(1), g["tgt_logits"].argmax(1))


@pytest.mark.parametrize("batch_size", [0, 6])
@pytest.mark.parametrize("tag", ["grade_js", "grade_mmd", "udagcn", "adagcn", "dane"])
def test_graph_trainers_from_stores_equal_lists_and_meet_the_golden(monkeypatch, tag, batch_size):
    _zero_dropouts(monkeypatch)
    g = load_golden("graph_trainers")
    attr = _gt_trainer(tag)[1]
    m, seen, (logits, labels) = _fit_pair(lambda: _gt_trainer(tag, batch_size=batch_size)[0], lambda m: getattr(m, attr),
                                          int(g["fit_seed"]), _dataset(g, "src"), _dataset(g, "tgt"))
    close([x[0] for x in seen], g[f"{tag}/fit{batch_size}/losses"], rtol=REL)
    close([x[1] for x in seen], g[f"{tag}/fit{batch_size}/accs"], rtol=0, atol=1e-12)
    for k, v in sub(g, f"{tag}/fit{batch_size}/final/").items():
        close(getattr(m, attr).state_dict()[k], v, rtol=1e-3, atol=2e-4)
    if batch_size == 0:
        close(logits, g[f"{tag}/fit0/tgt_logits"], rtol=0, atol=LOGIT_ATOL)
        exact(labels, g[f"{tag}/fit0/tgt_labels"])
        exact(logits.argmax(1), g[f"{tag}/fit0/tgt_logits"].argmax(1))


@pytest.mark.parametrize("batch_size", [0, 6])
def test_cwgcn_from_stores_equals_lists_and_meets_the_golden(batch_size):
    g = load_golden(f"cwgcn_graph_fit3_b{batch_size}")
    assert int(g["batch_size"]) == batch_size
    src, tgt = _graphs(g, "src"), _graphs(g, "tgt")
    runs = []
    for stores in (False, True):
        m = pygda_amd.models.CWGCN(in_dim=10, hid_dim=8, num_classes=2, mode='graph', batch_size=batch_size, gnn="gcn",
                                   lr=0.01, weight_decay=0.001, device=DEV, epoch=3, verbose=0)
        log, cls_stage1 = [], {}
        m.epoch_hook = lambda e, loss, acc, secs: log.append((loss, acc))
        stage = m._stage

        def stage_rec(loader, optimizer, step, *a, m=m, stage=stage, cls_stage1=cls_stage1):
            if m.stage == 2:
                cls_stage1.update({k: v.detach().clone() for k, v in m.gnn.state_dict().items()})
            return stage(loader, optimizer, step, *a)

        m._stage = stage_rec
        torch.manual_seed(int(g["seed"]))
        m.fit(*_wrap(stores, src, tgt))
        torch.cuda.synchronize()
        runs.append((m, log, cls_stage1))
    (ml, logl, _), (ms, logs, cls1) = runs
    assert logs == logl and len(logs) == 9                      # two stages: 2 x 3 source epochs, 3 target epochs
    for (k, a), b in zip(ml.gnn.state_dict().items(), ms.gnn.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(ml.src_stats[0], ms.src_stats[0]) and torch.equal(ml.src_stats[1], ms.src_stats[1])
    state = torch.get_rng_state()
    for side in (False, True):
        torch.set_rng_state(state)
        pl, yl = ml.predict(None, source=side)
        torch.set_rng_state(state)
        ps, ys = ms.predict(None, source=side)
        assert torch.equal(pl, ps) and torch.equal(yl, ys)
    torch.set_rng_state(state)                                  # the golden's predictions follow the fit directly
    _check_golden(g, ms, logs, cls1, predict=batch_size == 0)


# ----------------------------------------------------------------------------------------------- no wait --
def test_drawing_a_batch_and_its_graph_never_waits_for_the_device():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.fail("this torch build has no sync debug mode")
    store = _case(10, "identity")[0]
    loader = StoreLoader(store, batch_size=5, shuffle=True)

    def epoch():
        out = []
        for b in loader:
            b = b.to(DEV)
            g = as_graph(b.edge_index, b.x.size(0))
            ops.spmm_kstep(g, b.x, 1), ops.spmm_kstep(g, b.x, 1, transposed=True)     # nor does aggregating over it
            out.append((b, g))
        return out

    epoch()                                                     # warm: the variant's one build, the allocators
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()                    # the mode is live: a read-back raises
        got = epoch()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(got) == 3 and sum(b.num_graphs for b, _ in got) == len(store)
    assert all(g.nnz == int(g.rowptr[g.num_nodes]) for _, g in got)      # known from the host counts, and right
