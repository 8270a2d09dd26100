"""GPU: the sort-free PPMI graph of a ``GraphStore(ppmi="per_graph")`` batch (csrc/gda_collate.hip
``gda_collate_ppmi_csr_f32``).  ``ppmi_graph(conv)`` must equal, bit for bit and in every array, what the ingestion
makes of the batch's pair list -- which the test gathers itself with ``gda_collate_offsets`` and ``gda_collate_ppmi_f32``
(the assembly takes its weights from the same gather, but from a call of its own) -- for whole, permuted, partial,
single-graph and repeated-id batches, two walk lengths and both fill values; without calling the ingestion, without a host wait, and the same bits twice."""
import pytest
import torch

import numpy as np

import pygda_amd.graph
from pygda_amd import _lib
from pygda_amd.data import Data, GraphStore
from pygda_amd.graph import build_csr
from pygda_amd.nn.ppmi_conv import PPMIConv
from tests.test_gpu_graph_store import make_graph
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

F = 4
PATH = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
# (nodes, edges drawn, make_graph options) or a ready edge list.  0: one node, no edge; 1 and 7: explicit self-loop edges;
# 2: the path 0 - 1 - 2; 3: wider than a wavefront; 4, 5, 8, 10: an isolated last node; 6, 9: one-directional edges
SHAPES = [(1, 0, {}), (6, 7, dict(self_loops=2, isolated=False)), PATH, (70, 110, dict(dups=3)), (9, 10, {}),
          (14, 0, {}), (12, 16, dict(undirected=False, isolated=False)), (2, 1, dict(self_loops=1, isolated=False)),
          (23, 30, dict(self_loops=1)), (31, 40, dict(undirected=False, dups=2, isolated=False)), (5, 4, {}), (3, 3, dict(isolated=False))]
G = len(SHAPES)
SUBSET = [10, 2, 0, 4, 7]
BATCHES = {"dataset_order": list(range(G)), "permuted": [3, 11, 0, 7, 5, 9, 2, 10, 1, 8, 6, 4], "subset": SUBSET,
           "single": [3], "repeated": [2, 6, 2, 0, 6]}
ARRAYS = ("rowptr", "colidx", "val", "t_rowptr", "t_colidx", "t_val")

_cache = {}


def _graphs():
    if "graphs" not in _cache:
        g = torch.Generator().manual_seed(41)
        out = []
        for i, shape in enumerate(SHAPES):
            n, ei = (3, shape) if torch.is_tensor(shape) else (shape[0], make_graph(shape[0], shape[1], 700 + 13 * i, **shape[2]))
            out.append(Data(x=torch.randn(n, F, generator=g), edge_index=ei, y=torch.tensor([i % 3])))
        _cache["graphs"] = out
    return _cache["graphs"]


def _warm(path_len, improved):
    """``(store, layer)`` with the layer's walks drawn after ``np.random.seed(19)``; built once and shared."""
    key = (path_len, improved)
    if key not in _cache:
        store = GraphStore(_graphs(), DEV, ppmi="per_graph")
        conv = PPMIConv(F, 8, path_len=path_len, improved=improved)
        np.random.seed(19)
        store.ppmi_pairs(conv)
        _cache[key] = (store, conv)
    return _cache[key]


def _pair_list(store, conv, batch):
    """The batch's PPMI pair list and weights, gathered here: offsets scan with the pair pointer, then the pair gather."""
    h, p = batch.edge_index._gda_store_batch, store.ppmi_pairs(conv)
    B = h.ids.numel()
    m, targets = (int(c[h.ids_host].sum()) for c in (p.pair_counts, p.target_counts))
    pairs, w = torch.empty(2, m, dtype=torch.long, device=DEV), torch.empty(m, dtype=torch.float32, device=DEV)
    seg_ptr, pair_off = (torch.empty(B + 1, dtype=torch.long, device=DEV) for _ in range(2))
    _lib.call("gda_collate_offsets", h.ids, B, len(store), store.node_ptr, p.pair_ptr, seg_ptr, pair_off, _lib.stream())
    if m:
        _lib.call("gda_collate_ppmi_f32", h.ids, B, len(store), p.pair_ptr, pair_off, h.seg_ptr, p.local_src, p.local_dst,
                  p.ratio, p.num_pairs, targets, p.path_len, m, pairs, w, _lib.stream())
    return pairs, w


def _layout(split):
    return split.threshold, split.n_long, split.n_chunks


def _assert_same_graph(g, want):
    n, nnz = want.num_nodes, want.nnz                               # (the reference's count: one read-back)
    assert g.num_nodes == n and g._nnz == nnz == int(g.rowptr[n]) == int(g.t_rowptr[n])
    for a in ARRAYS:
        k = n + 1 if a.endswith("rowptr") else nnz
        got, ref = getattr(g, a)[:k], getattr(want, a)[:k]
        assert got.dtype == ref.dtype and torch.equal(got, ref), a
    for transposed in (False, True):
        assert _layout(g.split(transposed)) == _layout(want.split(transposed)), transposed
    assert (g.static, g.transient, g.t_to_fwd) == (want.static, want.transient, None)


def test_the_library_exports_the_entry_point():
    assert hasattr(_lib.lib(), "gda_collate_ppmi_csr_f32") and "gda_collate_ppmi_csr_f32" in _lib.EXPORTED_SYMBOLS


@pytest.mark.parametrize("path_len", [10, 3])
def test_the_dataset_has_the_cases_the_comparison_is_about(path_len):
    store, conv = _warm(path_len, False)
    p = store.ppmi_pairs(conv)
    ptr = p.pair_ptr.cpu()
    assert int(ptr[1]) == 0 and store.node_counts[0] == 1                       # the one-node graph has no pair
    assert bool((p.local_src == p.local_dst).any())                             # a pair (a, a): it weighs a's loop
    first = store.node_ptr[torch.bucketize(torch.arange(p.num_pairs, device=DEV), p.pair_ptr[1:], right=True)]
    with_pair = torch.zeros(store.num_nodes, dtype=torch.bool, device=DEV)
    with_pair[first + p.local_src] = True
    with_pair[first + p.local_dst] = True
    assert not bool(with_pair.all())                                            # a node no pair names
    batch = store.batch(SUBSET)
    _, w = _pair_list(store, conv, batch)
    assert bool((w == 0).any()) and bool((w > 0).any())                         # a weight the clip sets to exactly 0
    g = batch.edge_index._gda_store_batch.ppmi_graph(conv)
    assert bool(((g.t_rowptr[1:] - g.t_rowptr[:-1]) == 1).any())                # a row that is its loop alone
    assert int(store.node_counts[3]) > 64 and p.entry_counts.tolist() == (p.pair_counts - p.loop_counts + store.node_counts).tolist()


@pytest.mark.parametrize("improved", [False, True])
@pytest.mark.parametrize("path_len", [10, 3])
@pytest.mark.parametrize("name", list(BATCHES))
def test_the_assembled_graph_is_the_ingestion_of_the_pair_list(name, path_len, improved):
    store, conv = _warm(path_len, improved)
    batch = store.batch(BATCHES[name])
    n = batch.x.size(0)
    g = batch.edge_index._gda_store_batch.ppmi_graph(conv)
    assert batch.edge_index._gda_store_batch.ppmi_graph(conv) is g                # one graph per (batch, layer)
    pairs, w = _pair_list(store, conv, batch)
    want = build_csr(pairs, n, w, improved, True, True, "row", validate=False)
    _assert_same_graph(g, want)


def test_improved_changes_nothing_but_the_filled_loops():
    (store, conv), (store2, conv2) = _warm(10, False), _warm(10, True)
    assert store.ppmi_pairs(conv).seed == store2.ppmi_pairs(conv2).seed        # same draws after the same np seed
    a = store.batch(BATCHES["permuted"]).edge_index._gda_store_batch.ppmi_graph(conv)
    b = store2.batch(BATCHES["permuted"]).edge_index._gda_store_batch.ppmi_graph(conv2)
    for name in ("rowptr", "colidx", "t_rowptr", "t_colidx"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(a.val, b.val)


def test_the_assembly_calls_no_ingestion_and_never_waits(monkeypatch):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.fail("this torch build has no sync debug mode")
    store, conv = _warm(10, False)
    first = [store.batch(ids).edge_index._gda_store_batch.ppmi_graph(conv) for ids in BATCHES.values()]     # first use
    built, calls = [], []
    real_build, real_call = pygda_amd.graph.build_csr, _lib.call
    monkeypatch.setattr(pygda_amd.graph, "build_csr", lambda *a, **k: (built.append(1), real_build(*a, **k))[1])
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()                    # the mode is live: a read-back raises
        again = [store.batch(ids).edge_index._gda_store_batch.ppmi_graph(conv) for ids in BATCHES.values()]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert built == [] and "gda_build_csr_norm_map" not in calls
    # per assembly: the pair gather (one double log per pair) and the sort-free assembly that reads its weights
    assert calls.count("gda_collate_ppmi_csr_f32") == calls.count("gda_collate_ppmi_f32") == len(BATCHES)
    for a, b in zip(first, again):                              # two assemblies, the same bits
        assert a is not b and a._nnz == b._nnz
        for name in ARRAYS:
            k = a.num_nodes + 1 if name.endswith("rowptr") else a._nnz
            assert torch.equal(getattr(a, name)[:k].view(torch.int32), getattr(b, name)[:k].view(torch.int32)), name
