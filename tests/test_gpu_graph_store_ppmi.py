"""GPU: ``GraphStore(ppmi="per_graph")`` -- every ``PPMIConv`` layer's walks drawn once over the dataset-order graph and
kept per graph, a batch's PPMI graph gathered out of them (csrc/gda_collate.hip ``gda_collate_ppmi_f32``).  Every
comparison is bit for bit: a prefix batch against a fresh build of the collated prefix with the store's seed; a shuffled
batch against the sorted one, entry by entry; graphs a second store holds at the same place; batches without a pair;
the walks drawn once per (store, layer) and ``np.random`` left alone afterwards; no host wait; UDAGCN from stores
against lists, and over epochs."""
import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from pygda_amd.data import Data, GraphStore, _collate
from pygda_amd.graph import build_csr
from pygda_amd.nn.ppmi_conv import PPMIConv, ppmi_edges
from tests.test_gpu_graph_mode import _zero_dropouts
from tests.test_gpu_graph_store import make_graph
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

F = 10
# (nodes, edges drawn, make_graph options).  1 and 13: one node, nothing else; 2 and 6: nodes without an edge; 3: one
# node with nothing but self loops; 4, 7, 8, 9: duplicate edges; 5, 9, 12: one-directional edges; 4, 5, 11: self loops
SHAPES = [(5, 6, {}), (1, 0, {}), (7, 0, {}), (1, 2, dict(isolated=False, self_loops=2)),
          (12, 20, dict(self_loops=2, dups=3)), (40, 70, dict(undirected=False, self_loops=2)), (9, 0, {}),
          (2, 3, dict(isolated=False, dups=1)), (17, 30, dict(dups=4)),
          (33, 50, dict(undirected=False, dups=5, isolated=False)), (3, 4, {}), (24, 40, dict(self_loops=1)),
          (6, 5, dict(undirected=False)), (1, 0, {})]
TARGET_SHAPES = [(8, 10, dict(dups=2)), (1, 0, {}), (21, 30, dict(undirected=False, self_loops=1)), (4, 0, {}),
                 (15, 25, {}), (2, 1, dict(isolated=False)), (30, 45, dict(self_loops=3, dups=2)), (1, 1, dict(isolated=False, self_loops=1)),
                 (11, 14, dict(undirected=False)), (6, 8, {}), (19, 22, dict(dups=1)), (5, 3, {})]
G = len(SHAPES)
ARRAYS = ("rowptr", "colidx", "val", "t_rowptr", "t_colidx", "t_val")


def _graphs_of(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [Data(x=torch.randn(n, F, generator=g), edge_index=make_graph(n, e, seed + 31 * i, **kw),
                 y=torch.tensor([i % 3])) for i, (n, e, kw) in enumerate(shapes)]


def _drawn_seed(np_seed):
    """The seed ``ppmi_edges(seed=None)`` draws first after ``np.random.seed(np_seed)``."""
    np.random.seed(np_seed)
    return (int(np.random.randint(0, 2 ** 31)) << 31) | int(np.random.randint(0, 2 ** 31))


_cache = {}


def _data():
    if "graphs" not in _cache:
        _cache["graphs"] = _graphs_of(SHAPES, 500)
    return _cache["graphs"]


def _warm(path_len, np_seed=7, order=None, improved=False):
    """``(store, layer, graphs)`` with the layer's walks drawn after ``np.random.seed(np_seed)``; built once and shared."""
    key = (path_len, np_seed, None if order is None else tuple(order), improved)
    if key not in _cache:
        graphs = _data() if order is None else [_data()[i] for i in order]
        store = GraphStore(graphs, DEV, ppmi="per_graph")
        conv = PPMIConv(F, 8, path_len=path_len, improved=improved)
        np.random.seed(np_seed)
        assert store.ppmi_pairs(conv).seed == _drawn_seed(np_seed)
        _cache[key] = (store, conv, graphs)
    return _cache[key]


def _ppmi_graph(store, conv, ids):
    batch = store.batch(ids)
    return batch, batch.edge_index._gda_store_batch.ppmi_graph(conv)


def _assert_same_graph(g, want):
    n, nnz = want.num_nodes, want.nnz
    assert g.num_nodes == n and g.nnz == nnz == int(g.rowptr[n]) == int(g.t_rowptr[n])
    for a in ARRAYS:
        k = n + 1 if a.endswith("rowptr") else nnz
        assert torch.equal(getattr(g, a)[:k], getattr(want, a)[:k]), a


def _entries(g, batch, ids):
    """The stored entries of both orientations as sorted ``(store graph id, local row, local column, value bits)``."""
    seg, pos = batch.batch._gda_seg_ptr.cpu(), batch.batch.cpu()
    ids = torch.tensor(ids)
    out = []
    for rp, ci, va in ((g.rowptr, g.colidx, g.val), (g.t_rowptr, g.t_colidx, g.t_val)):
        rp, nnz = rp.cpu().long(), g.nnz
        row = torch.repeat_interleave(torch.arange(g.num_nodes), rp[1:] - rp[:-1])
        col, bits = ci[:nnz].cpu().long(), va[:nnz].cpu().view(torch.int32)
        assert torch.equal(pos[row], pos[col])                              # no entry crosses a graph
        first = seg[pos[row]]
        out.append(sorted(zip(ids[pos[row]].tolist(), (row - first).tolist(), (col - first).tolist(), bits.tolist())))
    return out


# --------------------------------------------------------------------------------------------- the graphs --
@pytest.mark.parametrize("path_len", [5, 10])
@pytest.mark.parametrize("k", [1, 2, 4, 6, 9, G])
def test_a_prefix_batch_is_the_fresh_build_of_the_collated_prefix(path_len, k):
    store, conv, graphs = _warm(path_len)
    s = _drawn_seed(7)
    batch, g = _ppmi_graph(store, conv, range(k))
    assert batch.edge_index._gda_store_batch.ppmi_graph(conv) is g                   # one graph per (batch, layer)
    ref = _collate(graphs[:k]).to(DEV)
    n = ref.x.size(0)
    ei, w = ppmi_edges(ref.edge_index, n, path_len, 40, seed=s)
    want = build_csr(ei, n, w, False, True, True, "row")
    _assert_same_graph(g, want)
    assert (g.static, g.transient) == (want.static, want.transient)
    assert g._split is not None and g._t_split is not None and g._split.n_long == g._t_split.n_long == 0
    x = torch.randn(n, 8, device=DEV, generator=torch.Generator(DEV).manual_seed(k))
    for transposed in (False, True):
        assert torch.equal(ops.spmm_kstep(g, x, 1, transposed=transposed), ops.spmm_kstep(want, x, 1, transposed=transposed))


def test_the_layer_route_and_the_improved_variant():
    """``PPMIConv._graph`` takes the handle's route for a ``per_graph`` store batch (and the ``improved`` flag of the
    layer reaches the ingestion); a ``per_batch`` store and a plain edge list keep today's route."""
    store, conv, graphs = _warm(5, improved=True)
    batch = store.batch(range(G))
    n = batch.x.size(0)
    g = conv._graph(batch.x, batch.edge_index, "k", None)
    assert g is batch.edge_index._gda_store_batch.ppmi_graph(conv) and conv.cache_dict["k"] is g
    ei, w = ppmi_edges(_collate(graphs).to(DEV).edge_index, n, 5, 40, seed=_drawn_seed(7))
    _assert_same_graph(g, build_csr(ei, n, w, True, True, True, "row"))
    calls = []
    orig = _lib.call
    try:
        _lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        plain, layer = GraphStore(graphs, DEV), PPMIConv(F, 8)
        assert plain.ppmi == "per_batch"
        layer._graph(batch.x, plain.batch(range(G)).edge_index, "k", None)
        layer._graph(batch.x, _collate(graphs).to(DEV).edge_index, "l", None)
    finally:
        _lib.call = orig
    assert calls.count("gda_ppmi_build") == 2 and "gda_ppmi_build_ratio" not in calls and "gda_collate_ppmi_f32" not in calls
    with pytest.raises(ValueError, match="per_batch"):
        plain.ppmi_pairs(layer)


@pytest.mark.parametrize("path_len", [5, 10])
def test_a_shuffled_batch_holds_the_entries_of_the_sorted_one(path_len):
    store, conv, _ = _warm(path_len)
    shuffled = [9, 3, 12, 0, 6, 5, 13, 8, 1, 4]
    for ids in (shuffled, shuffled[::-1], [5, 5, 3]):
        got = _entries(*_ppmi_graph(store, conv, ids)[::-1], ids)
        want = _entries(*_ppmi_graph(store, conv, sorted(ids))[::-1], sorted(ids))
        assert got == want and len(got[0]) == len(got[1]) > 0


@pytest.mark.parametrize("path_len", [5, 10])
def test_a_subset_is_weighted_with_its_own_target_count(path_len):
    """Graphs 0..3 sit at the same place in a second store that holds the subset first, so both stores draw the same
    walks for them (same seed, same node ids); the second store's prefix is, by the prefix test, the fresh build of the
    subset.  The first store's batch of the subset must give those graphs the same values -- the subset's target count
    in the log, not the dataset's and not a prefix's."""
    subset = [0, 1, 2, 3, 8, 5, 11]
    store, conv, _ = _warm(path_len)
    second, conv2, _ = _warm(path_len, order=subset + [i for i in range(G) if i not in subset])
    assert store.ppmi_pairs(conv).seed == second.ppmi_pairs(conv2).seed
    got = _entries(*_ppmi_graph(store, conv, subset)[::-1], subset)
    want = _entries(*_ppmi_graph(second, conv2, range(len(subset)))[::-1], list(range(len(subset))))
    full = _entries(*_ppmi_graph(store, conv, range(G))[::-1], list(range(G)))
    for side in (0, 1):
        same = [e for e in got[side] if e[0] < 4]
        assert same and same == [e for e in want[side] if e[0] < 4]
        assert same != [e for e in full[side] if e[0] < 4]              # (the dataset's count gives other weights)


def test_a_batch_without_a_pair_evaluates_no_log():
    store, conv, _ = _warm(5)
    calls = []
    orig = _lib.call
    try:
        _lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        batch, g = _ppmi_graph(store, conv, [2, 13, 6, 1, 2])
    finally:
        _lib.call = orig
    assert "gda_collate_ppmi_f32" not in calls and "gda_ppmi_build_ratio" not in calls and "gda_ppmi_build" not in calls
    n = batch.x.size(0)
    assert n == 7 + 1 + 9 + 1 + 7 and g.nnz == n
    own = torch.arange(n + 1, dtype=torch.int32, device=DEV)
    for rp, ci, va in ((g.rowptr, g.colidx, g.val), (g.t_rowptr, g.t_colidx, g.t_val)):
        assert torch.equal(rp, own) and torch.equal(ci[:n], own[:n]) and torch.equal(va[:n], torch.ones(n, device=DEV))


def test_beyond_the_builder_limits_is_an_error_that_names_the_sizes():
    store = GraphStore(_data(), DEV, ppmi="per_graph")
    with pytest.raises(ValueError, match=rf"{store.num_nodes} nodes.*path_len {2 ** 22}"):
        store.ppmi_pairs(PPMIConv(F, 8, path_len=2 ** 22))


# ------------------------------------------------------------------------------------------ one draw only --
def _udagcn(batch_size):
    return pygda_amd.models.UDAGCN(F, 8, 3, mode='graph', ppmi=True, num_layers=2, adv_dim=6, lr=0.01, weight_decay=0.003,
                                   device=DEV, epoch=3, verbose=0, batch_size=batch_size)


def _fit(batch_size, mode, spy=None):
    """A seeded three-epoch fit from stores: ``(trainer, per-epoch log, predict, target store)``."""
    src, tgt = (GraphStore(gs, DEV, ppmi=mode) for gs in (_data(), _graphs_of(TARGET_SHAPES, 900)))
    m = _udagcn(batch_size)
    seen = []
    m.epoch_hook = lambda e, loss, acc, secs: seen.append((float(loss), acc))
    torch.manual_seed(3)
    np.random.seed(5)
    orig = _lib.call
    try:
        if spy is not None:
            _lib.call = lambda name, *a: (spy.append(name), orig(name, *a))[1]
        m.fit(src, tgt)
        state = np.random.get_state()
        pred = m.predict(tgt)
    finally:
        _lib.call = orig
    return m, seen, pred, tgt, state


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("batch_size", [0, 6])
def test_the_walks_are_drawn_once_per_store_and_layer(monkeypatch, batch_size):
    _zero_dropouts(monkeypatch)
    encodes = []
    encode = pygda_amd.nn.UDAGCNBase.encode
    monkeypatch.setattr(pygda_amd.nn.UDAGCNBase, "encode", lambda self, *a, **k: (encodes.append(1), encode(self, *a, **k))[1])
    calls = []
    m, seen, _, tgt, after_fit = _fit(batch_size, "per_graph", calls)
    steps = 3 * (1 if batch_size == 0 else 2)                  # 14 and 12 graphs: one batch each, or two pairs of batches
    assert len(encodes) >= 2 * steps + 1
    # two stores x two PPMIConv layers, over three epochs and predict(); the weight builder never runs
    assert calls.count("gda_ppmi_build_ratio") == 4 and calls.count("gda_ppmi_build") == 0
    assert calls.count("gda_collate_ppmi_f32") == 2 * len(encodes)
    # eight draws in all (two per seed), all during the first step; predict() and further batches draw nothing
    np.random.seed(5)
    for _ in range(8):
        np.random.randint(0, 2 ** 31)
    assert _same_state(after_fit, np.random.get_state())
    np.random.set_state(after_fit)
    m.predict(tgt)
    conv = m.udagcn.ppmi_encoder.conv_layers[0]
    for ids in ([3, 1], range(len(tgt))):
        _ppmi_graph(tgt, conv, ids)
    assert _same_state(after_fit, np.random.get_state())
    assert len(tgt._ppmi_pairs) == 2

    # per batch, as before: the weight builder once per layer and batch
    del encodes[:]
    calls = []
    _fit(batch_size, "per_batch", calls)
    assert calls.count("gda_ppmi_build") == 2 * len(encodes) and len(encodes) >= 2 * steps + 1
    assert calls.count("gda_ppmi_build_ratio") == calls.count("gda_collate_ppmi_f32") == 0


def test_the_walks_live_as_long_as_the_layer():
    import gc
    store = GraphStore(_data(), DEV, ppmi="per_graph")
    conv = PPMIConv(F, 8)
    first = store.ppmi_pairs(conv)
    assert store.ppmi_pairs(conv) is first and len(store._ppmi_pairs) == 1
    del conv
    gc.collect()
    assert len(store._ppmi_pairs) == 0


# ----------------------------------------------------------------------------------------------- no wait --
def test_drawing_a_batch_and_its_ppmi_graph_never_waits_for_the_device():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.fail("this torch build has no sync debug mode")
    store, conv, _ = _warm(5)
    id_lists = ([4, 0, 9, 12, 1], [2, 13, 6], [11, 5, 8, 3, 7, 10])

    def epoch():
        out = []
        for ids in id_lists:
            b, g = _ppmi_graph(store, conv, ids)
            ops.spmm_kstep(g, b.x, 1), ops.spmm_kstep(g, b.x, 1, transposed=True)     # nor does aggregating over it
            out.append((b, g))
        return out

    epoch()                                                     # warm: the allocators, the ingestion workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()                    # the mode is live: a read-back raises
        got = epoch()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(got) == 3
    assert all(g.nnz == int(g.rowptr[g.num_nodes]) for _, g in got)      # known from the host counts, and right


# ---------------------------------------------------------------------------------------------- trainers --
def test_udagcn_step_from_per_graph_stores_equals_lists(monkeypatch):
    """One ``forward_model`` plus backward on the whole datasets in dataset order: loss, both logits, every gradient."""
    _zero_dropouts(monkeypatch)
    src, tgt = _data(), _graphs_of(TARGET_SHAPES, 900)
    runs = []
    for stores in (False, True):
        m = _udagcn(0)
        torch.manual_seed(11)
        net = m.udagcn = m.init_model()
        for mod in net.models:
            mod.train()
        if stores:
            sb, tb = (GraphStore(gs, DEV, ppmi="per_graph").batch(range(len(gs))) for gs in (src, tgt))
        else:
            sb, tb = _collate(src).to(DEV), _collate(tgt).to(DEV)
        torch.manual_seed(12)
        np.random.seed(13)
        loss, sl, tl = m.forward_model(sb, tb, 0.05, 2)
        net.zero_grad()
        loss.backward()
        runs.append((loss.detach(), sl.detach(), tl.detach(), {k: p.grad for k, p in net.named_parameters()},
                     np.random.get_state()))
    (ll, sll, tll, gl, state_l), (ls, sls, tls, gs_, state_s) = runs
    assert torch.isfinite(ll) and torch.equal(ll, ls) and torch.equal(sll, sls) and torch.equal(tll, tls)
    assert sll.shape == (len(src), 3) and tll.shape == (len(tgt), 3)
    assert gl.keys() == gs_.keys() and len(gl) > 4
    for k in gl:
        assert gl[k] is not None and torch.equal(gl[k], gs_[k]), k
    assert _same_state(state_l, state_s)                          # the same draws, in the same order


@pytest.mark.parametrize("batch_size", [0, 6])
def test_udagcn_fit_from_per_graph_stores_is_reproducible(monkeypatch, batch_size):
    _zero_dropouts(monkeypatch)
    (ma, loga, (pa, ya), _, _), (mb, logb, (pb, yb), _, _) = (_fit(batch_size, "per_graph") for _ in range(2))
    assert loga == logb and len(loga) == 3 and all(np.isfinite(l) for l, _ in loga)
    for (k, a), b in zip(ma.udagcn.state_dict().items(), mb.udagcn.state_dict().values()):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), k
    assert torch.equal(pa, pb) and torch.equal(ya, yb) and pa.shape == (len(TARGET_SHAPES), 3)
