"""CPU: the device-resident graph dataset (pygda_amd.data.GraphStore) on the host -- its loader draws what
``DataLoader`` over the list of graphs draws, the graph-mode trainers take it for a list, it is a Sequence, it checks
its graphs once, and the collation entry points (csrc/gda_collate.hip) validate their arguments before anything touches
a device.

The convolutions have no CPU path, so no trainer's own ``fit`` runs on this side (with lists either).  The acceptance
test drives each trainer's real loaders, epoch loop and ``_predict_loader`` with a torch-only network instead; the
trainers' own steps are compared store against list, bit for bit, in tests/test_gpu_graph_store.py."""
import ctypes

import pytest
import torch

import pygda_amd
from pygda_amd import _lib
from pygda_amd.data import Data, DataLoader, GraphStore, StoreLoader
from tests.conftest import T, load_golden

NULL, SIZE, ALIAS = -1, -2, -5


def _dataset(g, prefix):
    return [Data(x=T(g[f"{prefix}/{i}/x"]), edge_index=T(g[f"{prefix}/{i}/ei"]), y=T(g[f"{prefix}/{i}/y"]))
            for i in range(int(g[f"{prefix}/count"]))]


@pytest.fixture(scope="module")
def domains():
    g = load_golden("a2gnn_graph_fit3_b6")
    src, tgt = _dataset(g, "src"), _dataset(g, "tgt")
    assert (len(src), len(tgt)) == (14, 11)
    return src, tgt


def _same_batch(a, b):
    return (all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("x", "edge_index", "y", "batch"))
            and a.num_graphs == b.num_graphs and a.batch._gda_sorted and a.batch._gda_num_graphs == b.batch._gda_num_graphs)


# ----------------------------------------------------------------------------------------------- loader --
@pytest.mark.parametrize("batch_size", [0, 5, 6])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("seed", [0, 7])
def test_store_loader_draws_what_the_list_loader_draws(domains, which, batch_size, seed):
    graphs = domains[which]
    bs = batch_size or len(graphs)
    for g_id, g in enumerate(graphs):
        g.tag = g_id                       # which graph a list batch holds: read off the objects the collation is handed
    picked = []

    def collate(batch):
        picked.append([g.tag for g in batch])
        return len(batch)

    torch.manual_seed(seed)
    lists = torch.utils.data.DataLoader(graphs, batch_size=bs, shuffle=True, collate_fn=collate)
    for _ in range(2):
        list(lists)
    want, want_state = picked, torch.get_rng_state()

    torch.manual_seed(seed)
    loader = StoreLoader(GraphStore(graphs, "cpu"), batch_size=bs, shuffle=True)
    got = [ids for _ in range(2) for ids in loader.id_batches()]
    assert got == want and len(got) == 2 * -(-len(graphs) // bs)
    assert torch.equal(torch.get_rng_state(), want_state)

    # and the batches themselves, against the project's own list loader
    torch.manual_seed(seed)
    ref = [b for _ in range(2) for b in DataLoader(graphs, batch_size=bs, shuffle=True)]
    torch.manual_seed(seed)
    mine = [b for _ in range(2) for b in loader]
    assert len(ref) == len(mine) and all(_same_batch(a, b) for a, b in zip(mine, ref))
    assert torch.equal(torch.get_rng_state(), want_state)


# ---------------------------------------------------------------------------------------------- trainers --
def _trainer(tag, batch_size):
    M = pygda_amd.models
    common = dict(device="cpu", epoch=3, verbose=0, batch_size=batch_size)
    if tag == "grade":
        return M.GRADE(10, 8, 3, mode='graph', num_layers=2, dropout=0.0, disc="JS", **common)
    if tag == "udagcn":
        return M.UDAGCN(10, 8, 3, mode='graph', num_layers=2, ppmi=False, adv_dim=6, **common)
    if tag == "adagcn":
        return M.AdaGCN(10, 8, 3, mode='graph', num_layers=2, adv_dim=6, **common)
    return M.DANE(10, 8, 3, num_layers=2, mode='graph', dropout=0.0, gnn="gcn", k=5, **common)


class _PoolNet(torch.nn.Module):
    """Torch-only stand-in for a graph-mode network: mean readout over ``batch``, the in-degree as one more input."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(11, 3)

    def forward(self, b):
        deg = torch.zeros(b.x.size(0)).index_add_(0, b.edge_index[1], torch.ones(b.edge_index.size(1)))
        h = torch.cat([b.x, deg[:, None]], dim=1)
        pooled = torch.zeros(b.num_graphs, 11).index_add_(0, b.batch, h)
        return self.lin(pooled / torch.bincount(b.batch, minlength=b.num_graphs).clamp(min=1)[:, None])


def _run(tag, batch_size, src, tgt):
    m = _trainer(tag, batch_size)
    seen = []
    m.epoch_hook = lambda e, loss, acc, secs: seen.append((loss, acc))
    torch.manual_seed(11)
    net = _PoolNet()
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    m._loaders(src, tgt)

    def step(s, t, alpha, epoch):
        out = net(s)
        return torch.nn.functional.cross_entropy(out, s.y) + 0.1 * net(t).square().mean(), out

    m._train_epochs(net, opt, step, lambda e: 0.0)
    net.eval()
    logits, labels = m._predict_loader(m.target_loader, net)
    return seen, [p.detach().clone() for p in net.parameters()], logits, labels, torch.get_rng_state()


@pytest.mark.parametrize("batch_size", [0, 6])
@pytest.mark.parametrize("tag", ["grade", "udagcn", "adagcn", "dane"])
def test_graph_mode_trainers_take_stores_for_lists(domains, tag, batch_size):
    src, tgt = domains
    want = _run(tag, batch_size, src, tgt)
    assert len(want[0]) == 3
    for s, t in ((GraphStore(src, "cpu"), GraphStore(tgt, "cpu")), (GraphStore(src, "cpu"), tgt), (src, GraphStore(tgt, "cpu"))):
        got = _run(tag, batch_size, s, t)
        assert got[0] == want[0]                                       # losses and accuracies
        assert all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
        assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])


def test_cwgcn_scope_check_reads_a_store_like_a_list(domains):
    src, tgt = domains
    m = pygda_amd.models.CWGCN(in_dim=10, hid_dim=8, num_classes=3, mode='graph', gnn="gcn", device="cpu", verbose=0)
    m._check_scope(GraphStore(src, "cpu"), GraphStore(tgt, "cpu"))
    m._loaders(GraphStore(src, "cpu"), tgt)
    assert isinstance(m.source_loader, StoreLoader) and type(m.target_loader) is DataLoader
    with pytest.raises(ValueError, match="classes"):
        pygda_amd.models.CWGCN(in_dim=10, hid_dim=8, num_classes=5, mode='graph', gnn="gcn", device="cpu",
                               verbose=0)._check_scope(GraphStore(src, "cpu"), tgt)


# ---------------------------------------------------------------------------------------------- sequence --
def test_store_is_a_sequence_of_its_graphs(domains):
    import collections.abc
    src, _ = domains
    st = GraphStore(iter(src), "cpu")
    assert isinstance(st, collections.abc.Sequence) and len(st) == 14
    assert st[0] is src[0] and st[-1] is src[-1] and st[2:4] == src[2:4]
    assert list(st) == src and list(reversed(st)) == src[::-1] and src[3] in st and st.index(src[5]) == 5
    with pytest.raises(IndexError):
        st[14]
    assert st.node_counts.dtype == st.edge_counts.dtype == torch.long
    assert st.node_counts.tolist() == [g.x.size(0) for g in src]
    assert st.edge_counts.tolist() == [g.edge_index.size(1) for g in src]
    assert st.num_nodes == sum(g.x.size(0) for g in src) and st.num_features == 10
    one = st.batch([3, 0, 3])
    assert _same_batch(one, next(iter(DataLoader([src[3], src[0], src[3]], batch_size=3))))
    assert one.to("cpu") is one
    with pytest.raises(ValueError):
        st.batch([])


def test_empty_graphs_are_legal():
    gs = [Data(x=torch.zeros(0, 4), edge_index=torch.zeros(2, 0, dtype=torch.long), y=torch.tensor([1])),
          Data(x=torch.ones(3, 4), edge_index=torch.zeros(2, 0, dtype=torch.long), y=torch.tensor([0])),
          Data(x=torch.ones(2, 4), edge_index=torch.tensor([[0, 1, 1], [1, 0, 1]]), y=torch.tensor(2))]
    st = GraphStore(gs, "cpu")
    assert st.node_counts.tolist() == [0, 3, 2] and st.edge_counts.tolist() == [0, 0, 3]
    b = st.batch([0, 2, 1, 0])
    assert b.x.shape == (5, 4) and b.edge_index.tolist() == [[0, 1, 1], [1, 0, 1]] and b.y.tolist() == [1, 2, 0, 1]
    assert b.batch.tolist() == [1, 1, 2, 2, 2]


# ------------------------------------------------------------------------------------------------ errors --
def test_construction_errors_name_the_graph():
    ok = lambda: Data(x=torch.ones(3, 4), edge_index=torch.tensor([[0, 1], [1, 2]]), y=torch.tensor([1]))

    def broken(**kw):
        gs = [ok(), ok(), ok()]
        for k, v in kw.items():
            setattr(gs[2], k, v)
        return gs

    for kw in (dict(x=torch.ones(3)), dict(x=torch.ones(3, 4, dtype=torch.float64)), dict(x=torch.ones(3, 5)),
               dict(x=None), dict(y=torch.tensor([1, 2])), dict(y=torch.tensor([1.0])), dict(y=None),
               dict(edge_index=torch.tensor([[0, 3], [1, 2]])), dict(edge_index=torch.tensor([[0, -1], [1, 2]])),
               dict(edge_index=torch.tensor([0, 1])), dict(edge_index=torch.tensor([[0, 1], [1, 2]], dtype=torch.int32)),
               dict(x=torch.ones(0, 4))):                    # no nodes, but edges
        with pytest.raises(ValueError, match="graph 2"):
            GraphStore(broken(**kw), "cpu")
    with pytest.raises(ValueError, match=r"\[0, 3\), found \[0, 3\]"):
        GraphStore(broken(edge_index=torch.tensor([[0, 3], [1, 2]])), "cpu")
    GraphStore(broken(), "cpu")


# --------------------------------------------------------------------------------------------------- ABI --
def P(addr):
    return ctypes.c_void_p(addr)


# distinct non-NULL dummies: validation comes first, nothing is dereferenced
IDS, NPTR, EPTR, SEG, EOFF, X, Y, XO, BO, YO, ED, EO, RP, NOFF = (P(0x1000 * k) for k in range(1, 15))
CSR_IN = tuple(P(0x100000 + 0x1000 * k) for k in range(6))
CSR_OUT = tuple(P(0x200000 + 0x1000 * k) for k in range(6))


def offsets(ids=IDS, B=4, G=9, node_ptr=NPTR, edge_ptr=EPTR, seg=SEG, eoff=EOFF):
    return _lib.lib().gda_collate_offsets(ids, B, G, node_ptr, edge_ptr, seg, eoff, None)


def nodes(ids=IDS, B=4, G=9, node_ptr=NPTR, seg=SEG, x=X, F=8, y=Y, n=20, xo=XO, bo=BO, yo=YO):
    return _lib.lib().gda_collate_nodes_f32(ids, B, G, node_ptr, seg, x, F, y, n, xo, bo, yo, None)


def edges(ids=IDS, B=4, G=9, edge_ptr=EPTR, eoff=EOFF, seg=SEG, ed=ED, E=50, e=30, out=EO):
    return _lib.lib().gda_collate_edges(ids, B, G, edge_ptr, eoff, seg, ed, E, e, out, None)


def csr_offsets(ids=IDS, B=4, G=9, node_ptr=NPTR, rowptr=RP, out=NOFF):
    return _lib.lib().gda_collate_csr_offsets(ids, B, G, node_ptr, rowptr, out, None)


def csr(ids=IDS, B=4, G=9, node_ptr=NPTR, seg=SEG, batch=BO, n=20, noff=NOFF, nnz=60, ins=CSR_IN, outs=CSR_OUT):
    return _lib.lib().gda_collate_csr_f32(ids, B, G, node_ptr, seg, batch, n, noff, nnz, *ins, *outs, None)


def _swap(seq, k, v):
    return tuple(v if i == k else a for i, a in enumerate(seq))


def test_collation_entry_points_validate_their_arguments():
    for fn, names in ((offsets, ("ids", "node_ptr", "edge_ptr", "seg", "eoff")),
                      (nodes, ("ids", "node_ptr", "seg", "x", "y", "xo", "bo", "yo")),
                      (edges, ("ids", "edge_ptr", "eoff", "seg", "ed", "out")),
                      (csr_offsets, ("ids", "node_ptr", "rowptr", "out")),
                      (csr, ("ids", "node_ptr", "seg", "batch", "noff"))):
        for missing in names:
            assert fn(**{missing: None}) == NULL, (fn.__name__, missing)
        assert fn(B=-1) == SIZE and fn(G=-1) == SIZE, fn.__name__
    for k in range(6):
        assert csr(ins=_swap(CSR_IN, k, None)) == NULL and csr(outs=_swap(CSR_OUT, k, None)) == NULL, k
    assert nodes(F=-1) == SIZE and nodes(n=-1) == SIZE
    assert edges(E=-1) == SIZE and edges(e=-1) == SIZE and edges(E=0, e=1) == SIZE
    assert csr(n=-1) == SIZE and csr(nnz=-1) == SIZE
    assert csr(n=2 ** 31 - 1) == SIZE and csr(nnz=2 ** 31) == SIZE           # the CSR's indices are 32-bit
    # an output on top of an input (or of another output)
    assert offsets(seg=EOFF) == ALIAS and offsets(seg=IDS) == ALIAS and offsets(eoff=NPTR) == ALIAS
    assert nodes(xo=X) == ALIAS and nodes(yo=Y) == ALIAS and nodes(bo=IDS) == ALIAS and nodes(bo=YO) == ALIAS
    assert edges(out=ED) == ALIAS and edges(out=IDS) == ALIAS
    assert csr_offsets(out=IDS) == ALIAS and csr_offsets(out=NPTR) == ALIAS
    for k in range(6):
        assert csr(outs=_swap(CSR_OUT, k, CSR_IN[k])) == ALIAS, k
        assert csr(outs=_swap(CSR_OUT, k, CSR_OUT[(k + 3) % 6])) == ALIAS, k


def test_an_empty_batch_launches_nothing_and_looks_at_no_operand():
    none6 = (None,) * 6
    assert offsets(B=0, ids=None, node_ptr=None, edge_ptr=None, seg=None, eoff=None) == 0
    assert nodes(B=0, ids=None, node_ptr=None, seg=None, x=None, y=None, xo=None, bo=None, yo=None, n=0) == 0
    assert edges(B=0, ids=None, edge_ptr=None, eoff=None, seg=None, ed=None, out=None, e=0) == 0
    assert edges(e=0, ids=None, edge_ptr=None, eoff=None, seg=None, ed=None, out=None) == 0       # no edge to copy
    assert csr_offsets(B=0, ids=None, node_ptr=None, rowptr=None, out=None) == 0
    assert csr(B=0, ids=None, node_ptr=None, seg=None, batch=None, noff=None, ins=none6, outs=none6, n=0, nnz=0) == 0
