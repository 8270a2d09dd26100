"""GPU: graph-mode epochs over two ``GraphStore``s that draw every graph in one batch, captured with their collation and
replayed (``hipgraph.GraphedStoreStep``).  A captured fit must give, bit for bit, what the same fit gives eagerly from
the same stores -- per-epoch losses and accuracies, ``predict`` on both domains, and the state both host generators are
left in -- and what the list path gives wherever lists and stores already agree; every input the capture does not
cover keeps today's eager epochs."""
import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import ops
from pygda_amd.data import GraphStore
from tests.conftest import load_golden, sub
from tests.test_gpu_graph_mode import _dataset, _zero_dropouts
from tests.test_gpu_parity import DEV, LOGIT_ATOL, REL, close, exact

pytestmark = pytest.mark.gpu

EPOCHS = 6
TAGS = ["a2gnn_mmd", "grade_js", "grade_mmd", "udagcn_ppmi", "udagcn", "adagcn"]


def _trainer(tag, dropout=0.0, **kw):
    M = pygda_amd.models
    kw = dict(dict(device=DEV, epoch=EPOCHS, verbose=0, batch_size=0), **kw)
    if tag.startswith("a2gnn"):
        return M.A2GNN(10, 16, 3, mode='graph', num_layers=2, dropout=dropout, s_pnums=0, t_pnums=5, weight=0.5, lr=0.01,
                       weight_decay=0.001, adv=tag == "a2gnn_adv", **kw)
    if tag.startswith("grade"):
        return M.GRADE(10, 8, 3, mode='graph', num_layers=2, dropout=dropout, disc=tag[6:].upper(), weight=0.5, lr=0.01,
                       weight_decay=0.001, **kw)
    if tag == "adagcn":
        return M.AdaGCN(10, 8, 3, mode='graph', num_layers=2, dropout=dropout, adv_dim=6, gp_weight=5, domain_weight=1, lr=0.01,
                        weight_decay=0.001, **kw)
    return M.UDAGCN(10, 8, 3, mode='graph', num_layers=2, dropout=dropout, ppmi=tag == "udagcn_ppmi", adv_dim=6, lr=0.01,
                    weight_decay=0.003, **kw)


_golden = {}


def _domains():
    if not _golden:
        g = load_golden("graph_trainers")
        _golden["d"] = (_dataset(g, "src"), _dataset(g, "tgt"))
    return _golden["d"]


def _inputs(tag, kind, domains=None):
    src, tgt = domains or _domains()
    if kind == "list":
        return src, tgt
    ppmi = "per_graph" if tag == "udagcn_ppmi" and kind != "per_batch" else "per_batch"
    dev = "cpu" if kind == "cpu" else DEV
    return tuple(GraphStore(gs, dev) if dev == "cpu" else GraphStore(gs, dev, ppmi=ppmi) for gs in (src, tgt))


def _same_np(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _fit(m, data, seed=21):
    """A seeded fit and both predictions: everything a run leaves behind, on the host."""
    seen = []
    m.epoch_hook = lambda e, loss, acc, secs: seen.append((float(loss), float(acc)))
    ops.dropout_state.counter(torch.device(DEV)).zero_()          # the keep-bit stream of step 1, for every run
    torch.manual_seed(seed)
    np.random.seed(seed + 1)
    m.fit(*data)
    rng = (torch.get_rng_state(), np.random.get_state())
    tl, ty = m.predict(data[1])
    sl, sy = m.predict(data[0], source=True)
    return dict(log=seen, rng=rng, pred=[t.cpu() for t in (tl, ty, sl, sy)])


def _assert_same_run(a, b, rng=True):
    assert a["log"] == b["log"] and len(a["log"]) > 0 and all(np.isfinite(l) for l, _ in a["log"])
    for x, y in zip(a["pred"], b["pred"]):
        assert x.dtype == y.dtype and torch.equal(x, y)
    if rng:
        assert torch.equal(a["rng"][0], b["rng"][0]) and _same_np(a["rng"][1], b["rng"][1])


@pytest.mark.parametrize("tag", TAGS)
def test_a_captured_fit_equals_the_eager_fit_bit_for_bit(monkeypatch, tag):
    _zero_dropouts(monkeypatch)
    runs = {}
    for kind, graph in (("store", True), ("store", False), ("list", False)):
        m = _trainer(tag, use_hip_graph=graph)
        runs[kind, graph] = _fit(m, _inputs(tag, kind))
        assert (m._graphed is not None) == graph, (kind, graph)
    assert len(runs["store", True]["log"]) == EPOCHS
    _assert_same_run(runs["store", True], runs["store", False])
    if tag != "udagcn_ppmi":                  # (walks drawn once per graph: other walks than a list's, by design)
        _assert_same_run(runs["store", True], runs["list", False])


@pytest.mark.parametrize("tag", ["a2gnn_mmd", "grade_js", "udagcn_ppmi", "adagcn"])
def test_with_dropout_on_both_runs_mask_with_the_same_keep_bits(monkeypatch, tag):
    runs = []
    for graph in (True, False):
        m = _trainer(tag, dropout=0.4, use_hip_graph=graph)
        runs.append(_fit(m, _inputs(tag, "store")))
        assert (m._graphed is not None) == graph
    _assert_same_run(*runs)
    _zero_dropouts(monkeypatch)                                   # (UDAGCN's discriminator has a Dropout of its own)
    plain = _fit(_trainer(tag, dropout=0.0, use_hip_graph=False), _inputs(tag, "store"))
    assert plain["log"] != runs[0]["log"]                         # the masks were live


def test_captured_stores_reproduce_the_reference_golden():
    g = load_golden("a2gnn_graph_fit3_b0")
    src, tgt = _dataset(g, "src"), _dataset(g, "tgt")
    m = pygda_amd.models.A2GNN(10, 16, 3, mode='graph', num_layers=2, dropout=0.0, s_pnums=0, t_pnums=5, weight=0.5,
                               lr=0.01, weight_decay=0.001, device=DEV, epoch=3, verbose=0, batch_size=0, use_hip_graph=True)
    seen = []
    m.epoch_hook = lambda e, loss, acc, secs: seen.append((loss, acc))
    torch.manual_seed(int(g["seed"]))
    m.fit(GraphStore(src, DEV), GraphStore(tgt, DEV))
    assert m._graphed is not None
    close([x[0] for x in seen], g["losses"], rtol=REL)
    close([x[1] for x in seen], g["accs"], rtol=0, atol=1e-12)
    for k, v in sub(g, "final/").items():
        close(m.a2gnn.state_dict()[k], v, rtol=1e-3, atol=2e-4)
    logits, labels = m.predict(tgt)
    close(logits, g["tgt_logits"], rtol=0, atol=LOGIT_ATOL)
    exact(labels, g["tgt_labels"])
    exact(logits.argmax(1), g["tgt_logits"].argmax(1))


@pytest.mark.parametrize("case", ["list", "cpu", "batch_size", "per_batch", "switched_off", "environment"])
def test_what_the_capture_does_not_cover_stays_eager(monkeypatch, case):
    _zero_dropouts(monkeypatch)
    tag = "udagcn_ppmi" if case == "per_batch" else "grade_js"
    kw = dict(batch_size=4) if case == "batch_size" else {}
    kw["use_hip_graph"] = False if case == "switched_off" else None
    if case == "environment":
        monkeypatch.setenv("PYGDA_AMD_HIPGRAPH", "0")
    kind = case if case in ("list", "cpu", "per_batch") else "store"
    got = _fit(_trainer(tag, epoch=3, **kw), _inputs(tag, kind))
    m = _trainer(tag, epoch=3, **dict(kw, use_hip_graph=False))
    want = _fit(m, _inputs(tag, kind))
    assert m._graphed is None and len(want["log"]) == 3
    _assert_same_run(got, want)
    m = _trainer(tag, epoch=3, **kw)
    _fit(m, _inputs(tag, kind))
    assert m._graphed is None


def test_the_adversarial_a2gnn_is_still_undefined_in_graph_mode():
    for graph in (True, None, False):
        with pytest.raises(ValueError, match="adv=True is not defined for mode='graph'"):
            _trainer("a2gnn_adv", use_hip_graph=graph).fit(*_inputs("a2gnn_adv", "store"))


def test_a_second_fit_captures_again_and_matches_eager():
    runs = []
    for graph in (True, False):
        m, data = _trainer("a2gnn_mmd", use_hip_graph=graph), _inputs("a2gnn_mmd", "store")
        first = _fit(m, data, seed=5)
        held = m._graphed
        second = _fit(m, data, seed=6)
        assert (m._graphed is not None) == graph and (not graph or m._graphed is not held)
        runs.append((first, second))
    (cf, cs), (ef, es) = runs
    _assert_same_run(cf, ef)
    _assert_same_run(cs, es)
    assert cf["log"] != cs["log"]


def test_the_replays_take_the_loaders_draws_and_nothing_else():
    """Per epoch the eager loop's four draws (two base seeds, two sampler seeds) in its order: the ids a replay collates
    are the ids ``zip(source_loader, target_loader)`` would have handed out."""
    tag = "grade_js"
    m = _trainer(tag, use_hip_graph=True)
    data = _inputs(tag, "store")
    torch.manual_seed(33)
    m.fit(*data)
    after = torch.get_rng_state()
    shipped = [ids.cpu().tolist() for ids in m._graphed.ids]
    torch.manual_seed(33)
    m.grade = m.init_model()                                    # (fit draws the initial weights first)
    for _ in range(EPOCHS):
        its = [l.id_batches() for l in (m.source_loader, m.target_loader)]
        last = [next(it) for it in its]
    assert shipped == last and sorted(shipped[0]) == list(range(len(data[0])))
    assert torch.equal(after, torch.get_rng_state())


def test_a_data_parallel_run_over_stores_stays_eager(monkeypatch):
    """A one-rank RCCL group makes the run data-parallel (as ``test_gpu_parity.test_dp_path_single_rank_nccl`` sets it up):
    no store epoch is captured -- a captured step would hold no gradient all-reduce -- and with one rank the eager
    data-parallel epochs reproduce the single-process ones (that test's tolerances)."""
    import socket
    import torch.distributed as dist
    _zero_dropouts(monkeypatch)
    tag = "grade_js"
    base = _fit(_trainer(tag, epoch=3, use_hip_graph=False), _inputs(tag, "store"))
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1"); monkeypatch.setenv("MASTER_PORT", str(port))
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        monkeypatch.setenv("PYGDA_AMD_FORCE_DP", "1")
        from pygda_amd import distributed as D
        assert D.active()
        m = _trainer(tag, epoch=3, use_hip_graph=None)
        got = _fit(m, _inputs(tag, "store"))
        assert m._graphed is None
    finally:
        dist.destroy_process_group()
    assert len(got["log"]) == 3
    close([l for l, _ in got["log"]], np.array([l for l, _ in base["log"]]), rtol=1e-5)
    assert [a for _, a in got["log"]] == [a for _, a in base["log"]]
    close(got["pred"][0], base["pred"][0].numpy(), rtol=0, atol=1e-5)
    assert torch.equal(got["pred"][1], base["pred"][1])


def test_cwgcn_keeps_its_own_loop_over_stores():
    runs = []
    for graph in (None, False):
        m = pygda_amd.models.CWGCN(in_dim=10, hid_dim=8, num_classes=3, mode='graph', gnn="gcn", lr=0.01, weight_decay=0.001,
                                   device=DEV, epoch=2, verbose=0, batch_size=0, use_hip_graph=graph)
        seen = []
        m.epoch_hook = lambda e, loss, acc, secs: seen.append((float(loss), float(acc)))
        torch.manual_seed(9)
        np.random.seed(10)
        m.fit(*_inputs("cwgcn", "store"))
        assert getattr(m, "_graphed", None) is None
        runs.append(seen)
    assert runs[0] == runs[1] and len(runs[0]) > 0


def test_a_store_with_a_long_row_stays_eager_without_a_word(monkeypatch, recwarn):
    """A row beyond twice the long-row threshold sizes its layout with a read-back per batch, which no capture can hold:
    found at the first warm-up step, rolled back, eager epochs with the eager run's numbers -- also when the capture was
    asked for by name."""
    from pygda_amd.data import Data
    from pygda_amd.graph import SPLIT_THRESHOLD
    _zero_dropouts(monkeypatch)
    n = 2 * SPLIT_THRESHOLD + 8
    hub = torch.arange(1, n)
    star = Data(x=torch.randn(n, 10, generator=torch.Generator().manual_seed(4)),
                edge_index=torch.stack([torch.cat([hub, torch.zeros_like(hub)]), torch.cat([torch.zeros_like(hub), hub])]),
                y=torch.tensor([1]))
    src, tgt = _domains()
    domains = (list(src) + [star], tgt)
    runs = []
    for graph in (True, None, False):
        m = _trainer("grade_js", epoch=3, dropout=0.3, use_hip_graph=graph)
        runs.append(_fit(m, _inputs("grade_js", "store", domains)))
        assert m._graphed is None
    assert not [w for w in recwarn.list if "capture" in str(w.message)]
    _assert_same_run(runs[0], runs[2])
    _assert_same_run(runs[1], runs[2])
