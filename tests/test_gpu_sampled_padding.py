"""GPU: the padded rows of the static-shape sampled A2GNN step (pygda_amd/sampled_graph.py) reach no gradient.

The step runs at a capacity shape: every matrix has ``ncap`` rows, the first ``n_live`` are real.  The module's docstring
promises that the rows behind them "gather some valid feature row", have no entry in either CSR, are never drawn by the
MMD and are masked out of the cross-entropy, "so their gradients are exact zeros and nothing they hold reaches a
parameter".  Here that promise is tested directly:

* the same static-shape steps with three different paddings (tests/_sampled_padding.py::poison_tail: zeros / random valid
  ids and +-1e3 values / every padded row on a node with +-1e3 features) give the same losses, correct counts, parameters
  and Adam moments AS VALUES after every step, eager and captured;
* the gradient rows ``[n_live, ncap)`` of the logits, of both MMD feature matrices and of both layer-0 outputs are exact
  zeros;
* one static-shape step is the right function: loss and every parameter gradient against a float64 real-shape step of
  the CPU oracle on the live rows and edges, beside the ordinary real-shape eager step through the same check;
* two mutations (cross-entropy over all ``ncap`` rows, MMD draws over ``ncap``) are seen by the comparison;
* a GradSink whose activation has a second consumer raises instead of masking a masked gradient again.

Two configurations: G (20 k nodes, F = 64, hidden 32, 64 seeds at fan-out [5, 3]: the general kernels) and T (200 k
nodes, F = 128, hidden 128, 256 seeds at [15, 10]: ~38 k live rows, above ops.TALL_ROWS -- the tall split-fp16 projection
with the gather in its operand fetch, the activation in its epilogue and the masked data gradient, the one-launch
interior K-step), each asserting that its steps really took the static path it is about.
"""
import functools

import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from pygda_amd import sampled_graph as SG
from pygda_amd.data import Data
from pygda_amd.nn.a2gnn_base import ActPair, StackedAct
from tests._sampled_padding import VARIANTS, bound_report, differences, hot_features, oracle_step, poison_tail
from tests.test_gpu_cwgcn import _close
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

CFG = {"G": dict(nodes=20_000, feat=64, hid=32, seeds=64, fan=[5, 3]),
       "T": dict(nodes=200_000, feat=128, hid=128, seeds=256, fan=[15, 10])}
HP = dict(s_pnums=0, t_pnums=10, weight=10, num_layers=2, weight_decay=0)
CLASSES, HOT_LABEL, MIN_PAD = 5, 3, 16
SLACK = 2e-6


@functools.lru_cache(maxsize=None)
def _domains(cfg):
    """Source and target of a configuration, built once per module: bench.make_cfg_s plus ONE isolated node behind the
    graph (id = nodes) with alternating +-1e3 features and a valid label -- the "hot" padding's node.  The seeds are the
    first nodes of the graph and the extra node has no edge, so no live row ever holds it."""
    from bench import make_cfg_s
    c = CFG[cfg]
    out = []
    for seed in (200, 201):
        d = make_cfg_s(c["nodes"], 20, c["feat"], CLASSES, seed, DEV)
        x = torch.cat([d.x, hot_features(c["feat"]).to(DEV).view(1, -1)])
        y = torch.cat([d.y, torch.tensor([HOT_LABEL], device=DEV, dtype=d.y.dtype)])
        out.append(Data(x=x, edge_index=d.edge_index, y=y))
    return tuple(out)


@pytest.fixture(scope="module", autouse=True)
def _release_domains():
    yield
    _domains.cache_clear()                             # the graphs stay on the device for this module only


def _install_hooks(m, net, got):
    """Tensor hooks (they return None and add no consumer) on the source logits, on both MMD feature matrices and on both
    domains' layer-0 outputs: ``got[name] = (layout, gradient)``."""
    def hook(t, name, layout="rows"):
        if torch.is_grad_enabled() and t.requires_grad:
            t.register_hook(lambda g: got.__setitem__(name, (layout, g.detach().clone())))

    first_conv, source_branch, domain_loss = net.first_conv, m._source_branch, m._domain_loss

    def first_conv_hooked(x, edge_index, prop_nums, draws=0):
        h = first_conv(x, edge_index, prop_nums, draws=draws)
        name = "layer0_source" if prop_nums <= 0 else "layer0_target"
        if isinstance(h, StackedAct):
            hook(h.y, name, "stacked")                # the two source passes' rows, one block behind the other
        elif isinstance(h, ActPair):
            hook(h.draws[0], name)
        elif isinstance(h, ops.ColMajor):
            hook(h.t, name, "colmajor")
        else:
            hook(h, name)
        return h

    def source_branch_hooked(source_data):
        loss, logits, feats = source_branch(source_data)
        hook(logits, "logits_source")
        return loss, logits, feats

    def domain_loss_hooked(loss, source_features, target_features, alpha):
        hook(source_features, "features_source")
        hook(target_features, "features_target")
        return domain_loss(loss, source_features, target_features, alpha)

    net.first_conv, m._source_branch, m._domain_loss = first_conv_hooked, source_branch_hooked, domain_loss_hooked


def _run(cfg, *, variant=None, capture=False, static=True, steps=1, dropout=0.5, hooks=False, mutate=None):
    """``steps`` sampled steps of a fresh trainer (same seeds, same dropout counter reset as
    tests/test_gpu_sampler.py::_sampled_fit) -> the record :func:`tests._sampled_padding.differences` compares, plus what
    the preconditions need.  ``variant``: the padding, rewritten by a wrapper around ``_StaticBatch.load`` after the ring
    block was copied in (outside the capture).  ``static=False``: the ordinary eager loop on the real shapes."""
    c = CFG[cfg]
    src, tgt = _domains(cfg)
    rec = dict(loss=[], correct=[], param=[], exp_avg=[], exp_avg_sq=[], pad=[], draws=[], hooks={})
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PYGDA_AMD_SAMPLED_GRAPH", "1" if static else "0")
        mp.setenv("PYGDA_AMD_SAMPLED_GRAPH_CAPTURE", "1" if capture else "0")
        m = pygda_amd.models.A2GNN(c["feat"], c["hid"], CLASSES, dropout=dropout, lr=0.005, device=DEV, epoch=1,
                                   verbose=0, batch_size=c["seeds"], num_neigh=c["fan"], **HP)
        torch.manual_seed(1)
        ops.dropout_state.counter(torch.device(DEV)).zero_()
        ops.dropout_state.seed = 12345
        net, optimizer, step, alpha = m._prepare(src, tgt)
        for loader in (m.source_loader, m.target_loader):
            loader.input_nodes = loader.input_nodes[:steps * c["seeds"]]
        named = dict(net.named_parameters())
        rec["state0"] = {k: v.detach().clone() for k, v in net.state_dict().items()}

        def snapshot():
            torch.cuda.synchronize()
            rec["param"].append({k: p.detach().clone() for k, p in named.items()})
            for what in ("exp_avg", "exp_avg_sq"):
                rec[what].append({k: optimizer.state[p][what].detach().clone() for k, p in named.items()})

        load, step_static, randint = SG._StaticBatch.load, SG.GraphedSampledStep.step, torch.randint

        def load_poisoned(self, slot, sizes, stream_handle):
            load(self, slot, sizes, stream_handle)
            if variant is not None:
                poison_tail(self, variant, hot=c["nodes"], seed=7)

        def step_recorded(self, slot_s, sizes_s, slot_t, sizes_t):
            ticket = step_static(self, slot_s, sizes_s, slot_t, sizes_t)
            if ticket is not None:
                torch.cuda.synchronize()
                loss, correct, _ = self.result(ticket)
                rec["loss"].append(loss)
                rec["correct"].append(correct)
                rec["pad"].append((self.static[0].ncap - sizes_s[0], self.static[1].ncap - sizes_t[0]))
                snapshot()
            return ticket

        def randint_recorded(*args, **kw):
            out = randint(*args, **kw)
            if len(args) == 2 and isinstance(args[0], int) and len(tuple(args[1])) == 2:      # an MMD draw [times, n]
                rec["draws"].append((args[0], out.clone()))
            return out

        mp.setattr(SG._StaticBatch, "load", load_poisoned)
        mp.setattr(SG.GraphedSampledStep, "step", step_recorded)
        mp.setattr(torch, "randint", randint_recorded)
        for target, name, value in (mutate or ()):
            mp.setattr(target, name, value)
        if hooks:
            _install_hooks(m, net, rec["hooks"])
        seen = []
        m.epoch_hook = lambda e, loss, acc, secs: seen.append(loss)
        hits = ops.sink_hits
        torch.manual_seed(77)                      # the CPU generator the MMD draws come from
        m._train_epochs(net, optimizer, step, alpha)
        torch.cuda.synchronize()
        rec["sink_hits"] = ops.sink_hits - hits
    st = rec["stepper"] = (getattr(m, "_sampled_graphed", None) or (None, None))[1]
    rec["model"], rec["net"] = m, net
    if static:
        assert st is not None and st.replays == steps and st.fallbacks == 0, (getattr(st, "replays", None), steps)
        assert (st.graph is not None) == capture
        assert len(rec["loss"]) == steps
        for pad in rec["pad"]:
            assert min(pad) >= MIN_PAD, rec["pad"]       # there IS padding in every compared batch, both domains
    else:
        assert st is None and steps == 1 and len(seen) == 1
        rec["loss"].append(seen[0])
        snapshot()
    return rec


def _assert_tall_path(rec):
    """T's preconditions: the steps ran the kernels the configuration is about."""
    st, net = rec["stepper"], rec["net"]
    for sb in st.static:
        assert sb.ncap >= ops.TALL_ROWS and sb.live[0] >= ops.TALL_ROWS, (sb.ncap, sb.live)
        assert ops.tall_fused_ok(ops.GatheredRows(sb.loader.data.x, sb.nodes), net.convs[0].lin.weight)
    assert rec["sink_hits"] > 0
    assert any(kind == "interior-lds" for _, _, kind in st.template), st.template


def _same_under_every_padding(cfg, capture, steps=3):
    runs = {v: _run(cfg, variant=v, capture=capture, steps=steps) for v in VARIANTS}
    print(f"\n{cfg} capture={capture}: padded rows (source, target) per step {runs['zero']['pad']}, "
          f"losses {runs['zero']['loss']}")
    for v in VARIANTS[1:]:
        assert runs[v]["pad"] == runs["zero"]["pad"]
        d = differences(runs["zero"], runs[v])
        assert not d, f"{cfg}: padding 'zero' against {v!r}: " + "; ".join(d[:8])
    assert all(np.isfinite(runs["hot"]["loss"]))
    return runs


@pytest.mark.parametrize("capture", [False, True])
def test_general_static_steps_do_not_depend_on_their_padding(capture):
    """G: three static-shape steps (dropout 0.5: the masks are keyed on the element index and ``ncap`` is the
    same in all runs), eager and captured, under the three paddings: every step's loss and correct count, every parameter
    and both Adam moments after every step are equal as values.  ``exp_avg`` after the first step is (1 - beta1) x the
    TOTAL gradient (second-leaf sums included), readable after a replay that ran no Python.  No tolerance."""
    _same_under_every_padding("G", capture)


def test_tall_static_steps_do_not_depend_on_their_padding():
    """T, captured: the tall fused projections (gather in the operand fetch, activation in the epilogue, masked
    data gradient), the gathered weight gradient and the one-launch interior K-step at the padded shape."""
    runs = _same_under_every_padding("T", True)
    for r in runs.values():
        _assert_tall_path(r)


def _pad_and_live(layout, g, n, ncap):
    if layout == "stacked":
        v = g.view(2, ncap, -1)
        return v[:, n:], v[:, :n]
    if layout == "colmajor":
        return g[:, n:ncap], g[:, :n]
    assert g.size(0) == ncap, (tuple(g.shape), ncap)
    return g[n:], g[:n]


@pytest.mark.parametrize("cfg", ["G", "T"])
def test_gradient_rows_behind_the_live_ones_are_exact_zeros(cfg):
    """One eager static-shape step under the "hot" padding (every padded row gathers +-1e3 features): the
    gradient rows [n_live, ncap) of the source logits, of the source and target features the MMD reads and of both
    domains' layer-0 outputs are exactly zero, while the live rows are not.  The hooks sit on the activation outputs
    themselves, sinked ones included: a tensor hook that returns None hands the sink's buffer on untouched, and the step
    counts the same ``sink_hits`` with the hooks as without (asserted)."""
    plain = _run(cfg, variant="hot", hooks=False)
    rec = _run(cfg, variant="hot", hooks=True)
    assert rec["sink_hits"] == plain["sink_hits"] > 0, (rec["sink_hits"], plain["sink_hits"])
    assert not differences(plain, rec)
    if cfg == "T":
        _assert_tall_path(rec)
    st = rec["stepper"]
    want = {"logits_source": 0, "features_source": 0, "layer0_source": 0, "features_target": 1, "layer0_target": 1}
    assert set(rec["hooks"]) == set(want), sorted(rec["hooks"])
    for name, dom in want.items():
        layout, g = rec["hooks"][name]
        sb = st.static[dom]
        pad, live = _pad_and_live(layout, g, sb.live[0], sb.ncap)
        print(f"{cfg} {name} [{layout}] {tuple(g.shape)}: {sb.ncap - sb.live[0]} padded rows, max |g| padded "
              f"{float(pad.abs().max()):.3e} live {float(live.abs().max()):.3e}")
        assert pad.numel() > 0
        assert float(pad.abs().max()) == 0.0, name
        assert float(live.abs().max()) > 0.0 and bool(torch.isfinite(live).all()), name


def _live_batch(sb):
    n, e = sb.live[0], sb.live[1]
    data, nodes = sb.loader.data, sb.nodes[:n]
    return data.x[nodes].cpu(), sb.ei[:, :e].cpu().clone(), data.y[nodes].cpu()


def _gradients(rec):
    """Every parameter's total gradient of a run's ONE step, recovered from Adam's fresh first moment:
    exp_avg = g * (1.0f - beta1) in fp32 (csrc/gda_adam_rule.h)."""
    c = float(np.float32(1.0) - np.float32(0.9))
    return {k: v.double().cpu() / c for k, v in rec["exp_avg"][0].items()}


@pytest.mark.parametrize("cfg", ["G", "T"])
def test_the_static_step_is_the_real_shape_step_against_float64(cfg):
    """One eager static-shape step, dropout 0, against ``oracle.pygda_cpu.a2gnn_forward_model`` in float64 on
    the batch's live rows and live edges with the step's own 5 x 1000 MMD draws (seeded CPU generator, recorded as the
    step made them): the loss and every parameter gradient within tests/test_gpu_cwgcn._close's bound,
    |gpu - f64| <= 8 |oracle fp32 - f64| + 2e-6 max|f64| -- and the ordinary real-shape eager step
    (PYGDA_AMD_SAMPLED_GRAPH=0) on the same batch and draws through the same check, which tells a padding problem from a
    kernel-accuracy one.  The figures are printed before anything asserts.  Where the real-shape step itself misses the
    bound for a tensor, the static step is held to twice the real-shape step's own distance from float64 plus the same
    slack (the same kernels on the same live operands, another slab split).

    Measured (MI355X): no tensor needs that rule.  G, 1236 / 1209 live rows of 1280: loss 2.4e-7 off float64 (limit
    5.4e-6), gradients between 2.0e-8 and 1.3e-7 (limits 3.0e-7 .. 1.6e-6), static and real-shape step identical in every
    figure.  T, 35658 / 36033 live rows of 36352 / 36608: loss 1.2e-7 (limit 5.2e-6); layer 0's weight gradient 1.59e-6,
    the fp32 oracle's own 1.59e-6 (limit 1.27e-5); the other gradients 1.1e-8 .. 6.4e-7, the static step within 1.4 x the
    real-shape step's distance everywhere.  T's case takes ~30 s, ~25 s of them the oracle's [2000, 2000, 128] MMD
    temporaries in float64 and float32 on the host; the GPU part is well under a second."""
    c = CFG[cfg]
    stat = _run(cfg, dropout=0.0)
    real = _run(cfg, dropout=0.0, static=False)
    st = stat["stepper"]
    if cfg == "T":
        for sb in st.static:
            assert sb.ncap >= ops.TALL_ROWS and sb.live[0] >= ops.TALL_ROWS
    live = (st.static[0].live[0], st.static[1].live[0])
    draws, draws_real = stat["draws"][-2:], real["draws"][-2:]
    assert [d[0] for d in draws] == list(live) == [d[0] for d in draws_real], (live, [d[0] for d in draws])
    for (_, a), (_, b), n in zip(draws, draws_real, live):
        assert torch.equal(a, b) and tuple(a.shape) == (5, 1000) and 0 <= int(a.min()) and int(a.max()) < n
    assert all(torch.equal(v, real["state0"][k]) for k, v in stat["state0"].items())
    want = oracle_step(stat["state0"], (c["feat"], c["hid"], CLASSES, HP["num_layers"]),
                       _live_batch(st.static[0]), _live_batch(st.static[1]), (draws[0][1], draws[1][1]),
                       HP["s_pnums"], HP["t_pnums"], HP["weight"])
    (l64, g64), (l32, g32) = want[torch.float64], want[torch.float32]
    gs, gr = _gradients(stat), _gradients(real)
    assert set(gs) == set(g64)
    print(f"\n{cfg}: live rows {live}, padded rows {stat['pad'][0]}, loss f64 {float(l64):.9f}")
    figures = {}
    for name, s, r, f32, f64 in [("loss", stat["loss"][0], real["loss"][0], l32, l64)] + \
                                [(k, gs[k], gr[k], g32[k], g64[k]) for k in g64]:
        e_s, e_ref, lim = bound_report(f"static {name}", s, f32, f64, SLACK)
        e_r, _, _ = bound_report(f"real   {name}", r, f32, f64, SLACK)
        figures[name] = (e_s, e_r, lim, float(f64.abs().max()))
    for name, s, f32, f64 in [("loss", stat["loss"][0], l32, l64)] + [(k, gs[k], g32[k], g64[k]) for k in g64]:
        e_s, e_r, lim, top = figures[name]
        if e_r <= lim:
            _close(s, f32, f64, f"{cfg} static {name}", SLACK)
        else:
            assert e_s <= 2 * e_r + SLACK * top, f"{cfg} static {name}: {e_s:.3e} > 2 x {e_r:.3e} + slack (limit {lim:.3e})"


def _ce_over_every_row(self):
    """Mutation: ``_StaticBatch.materialise`` without the ``_gda_valid_rows`` tag -- the cross-entropy then runs over all
    ``ncap`` rows (every index stays in range)."""
    d = _MATERIALISE(self)
    if d.y is not None:
        d.y = self.loader.data.y[self.nodes]
    return d


def _draw_over_ncap(self, key):
    """Mutation: ``GraphedSampledStep._fill_one`` drawing the MMD rows over ``ncap`` instead of the live counts."""
    from pygda_amd.hipgraph import _ship
    ns, nt, times, n = key[:4]
    e = self._samples[key]
    k = e["turn"]
    e["turn"] = 1 - k
    if e["done"][k] is not None:
        e["done"][k].synchronize()
    pins = e["pinv"][k]
    torch.randint(self.static[0].ncap, (times, n), out=pins[0])
    torch.randint(self.static[1].ncap, (times, n), out=pins[1])
    ops.selection_csr_host(pins[0], ns, 0, 2 * n, out=(pins[2], pins[3]))
    ops.selection_csr_host(pins[1], nt, n, 2 * n, out=(pins[4], pins[5]))
    _ship(e["dev"], e["pin"][k])
    ev = torch.cuda.Event()
    ev.record()
    e["done"][k] = ev


_MATERIALISE = SG._StaticBatch.materialise


@pytest.mark.parametrize("mutation", ["ce_over_ncap", "mmd_over_ncap"])
def test_the_comparison_sees_a_leak(mutation):
    """Negative controls on G (eager static, one step): with the cross-entropy over all ``ncap`` rows, or the
    MMD drawing over ``ncap``, the comparison of the padding tests reports a difference between the "zero" and the "hot" padding,
    in at least one parameter's ``exp_avg``.  Both mutations keep every index in range: they change numbers only."""
    mutate = [(SG._StaticBatch, "materialise", _ce_over_every_row)] if mutation == "ce_over_ncap" else \
        [(SG.GraphedSampledStep, "_fill_one", _draw_over_ncap)]
    runs = {v: _run("G", variant=v, mutate=mutate) for v in ("zero", "hot")}
    d = differences(runs["zero"], runs["hot"])
    print(f"\n{mutation}: {len(d)} differences, e.g. {d[:3]}")
    assert any("exp_avg[" in s for s in d), d
    assert SG._StaticBatch.materialise is _MATERIALISE                     # the mutation is gone again


def test_a_grad_sink_whose_activation_has_a_second_consumer_raises():
    """ADVICE round 6, pygda_amd/ops.py GradSink.mine: inside ``grad_sinks()`` an activation output
    ``y = relu_dropout(x [64, 8], 0.5)`` feeds a sink-writing consumer -- the sampled MMD against a fixed ``t [64, 8]``,
    whose gradient scatter stores the masked gradient in the sink -- AND a plain torch one, ``(y * w).sum()``.  Autograd
    sums the sink's buffer (masked and scaled by 1 / (1 - p) already) with the other gradient into a fresh tensor; before
    the guard the ordinary backward masked and scaled that sum again.  Measured on this very computation against
    ``ops.GRAD_SINKS = False`` before the fix: the gradient of ``x`` came out with the whole MMD part added a second time
    -- relative L2 error 0.0664 (= |MMD part| / |gradient|), largest entry off by 0.17 max|gradient| -- silently.  Now
    ``backward()`` raises ``GdaError`` naming the sink; a single consumer still counts a ``sink_hit`` and gives the
    sink-less gradient bit for bit.

    (``ops.mmd_loss(y, t)`` on the rows as given has no selection CSRs and never writes a sink; the sampled form,
    ``utils.MMD`` with its row draws, is the one the trainer calls and the one used here.  A projection of 64 rows does not
    write one either: nn.linear.Linear reshapes inputs below 1024 rows, and the view carries no sink.)"""
    from pygda_amd.utils import MMD
    gen = torch.Generator().manual_seed(3)
    x0 = torch.randn(64, 8, generator=gen).to(DEV)
    t0 = torch.randn(64, 8, generator=gen).relu().to(DEV)
    w = torch.randn(64, 8, generator=gen).to(DEV)
    st = ops.dropout_state
    st.next_step(torch.device(DEV))

    def grad(sinks, second):
        x = x0.clone().requires_grad_()
        st.site = 2
        with (ops.grad_sinks() if sinks else torch.enable_grad()):
            y = ops.relu_dropout(x, 0.5, True)
            assert (ops.sink_of(y) is not None) == sinks
            torch.manual_seed(5)
            total = MMD(y, t0, sampling_num=32, times=2, scale=10.0)
        if second:
            total = total + (y * w).sum()
        total.backward()
        return x.grad

    hits = ops.sink_hits
    one = grad(True, False)
    assert ops.sink_hits - hits == 1                                        # the single consumer: the epilogue path
    assert torch.equal(one, grad(False, False)) and float(one.abs().max()) > 0
    want = grad(False, True)
    assert not torch.equal(want, one)
    hits = ops.sink_hits
    with pytest.raises(_lib.GdaError, match="GradSink"):
        grad(True, True)
    assert ops.sink_hits == hits
    # the protocol is intact afterwards
    assert torch.equal(one, grad(True, False))
