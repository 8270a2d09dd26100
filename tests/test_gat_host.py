"""GAT edge softmax without a GPU: the float64 yardstick ``brute_gat`` of tests/test_gpu_gat.py -- PyG's single-head
GATConv aggregation on an explicit edge list -- against a dense ``[n, n]`` formulation of the same operation, and the
graphs, inputs and shape lists both files share, with the conditions those inputs have to meet (row lengths on both
sides of every lane-group size, dead rows in the last block at every group size, exact logits, overflowing logits,
module-level logits away from the LeakyReLU kink)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from pygda_amd.nn import GATConv

# on both sides of every pick_group boundary (8 | 16 | 32 | 64); d > G with one, two and five column strides and a
# ragged tail (65, 130, 257 at G = 64)
WIDTHS = [1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 130, 257]
SLOPES = [0.2, 0.0, 1.0]
GROUPS = (8, 16, 32, 64)
REGIMES = ("mild", "wide", "flat")
MODULE_WIDTHS = (8, 32, 128)
MODULE_GRAPHS = ("loops_dups", "powerlaw")
MODULE_IN = 12
PRE_GAP = 1e-3          # module level: the float64 |pre| of every edge stays this far from the LeakyReLU kink
# seeds of module_case for which the float64 run meets PRE_GAP (test_module_inputs_stay_away_from_the_kink)
MODULE_SEEDS = {("loops_dups", 8): 0, ("loops_dups", 32): 0, ("loops_dups", 128): 0,
                ("powerlaw", 8): 0, ("powerlaw", 32): 2, ("powerlaw", 128): 10}


# ---- the yardstick -----------------------------------------------------------------------------------------------------
def brute_gat(h, a_src, a_dst, src, dst, slope, gout):
    """``(out, alpha, gh, ga_src, ga_dst)`` in the dtype of ``h`` on the edge list ``src -> dst`` (duplicates are separate
    softmax entries, as PyG keeps them): ``pre = a_src[src] + a_dst[dst]``, LeakyReLU, a softmax per destination with
    the maximum subtracted (no 1e-16 in the denominator: the kernel adds none), ``out = index_add(alpha * h[src])``;
    ``alpha`` in edge-list order, the gradients from autograd of ``(out * gout).sum()``.  A destination without an
    in-edge has a zero output row and a zero ``ga_dst``."""
    h, a_src, a_dst = (v.detach().clone().requires_grad_(True) for v in (h, a_src, a_dst))
    n, dt = h.size(0), h.dtype
    e = F.leaky_relu(a_src[src] + a_dst[dst], slope)
    m = torch.full((n,), float("-inf"), dtype=dt).scatter_reduce(0, dst, e.detach(), reduce="amax")
    ex = (e - m[dst]).exp()
    alpha = ex / torch.zeros(n, dtype=dt).index_add_(0, dst, ex)[dst]
    out = torch.zeros(n, h.size(1), dtype=dt).index_add_(0, dst, alpha[:, None] * h[src])
    (out * gout.to(dt)).sum().backward()
    return out.detach(), alpha.detach(), h.grad, a_src.grad, a_dst.grad


def dense_gat(h, a_src, a_dst, src, dst, slope, gout):
    """The same operation through an ``[n, n]`` multiplicity matrix ``M`` (``M_ij`` = copies of the edge ``j -> i``):
    ``alpha_ij = M_ij exp(e_ij) / sum_j M_ij exp(e_ij)``, ``out = alpha h``.  Returns ``alpha`` as the matrix."""
    h, a_src, a_dst = (v.detach().clone().requires_grad_(True) for v in (h, a_src, a_dst))
    n = h.size(0)
    M = torch.zeros(n, n, dtype=h.dtype).index_put_((dst, src), torch.ones(src.numel(), dtype=h.dtype), accumulate=True)
    w = M * F.leaky_relu(a_src[None, :] + a_dst[:, None], slope).exp()
    z = w.sum(1, keepdim=True)
    alpha = w / torch.where(z > 0, z, torch.ones_like(z))          # an empty row: 0 / 1
    out = alpha @ h
    (out * gout).sum().backward()
    return out.detach(), alpha.detach(), h.grad, a_src.grad, a_dst.grad, M


# ---- graphs: (n, src, dst), the edge list as the kernels see it (self loops included where there are any) -------------
def with_loops(n, src, dst):
    """What GATConv does to an edge list: existing self loops removed, one appended per node."""
    keep, loop = src != dst, torch.arange(n)
    return n, torch.cat([src[keep], loop]), torch.cat([dst[keep], loop])


def _shuffled(n, src, dst, seed):
    p = torch.randperm(src.numel(), generator=torch.Generator().manual_seed(seed))
    return n, src[p], dst[p]


def ladder():
    """Row ``i`` has exactly ``i`` in-edges, ``i = 0 .. 131``, no self loops: every row length 0, 1, G - 1, G, G + 1 and
    2 G + 3 occurs for every G."""
    n = 132
    dst = torch.cat([torch.full((i,), i, dtype=torch.int64) for i in range(n)])
    src = torch.cat([(i + 1 + torch.arange(i)) % n for i in range(n)])
    return _shuffled(n, src, dst, 1)


def uniform():
    """67 nodes (no multiple of 4, 8, 16 or 32: the last block has dead rows at every G), about 5 in-edges per row, one
    self loop per node."""
    n, g = 67, torch.Generator().manual_seed(2)
    return with_loops(n, torch.randint(0, n, (5 * n,), generator=g), torch.randint(0, n, (5 * n,), generator=g))


def powerlaw():
    """300 nodes: destination 0 with 200 in-edges, source 1 with 200 out-edges (the long transposed row of
    k_gat_bwd_src), two random edges per node, one self loop per node."""
    n, g = 300, torch.Generator().manual_seed(3)
    hub = torch.arange(2, 202)
    src = torch.cat([hub, torch.ones(200, dtype=torch.int64), torch.randint(2, n, (2 * n,), generator=g)])
    dst = torch.cat([torch.zeros(200, dtype=torch.int64), hub, torch.randint(2, n, (2 * n,), generator=g)])
    return _shuffled(*with_loops(n, src, dst), 4)


def loops_dups():
    """The RAW list of a 70-node graph for the module path (which removes the loops and adds one per node): self loops
    in the input, every third edge listed three times, node 5 isolated."""
    n, g = 70, torch.Generator().manual_seed(5)
    src, dst = torch.randint(0, n, (3 * n,), generator=g), torch.randint(0, n, (3 * n,), generator=g)
    keep = (src != 5) & (dst != 5)
    src, dst = src[keep], dst[keep]
    loops = torch.tensor([0, 7, 7, 69])
    return _shuffled(n, torch.cat([src, src[::3], src[::3], loops]), torch.cat([dst, dst[::3], dst[::3], loops]), 6)


def n1():
    return 1, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)


GRAPHS = {"ladder": ladder, "uniform": uniform, "powerlaw": powerlaw, "loops_dups": loops_dups, "n1": n1}
_MADE = {}


def graph(name):
    """The graph ``name`` once (shared, left unchanged)."""
    if name not in _MADE:
        _MADE[name] = GRAPHS[name]()
    return _MADE[name]


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def op_inputs(n, d, regime, seed=0):
    """``(h, a_src, a_dst, gout)`` in float32.  ``a_src`` and ``a_dst`` are multiples of 2^-6 of magnitude at most 64, so
    ``pre = a_src + a_dst`` (at most 13 significant bits) is EXACT in float32 and in float64: the sign of ``pre`` -- the
    LeakyReLU branch -- is the same in both precisions by construction, not by luck.
      mild  magnitudes up to 2
      wide  +-60: ``pre`` passes 88 on some rows (an fp32 softmax without the max subtraction overflows) and other
            edges of those rows underflow to a weight of exactly 0
      flat  ``pre == 0`` on every edge: all logits equal, the LeakyReLU derivative taken AT the kink"""
    g = torch.Generator().manual_seed(1000 * d + 10 * n + seed)
    h, gout = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    if regime == "flat":
        return h, torch.full((n,), 0.75), torch.full((n,), -0.75), gout
    top = {"mild": 2, "wide": 60}[regime] * 64
    a_src, a_dst = (torch.randint(-top, top + 1, (n,), generator=g).float() / 64 for _ in range(2))
    return h, a_src, a_dst, gout


def module_case(name, d):
    """``(conv, x, edge_index, w)`` on the CPU in float32: ``GATConv(12, d)`` with a non-zero bias, its input, the graph
    and the loss weights of ``(out * w).sum()``, from the seed recorded for this case."""
    n, src, dst = graph(name)
    torch.manual_seed(MODULE_SEEDS[name, d])
    conv = GATConv(MODULE_IN, d)
    g = torch.Generator().manual_seed(MODULE_SEEDS[name, d] + 100)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(d, generator=g))
    return conv, torch.randn(n, MODULE_IN, generator=g), torch.stack([src, dst]), torch.randn(n, d, generator=g)


def module_pre(conv, x, edge_index):
    """The float64 ``pre`` of every edge the module aggregates over."""
    c = copy.deepcopy(conv).double()
    _, src, dst = with_loops(x.size(0), edge_index[0], edge_index[1])
    with torch.no_grad():
        h = F.linear(x.double(), c.lin.weight)
        return (h * c.att_src.view(1, -1)).sum(-1)[src] + (h * c.att_dst.view(1, -1)).sum(-1)[dst]


# ---- the yardstick against the dense formulation ---------------------------------------------------------------------------
def _small_graphs():
    g = torch.Generator().manual_seed(7)
    n = 40
    src, dst = torch.randint(0, n, (4 * n,), generator=g), torch.randint(1, n - 1, (4 * n,), generator=g)
    yield n, torch.cat([src, src[:30], src[:30]]), torch.cat([dst, dst[:30], dst[:30]])      # rows 0 and 39 are empty
    yield with_loops(n, src, dst)
    yield n1()
    yield 9, torch.cat([(i + 1 + torch.arange(i)) % 9 for i in range(9)]), \
        torch.cat([torch.full((i,), i, dtype=torch.int64) for i in range(9)])


@pytest.mark.parametrize("slope", SLOPES)
def test_brute_gat_is_the_dense_edge_softmax(slope):
    for case, (n, src, dst) in enumerate(_small_graphs()):
        for d in (1, 5):
            h, a_src, a_dst, gout = (v.double() for v in op_inputs(n, d, "mild", seed=case))
            h, gout = h + 0.1 * torch.randn(n, d, generator=torch.Generator().manual_seed(case), dtype=torch.float64), \
                gout * 1.0000001                                               # not float32 numbers any more
            out, alpha, gh, gs, gd = brute_gat(h, a_src, a_dst, src, dst, slope, gout)
            d_out, d_alpha, d_gh, d_gs, d_gd, M = dense_gat(h, a_src, a_dst, src, dst, slope, gout)
            for name, a, b in (("out", out, d_out), ("alpha", alpha, d_alpha[dst, src] / M[dst, src]),
                               ("gh", gh, d_gh), ("ga_src", gs, d_gs), ("ga_dst", gd, d_gd)):
                err = (a - b).abs().max().item()
                assert err <= 1e-12, f"{name} graph {case} d={d}: {err:.3e}"
            deg = torch.bincount(dst, minlength=n)
            sums = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, alpha)
            assert (sums[deg > 0] - 1).abs().max() <= 1e-12
            assert not out[deg == 0].any() and not gd[deg == 0].any()


def test_brute_gat_derivative_at_the_kink_takes_the_slope_branch():
    """``pre == 0``: torch's LeakyReLU backward tests ``pre > 0``, as the kernel does -- the weight is the slope."""
    n, src, dst = graph("ladder")
    h, a_src, a_dst, gout = op_inputs(n, 8, "flat")
    for dt in (torch.float32, torch.float64):
        _, alpha, _, gs0, gd0 = brute_gat(h.to(dt), a_src.to(dt), a_dst.to(dt), src, dst, 0.0, gout)
        assert not gs0.any() and not gd0.any()
        _, _, _, gs1, gd1 = brute_gat(h.to(dt), a_src.to(dt), a_dst.to(dt), src, dst, 1.0, gout)
        _, _, _, gs2, _ = brute_gat(h.to(dt), a_src.to(dt), a_dst.to(dt), src, dst, 0.2, gout)
        assert gs1.abs().max() > 0.1
        assert gd1.abs().max() < 1e-5          # one derivative for the whole row: sum_k alpha_k (dalpha_k - s) = 0
        torch.testing.assert_close(gs2, 0.2 * gs1, rtol=1e-5, atol=1e-7)
        deg = torch.bincount(dst, minlength=n).to(dt)
        assert torch.equal(alpha, (torch.ones((), dtype=dt) / deg)[dst])


# ---- the conditions on the shared graphs and inputs ------------------------------------------------------------------------
def test_graphs_have_the_rows_the_kernels_can_get_wrong():
    n, src, dst = graph("ladder")
    deg = torch.bincount(dst, minlength=n)
    assert n == 132 and torch.equal(deg, torch.arange(n)) and (src != dst).all()
    for G in GROUPS:
        assert {0, 1, G - 1, G, G + 1, 2 * G + 3} <= set(deg.tolist())
    n, src, dst = graph("uniform")
    assert n == 67 and all(n % (256 // G) for G in GROUPS)                     # dead rows in the last block
    assert ((src == dst).sum() == n) and 4 <= (src.numel() - n) / n <= 5
    n, src, dst = graph("powerlaw")
    assert n == 300 and torch.bincount(dst, minlength=n)[0] == 201 and torch.bincount(src, minlength=n)[1] == 201
    assert all(n % (256 // G) for G in GROUPS[:3]) and (src == dst).sum() == n
    n, src, dst = graph("loops_dups")
    assert (src == dst).sum() >= 4 and not ((src == 5) | (dst == 5)).any() and n % 4
    pairs = (dst * n + src).tolist()
    assert sum(pairs.count(p) >= 3 for p in set(pairs)) >= 20
    _, s2, d2 = with_loops(n, src, dst)
    assert (s2 == d2).sum() == n and torch.bincount(d2, minlength=n)[5] == 1
    assert graph("n1")[0] == 1 and graph("n1")[1].tolist() == [0] and graph("n1")[2].tolist() == [0]


@pytest.mark.parametrize("regime", REGIMES)
def test_op_level_logits_are_exact_in_both_precisions(regime):
    n, src, dst = graph("ladder")
    for d in (8, 16, 32, 130):
        _, a_src, a_dst, _ = op_inputs(n, d, regime)
        for a in (a_src, a_dst):
            assert a.abs().max() <= 64 and torch.equal(a * 64, (a * 64).round())
        pre32, pre64 = a_src[src] + a_dst[dst], a_src.double()[src] + a_dst.double()[dst]
        assert torch.equal(pre32.double(), pre64)
        if regime == "flat":
            assert not pre64.any()
        if regime == "mild":
            assert pre64.abs().max() <= 4 and (pre64 > 0).any() and (pre64 < 0).any()
        if regime == "wide":
            assert pre64.max() > 88.73                                            # exp overflows float32 there
            for slope in SLOPES:
                e = F.leaky_relu(pre64, slope)
                m = torch.full((n,), float("-inf"), dtype=torch.float64).scatter_reduce(0, dst, e, reduce="amax")
                # below exp(-104) float32 has no number left, denormal or not: such weights are 0 on any device
                assert ((e - m[dst]) < -104).sum() >= 10, f"d={d} slope={slope}"
                assert m.max() > 88.73


@pytest.mark.parametrize("name", MODULE_GRAPHS)
@pytest.mark.parametrize("d", MODULE_WIDTHS)
def test_module_inputs_stay_away_from_the_kink(name, d):
    """A condition on the inputs of test_conv_module_against_float64, never a reason to skip a comparison: a seed that
    misses it is replaced in MODULE_SEEDS."""
    conv, x, ei, _ = module_case(name, d)
    pre = module_pre(conv, x, ei)
    assert pre.abs().min() >= PRE_GAP, f"min |pre| = {pre.abs().min():.3e}"
    assert (pre > 0).any() and (pre < 0).any()
