"""The GAT edge-softmax kernels (csrc/gda_gat.hip: k_gat_fwd, k_gat_bwd_dst, k_gat_bwd_src) on the MI355X against the
float64 yardstick of tests/test_gat_host.py under the project's bound, at every lane-group size (G = 8, 16, 32, 64), with
the columns strided over the group (d > G, ragged tails), rows shorter and longer than the group, empty rows, dead rows
in the last block, logits an unshifted softmax overflows on, the LeakyReLU derivative at the kink, two runs bit for bit,
the GATConv module against the host composition, and the refusals of the wrapper and of the C entry points."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from pygda_amd import _lib
from pygda_amd.graph import build_csr
from pygda_amd.nn import GATConv
from pygda_amd.nn.gat_conv import _GatAggregate
from pygda_amd.nn.host import _host_conv
from tests.test_gat_host import MODULE_GRAPHS, MODULE_WIDTHS, REGIMES, SLOPES, WIDTHS, brute_gat, graph, module_case, op_inputs
from tests.test_gpu_cwgcn import _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("out", "alpha", "gh", "ga_src", "ga_dst")


def close(gpu, f32, f64, name):
    """The project's bound, |gpu - f64| <= 8 |fp32 torch - f64| + 2e-6 max|f64|, the figures printed first."""
    a, b, c = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64) for v in (gpu, f32, f64))
    e_gpu, e_ref, top = np.abs(a - c).max(), np.abs(b - c).max(), np.abs(c).max()
    print(f"{name}: |gpu - f64| = {e_gpu:.3e}, |fp32 torch - f64| = {e_ref:.3e}, max|f64| = {top:.3e}, "
          f"ratio {e_gpu / (8 * e_ref + 2e-6 * max(top, 1e-30)):.3f}")
    _close(gpu, f32, f64, name)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_DEVICE_GRAPHS = {}


def device_graph(name):
    """``(graph, pos, row, deg)``: the CSR built as nn/gat_conv._gat_graph builds it (a list without self loops -- the
    ladder -- is ingested as it is), the CSR position of every edge-list entry (copies of one edge, whose weights are
    equal, in any order), the row of every CSR entry and the row lengths.  Built once per graph."""
    if name not in _DEVICE_GRAPHS:
        n, src, dst = graph(name)
        loops = src == dst
        if loops.any():                               # one loop per node: what the module's graph removes and appends
            assert torch.equal(torch.bincount(src[loops], minlength=n), torch.ones(n, dtype=torch.int64))
        ei = torch.stack([src[~loops], dst[~loops]]).to(DEV)
        g = build_csr(ei, n, None, False, bool(loops.any()), False, "col", with_edge_map=True)
        rowptr = g.rowptr.cpu().long()
        deg = rowptr[1:] - rowptr[:-1]
        assert int(rowptr[n]) == src.numel()
        col = g.colidx[:src.numel()].cpu().long()
        row = torch.repeat_interleave(torch.arange(n), deg)
        a, b = torch.argsort(row * n + col, stable=True), torch.argsort(dst * n + src, stable=True)
        assert torch.equal((row * n + col)[a], (dst * n + src)[b]), "the CSR holds other entries than the edge list"
        pos = torch.empty_like(a)
        pos[b] = a
        _DEVICE_GRAPHS[name] = (g, pos, row, deg)
    return _DEVICE_GRAPHS[name]


def run_gpu(g, nnz, h, a_src, a_dst, slope, gout):
    """``(out, alpha [nnz, CSR order], gh, ga_src, ga_dst)`` of one forward and backward on the device."""
    h, a_src, a_dst = (v.to(DEV).requires_grad_(True) for v in (h, a_src, a_dst))
    out = _GatAggregate.apply(h, a_src, a_dst, g, slope)
    alpha = out.grad_fn.saved_tensors[3][:nnz].clone()
    out.backward(gout.to(DEV))
    return out.detach(), alpha, h.grad, a_src.grad, a_dst.grad


def compare(name, d, regime, slope):
    """Two device runs bit for bit, then every output against float64 under the bound; returns what the callers look at
    further: the device results (alpha per CSR entry), the float64 alpha per CSR entry, the row of every entry."""
    n, src, dst = graph(name)
    g, pos, row, deg = device_graph(name)
    h, a_src, a_dst, gout = op_inputs(n, d, regime)
    runs = [run_gpu(g, src.numel(), h, a_src, a_dst, slope, gout) for _ in range(2)]
    for key, a, b in zip(NAMES, *runs):
        assert same_bits(a, b), f"{key}: two runs differ"
        assert torch.isfinite(a).all(), f"{key}: not finite"
    ref = {}
    for dt in (torch.float64, torch.float32):
        r = list(brute_gat(h.to(dt), a_src.to(dt), a_dst.to(dt), src, dst, slope, gout))
        r[1] = torch.empty_like(r[1]).index_copy_(0, pos, r[1])                  # alpha: edge-list order -> CSR order
        ref[dt] = r
    tag = f"{name} d={d} {regime} slope={slope}"
    for i, key in enumerate(NAMES):
        close(runs[0][i], ref[torch.float32][i], ref[torch.float64][i], f"{key} {tag}")
    live = deg > 0
    if live.any():
        sums = [torch.zeros(n, dtype=torch.float64).index_add_(0, row, v.double().cpu())[live]
                for v in (runs[0][1], ref[torch.float32][1], ref[torch.float64][1])]
        close(*sums, f"alpha_row_sum {tag}")
    if not live.all():                                  # a destination without an in-edge: exact zeros, never 0 / 0
        assert not runs[0][0].cpu()[~live].any() and not runs[0][4].cpu()[~live].any()
    return runs[0], ref[torch.float64], row, deg


@pytest.mark.parametrize("name", ["ladder", "uniform", "powerlaw", "n1"])
@pytest.mark.parametrize("d", WIDTHS)
def test_aggregate_against_float64(d, name):
    (out, alpha, gh, ga_src, ga_dst), _, row, deg = compare(name, d, "mild", 0.2)
    if name == "ladder":
        assert deg[0] == 0 and not out[0].any() and ga_dst[0] == 0
    if name == "n1":
        assert torch.equal(alpha.cpu(), torch.ones(1))
        assert same_bits(out.cpu(), op_inputs(1, d, "mild")[0])


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("d", [8, 16, 32, 130])              # one width per lane-group size
def test_logit_regimes_and_slopes(d, slope, regime):
    (out, alpha, gh, ga_src, ga_dst), f64, row, deg = compare("ladder", d, regime, slope)
    alpha = alpha.cpu()
    if regime == "wide":
        zero = alpha == 0
        assert zero.sum() >= 10, "no weight underflows: the regime does not reach what it is for"
        assert f64[1][zero].max() < 1e-30
    if regime == "flat":
        assert same_bits(alpha, (torch.ones((), dtype=torch.float32) / deg.float())[row])
        if slope == 0.0:                               # pre > 0 is false at 0: the derivative there is the slope
            assert not ga_src.any() and not ga_dst.any()
        else:
            assert ga_src.abs().max() > 0.01


@pytest.mark.parametrize("name", MODULE_GRAPHS)
@pytest.mark.parametrize("d", MODULE_WIDTHS)
def test_conv_module_against_float64(d, name):
    conv, x, ei, w = module_case(name, d)

    def run(c, x, ei, w, forward):
        x = x.clone().requires_grad_(True)
        out = forward(c, x, ei)
        (out * w).sum().backward()
        return [out.detach(), c.lin.weight.grad, c.att_src.grad, c.att_dst.grad, c.bias.grad, x.grad]

    gpu = run(copy.deepcopy(conv).to(DEV), x.to(DEV), ei.to(DEV), w.to(DEV), lambda c, x, ei: c(x, ei))
    f64, f32 = (run(copy.deepcopy(conv).to(dt), x.to(dt), ei, w.to(dt), _host_conv) for dt in (torch.float64, torch.float32))
    for i, key in enumerate(("out", "lin.weight.grad", "att_src.grad", "att_dst.grad", "bias.grad", "x.grad")):
        close(gpu[i], f32[i], f64[i], f"module {key} {name} d={d}")


def test_aggregate_refuses_what_the_kernels_do_not_cover():
    """Every call here is refused before any launch: by the wrapper (a GdaError that names the problem), or by the C
    entry point (a status of include/gda_hip.h)."""
    n, src, dst = graph("uniform")
    g = device_graph("uniform")[0]
    h, a_src, a_dst, _ = (v.to(DEV) for v in op_inputs(n, 8, "mild"))
    apply = _GatAggregate.apply
    with pytest.raises(_lib.GdaError, match="h must have dtype"):
        apply(h.double(), a_src, a_dst, g, 0.2)
    with pytest.raises(_lib.GdaError, match="a_src must have dtype"):
        apply(h, a_src.double(), a_dst, g, 0.2)
    with pytest.raises(_lib.GdaError, match="a_dst must have dtype"):
        apply(h, a_src, a_dst.half(), g, 0.2)
    with pytest.raises(_lib.GdaError, match="a_src must be a tensor on the MI355X"):
        apply(h, a_src.cpu(), a_dst, g, 0.2)
    with pytest.raises(_lib.GdaError, match="2-D"):
        apply(h.view(n, 2, 4), a_src, a_dst, g, 0.2)
    with pytest.raises(_lib.GdaError, match="expected"):
        apply(torch.cat([h, h]), a_src, a_dst, g, 0.2)                             # more rows than the graph has
    with pytest.raises(_lib.GdaError, match="expected"):
        apply(h[:-1], a_src[:-1], a_dst[:-1], g, 0.2)                              # fewer
    with pytest.raises(_lib.GdaError, match="expected"):
        apply(h, a_src[:-1], a_dst, g, 0.2)
    with pytest.raises(_lib.GdaError, match="expected"):
        apply(h, a_src, torch.cat([a_dst, a_dst]), g, 0.2)
    loops = src == dst
    bare = build_csr(torch.stack([src[~loops], dst[~loops]]).to(DEV), n, None, False, True, False, "col")
    with pytest.raises(_lib.GdaError, match="edge map"):
        apply(h, a_src, a_dst, bare, 0.2)

    with open(os.path.join(ROOT, "include", "gda_hip.h")) as f:
        status = {k: int(v) for k, v in re.findall(r"#define (GDA_OK|GDA_E_NULL|GDA_E_SIZE)\s+\(?(-?\d+)\)?", f.read())}
    assert set(status) == {"GDA_OK", "GDA_E_NULL", "GDA_E_SIZE"} and status["GDA_OK"] == 0
    L = _lib.lib()
    out, alpha = torch.empty_like(h), torch.empty(g.nnz_cap, device=DEV)
    fwd = [g.rowptr, g.colidx, n, 8, h, a_src, a_dst, 0.2, out, alpha, None]
    bwd = [g.rowptr, g.colidx, g.t_rowptr, g.t_colidx, g.t_to_fwd, n, 8, h, a_src, a_dst, 0.2, alpha, out,
           torch.empty_like(h), torch.empty_like(a_src), torch.empty_like(a_dst), torch.empty_like(alpha), None]
    for fn, args, i_n in ((L.gda_gat_fwd_f32, fwd, 2), (L.gda_gat_bwd_f32, bwd, 5)):
        def call(**change):
            a = list(args)
            for i, v in change.items():
                a[int(i[1:])] = v
            return fn(*a)

        pointers = [i for i, v in enumerate(args[:-1]) if torch.is_tensor(v)]
        nothing = {f"_{i}": None for i in pointers}
        assert call(**nothing, **{f"_{i_n}": 0}) == status["GDA_OK"]                # no rows: nothing to do, nothing read
        assert call(**nothing, **{f"_{i_n + 1}": 0}) == status["GDA_OK"]            # no columns
        for i in pointers:
            assert call(**{f"_{i}": None}) == status["GDA_E_NULL"], f"argument {i}"
        for i in (i_n, i_n + 1):
            assert call(**{f"_{i}": -1}) == status["GDA_E_SIZE"]
            assert call(**{f"_{i}": 2 ** 31 - 1}) == status["GDA_E_SIZE"]           # beyond the int32 row / column index
