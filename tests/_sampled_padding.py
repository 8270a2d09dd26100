"""Helpers of tests/test_gpu_sampled_padding.py that need no GPU (tests/test_sampled_padding_host.py runs them on the host).

The sampled A2GNN step runs at a static capacity shape (pygda_amd/sampled_graph.py): every matrix has ``ncap`` rows, the
first ``n_live`` are real.  What lies behind the live prefixes of a ``_StaticBatch`` block is PADDING -- node ids
``[n_live, ncap)``, the edge-list columns from ``e`` on, the entries of both CSRs from ``nnz`` on -- and the module's
docstring promises that nothing it holds reaches a parameter.  :func:`poison_tail` rewrites exactly that padding,
:func:`differences` compares two recorded runs as values, :func:`oracle_step` is the real-shape CPU yardstick of one step.
"""
import numpy as np
import torch

VARIANTS = ("zero", "random", "hot")
POISON = 1.0e3            # size of every poisoned value: finite, far from anything a live row holds


def poison_tail(static, variant, hot=0, seed=0):
    """Rewrite, in place, the padding of a ``_StaticBatch`` block whose live sizes are ``static.live`` = (n, e, nnz, ..):
    ``nodes[n:ncap]``, the edge-list columns from ``e`` on, ``colidx`` / ``val`` and ``t_colidx`` / ``t_val`` from ``nnz``
    on.  ``counts``, both ``rowptr`` arrays and every live prefix stay as they are.  Everything written is finite and in
    range (node ids in [0, N), column ids in [0, ncap), values about +-1e3): a wrong read shows as a wrong number.

    ``"zero"``: ids 0, values 0.  ``"random"``: valid random ids, random values in [-1e3, 1e3] (generator ``seed``).
    ``"hot"``: every padded row holds node ``hot`` (the caller has given that node alternating +-1e3 features and a valid
    label); padded CSR entries and edges point at the first padded row -- whose activations derive from those features --
    with weights alternating +-1e3."""
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")
    n, e, nnz = (int(v) for v in static.live[:3])
    ncap = int(static.ncap)
    n_nodes = int(static.loader.data.x.size(0))
    if not 0 <= int(hot) < n_nodes:
        raise ValueError("the hot node must be a node of the graph")
    g = static.graph
    dev = static.nodes.device
    gen = torch.Generator().manual_seed(int(seed))
    pad_row = min(n, ncap - 1)

    def ids(count, high, fixed):
        if variant == "zero":
            return torch.zeros(count, dtype=torch.int64)
        if variant == "random":
            return torch.randint(0, high, (count,), generator=gen)
        return torch.full((count,), int(fixed), dtype=torch.int64)

    def vals(count):
        if variant == "zero":
            return torch.zeros(count, dtype=torch.float32)
        if variant == "random":
            return (torch.rand(count, generator=gen) * 2 - 1) * POISON
        v = torch.full((count,), POISON, dtype=torch.float32)
        v[1::2] = -POISON
        return v

    nodes = static.nodes[:ncap]
    nodes[n:] = ids(ncap - n, n_nodes, hot).to(dev)
    ecap = static.ei.size(1)
    for r in range(2):
        static.ei[r, e:] = ids(ecap - e, ncap, pad_row).to(dev)
    for ci, va in ((g.colidx, g.val), (g.t_colidx, g.t_val)):
        cap = ci.numel()
        ci[nnz:] = ids(cap - nnz, ncap, pad_row).to(dev, torch.int32)
        va[nnz:cap] = vals(cap - nnz).to(dev)
    return static


def hot_features(width):
    """The designated node's feature row: alternating +-1e3."""
    v = torch.full((width,), POISON, dtype=torch.float32)
    v[1::2] = -POISON
    return v


def differences(a, b):
    """Names of everything that differs AS VALUES (``torch.equal``: a zero of either sign is a zero) between two recorded
    runs: ``{"loss": [..], "correct": [..], "param" | "exp_avg" | "exp_avg_sq": [{name: tensor} per step]}``."""
    out = []
    if len(a["loss"]) != len(b["loss"]):
        return [f"steps: {len(a['loss'])} against {len(b['loss'])}"]
    for k in range(len(a["loss"])):
        for what in ("loss", "correct"):
            if a[what][k] != b[what][k]:
                out.append(f"step {k}: {what} {a[what][k]!r} != {b[what][k]!r}")
        for what in ("param", "exp_avg", "exp_avg_sq"):
            if a[what][k].keys() != b[what][k].keys():
                out.append(f"step {k}: {what} names differ")
                continue
            for name, v in a[what][k].items():
                if not torch.equal(v, b[what][k][name]):
                    w = b[what][k][name]
                    gap = float((v.double() - w.double()).abs().max()) if v.shape == w.shape else float("nan")
                    out.append(f"step {k}: {what}[{name}] max |a - b| = {gap:.3e}")
    return out


def oracle_step(state, dims, src, tgt, samples, s_pnums, t_pnums, weight, chunk_rows=128):
    """One real-shape step of ``oracle.pygda_cpu`` on the live rows and live edges of a batch pair, dropout 0, with the
    step's own MMD draws ``samples = (s_idx, t_idx)``: ``{torch.float64 | torch.float32: (loss, {name: gradient})}``.
    ``state``: the device net's ``state_dict()``; ``dims`` = (in, hidden, classes, layers); ``src`` / ``tgt`` =
    ``(x, edge_index, y)`` CPU tensors (``y`` of the target may be None)."""
    from oracle import pygda_cpu as O
    out = {}
    for dt in (torch.float64, torch.float32):
        net = O.A2GNNBase(dims[0], dims[1], dims[2], num_layers=dims[3], dropout=0.0).to(dt)
        net.load_state_dict({k: v.detach().cpu().to(dt) for k, v in state.items()})
        net.train()
        S = O.Graph(src[0].to(dt), src[1], src[2])
        T = O.Graph(tgt[0].to(dt), tgt[1], tgt[2])
        loss, _, _ = O.a2gnn_forward_model(net, S, T, 0.0, s_pnums, t_pnums, False, weight, chunk_rows,
                                           mmd_samples=samples)
        names, params = zip(*net.named_parameters())
        grads = torch.autograd.grad(loss, params)
        out[dt] = (loss.detach(), {k: g.detach() for k, g in zip(names, grads)})
        del net, loss, grads
    return out


def bound_report(name, gpu, f32, f64, slack=2e-6):
    """The figures of tests/test_gpu_cwgcn._close for one tensor: (|gpu - f64|, |fp32 oracle - f64|, the limit
    8 |fp32 - f64| + slack max|f64|), printed before anything asserts."""
    gpu, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                     for v in (gpu, f32, f64))
    e_gpu, e_ref = float(np.abs(gpu - f64).max()), float(np.abs(f32 - f64).max())
    lim = 8 * e_ref + slack * max(float(np.abs(f64).max()), 1e-30)
    print(f"  {name}: |gpu - f64| = {e_gpu:.3e}  |fp32 - f64| = {e_ref:.3e}  limit = {lim:.3e}  max|f64| = "
          f"{float(np.abs(f64).max()):.3e}")
    return e_gpu, e_ref, lim
