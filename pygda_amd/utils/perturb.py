"""The structure-perturbation helpers GTrans is written on, under the names and signatures of pygda/utils/perturb.py,
in torch on either device and differentiable where the reference's are.

``get_modified_adj`` is the flip operator: the flip weights -- mirrored by ``to_symmetric`` when the graph is undirected
-- are appended to the weighted edge list, duplicates are summed by ``coalesce`` (sorted by ``(row, col)``, gradient
carried to the values), and every weight above 1 is reflected to ``2 - w``.  ``project`` puts a weight vector back
inside the budget: when its clamped sum exceeds ``n_perturbations`` a shift ``miu`` is found by ``bisection`` so that
``clamp(values - miu, 0, 1)`` sums to the budget.  ``inner`` / ``inner_margin`` / ``diff`` are the cosine losses over
rows normalised by ``norm + 1e-15``; ``linear_to_triu_idx`` inverts the row-major numbering of the strict upper triangle.
tests/test_gtrans_host.py holds every one of them to the outputs recorded from the reference, bit for bit in float64.

The GTrans trainer composes its host fit from these; on the device its steps take the kernels of csrc/gda_gtrans.hip
(``ops.wgcn_norm``, ``ops.gtrans_loss``, ``ops.gtrans_project``) and only the final sampling comes through here."""
import torch


def coalesce(index, value, m, n, op='sum'):
    """``torch_sparse.coalesce``: entries sorted by ``(row, col)``, duplicates reduced by ``op`` ('sum' or 'mean', in
    input order); differentiable in ``value``."""
    key = index[0] * n + index[1]
    uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
    out_index = torch.stack([uniq // n, uniq % n])
    if value is None:
        return out_index, None
    out = torch.zeros(uniq.numel(), dtype=value.dtype, device=value.device).index_add(0, inv, value)
    if op == 'mean':
        cnt = torch.zeros(uniq.numel(), dtype=value.dtype, device=value.device).index_add(
            0, inv, torch.ones_like(value))
        out = out / cnt
    elif op not in ('sum', 'add'):
        raise ValueError(f"coalesce: op must be 'sum' or 'mean', got {op!r}")
    return out_index, out


def linear_to_triu_idx(n: int, lin_idx: torch.Tensor) -> torch.Tensor:
    """``[2, k]`` (row, col) of the strict-upper-triangle positions numbered ``lin_idx`` row by row.  Row ``r`` starts at
    ``r (2n - r - 1) / 2``; the row is the closed-form root of that quadratic, taken in float64."""
    disc = torch.sqrt(-8 * lin_idx.double() + 4 * n * (n - 1) - 7)
    row = (n - 2 - torch.floor(disc / 2.0 - 0.5)).long()
    rest = n - row
    col = lin_idx + row + 1 - n * (n - 1) // 2 + rest * (rest - 1) // 2
    return torch.stack((row, col))


def _unit_rows(t):
    return t / (t.norm(dim=1).view(-1, 1) + 1e-15)


def _row_cosine(t1, t2):
    return (_unit_rows(t1) * _unit_rows(t2)).sum(1)


def inner(t1, t2):
    """Mean over rows of ``1 - cos(t1_i, t2_i)``."""
    return (1 - _row_cosine(t1, t2)).mean()


def inner_margin(t1, t2, margin):
    """Mean over rows of ``relu(1 - cos(t1_i, t2_i) - margin)``."""
    return torch.relu(1 - _row_cosine(t1, t2) - margin).mean()


def diff(t1, t2):
    """Mean over rows of half the squared distance of the normalised rows."""
    return 0.5 * ((_unit_rows(t1) - _unit_rows(t2)) ** 2).sum(1).mean()


def bisection(edge_weights, a, b, n_perturbations, epsilon=1e-5, iter_max=1e5):
    """The shift ``miu`` in ``[a, b]`` at which ``clamp(edge_weights - miu, 0, 1).sum()`` meets ``n_perturbations``:
    midpoints until the excess is exactly 0 or the bracket is no wider than ``epsilon``.  The half that keeps the sign
    change is kept; the last midpoint is returned."""
    def excess(shift):
        return torch.clamp(edge_weights - shift, 0, 1).sum() - n_perturbations

    lo, hi, miu = a, b, a
    for _ in range(int(iter_max)):
        miu = (lo + hi) / 2
        at_mid = excess(miu)
        if at_mid == 0.0:
            return miu
        if at_mid * excess(lo) < 0:
            hi = miu
        else:
            lo = miu
        if hi - lo <= epsilon:
            break
    return miu


def project(n_perturbations, values, eps, inplace=False):
    """``values`` inside ``[eps, 1 - eps]`` and inside the budget: shifted by :func:`bisection`'s ``miu`` over
    ``[min - 1, max]`` when ``clamp(values, 0, 1)`` sums to more than ``n_perturbations``, only clamped otherwise.  A
    copy unless ``inplace``."""
    out = values if inplace else values.clone()
    over_budget = torch.clamp(out, 0, 1).sum() > n_perturbations
    shifted = out - bisection(out, (out - 1).min(), out.max(), n_perturbations) if over_budget else out
    out.data.copy_(torch.clamp(shifted, min=eps, max=1 - eps))
    return out


def to_symmetric(edge_index, edge_weight, n, op='mean'):
    """Both directions of every edge with its weight, duplicates reduced by ``op``."""
    both = torch.cat((edge_index, edge_index.flip(0)), dim=-1)
    return coalesce(both, edge_weight.repeat(2), m=n, n=n, op=op)


def get_modified_adj(modified_edge_index, perturbed_edge_weight, n, device, edge_index, edge_weight,
                     make_undirected=False):
    """The weighted edge list with the flip weights added in: summed per ``(row, col)``, a sum above 1 reflected to
    ``2 - sum`` (an existing edge is removed by the amount a new one would be added)."""
    if make_undirected:
        modified_edge_index, perturbed_edge_weight = to_symmetric(modified_edge_index, perturbed_edge_weight, n)
    index = torch.cat((edge_index.to(device), modified_edge_index), dim=-1)
    weight = torch.cat((edge_weight.to(device), perturbed_edge_weight))
    index, weight = coalesce(index, weight, m=n, n=n, op='sum')
    return index, torch.where(weight > 1, 2 - weight, weight)
