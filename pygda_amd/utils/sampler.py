"""SOGA's sample tables (pygda/utils/sampler.py ``RandomWalker`` / ``Negative_Sampler`` as ``SOGABase.init_target``
drives them), restated on numpy arrays without networkx.

``soga_samples(edge_index, n, num_negative)`` returns, for the ``struct`` and the ``neigh`` view, the triple
``(center [n, 1], positive [n, 1], negative [n, num_negative])`` of int64 arrays.  It consumes Python's ``random`` and
``np.random`` in the reference's order -- per view: one ``random.shuffle`` of the nodes, per node in that order a
length-2 walk (two ``np.random.random()`` draws through the node's alias table, none for a node without a successor,
which is its own positive), then ``n * num_negative`` draws of ``random.randrange`` / ``random.random`` through the
degree-proportional alias table -- so that with the same two seeds the tables are the reference's, bit for bit.

The graph is the reference's ``to_networkx`` ``DiGraph``: nodes ``0 .. n-1``, the edges added in ``edge_index`` order,
duplicates collapsing, a node's neighbours its successors in first-insertion order, its degree in-degree plus
out-degree (a self loop counts twice).  Row ``i`` of the tables is the ``i``-th walk, not node ``i``."""
import random

import numpy as np


def _digraph(edge_index, n):
    """``(successors, degree)``: per node the list of distinct successors in first-insertion order, and in + out degree."""
    ei = np.asarray(edge_index.cpu() if hasattr(edge_index, "cpu") else edge_index).astype(np.int64).reshape(2, -1)
    if ei.size and (ei.min() < 0 or ei.max() >= n):
        raise ValueError(f"soga_samples: edge_index refers to nodes outside [0, {n})")
    succ = [dict() for _ in range(n)]
    degree = np.zeros(n, dtype=np.int64)
    for u, v in zip(ei[0].tolist(), ei[1].tolist()):
        if v not in succ[u]:
            succ[u][v] = None
            degree[u] += 1
            degree[v] += 1
    return [list(s) for s in succ], degree


def _uniform_alias(d):
    """The alias table of ``d`` equal shares ``1 / d``, scaled by ``d`` in float64 as the reference scales them:
    ``(1 / d) * d`` falls below 1.0 for some ``d``, which sends those slots through the balancing loop."""
    accept, alias = [0] * d, [0] * d
    if d == 0:
        return accept, alias
    share = np.array([1.0 / float(d)] * d) * d
    small = [i for i in range(d) if share[i] < 1.0]
    large = [i for i in range(d) if not share[i] < 1.0]
    while small and large:
        lo, hi = small.pop(), large.pop()
        accept[lo], alias[lo] = share[lo], hi
        share[hi] = share[hi] - (1 - share[lo])
        (small if share[hi] < 1.0 else large).append(hi)
    for i in large + small:
        accept[i] = 1
    return accept, alias


def _degree_alias(degree):
    """The negative sampler's tables over ``degree / degree.sum()`` against the uniform share ``1 / n``."""
    n = degree.size
    probs = degree.astype(np.float64)
    probs = probs / np.sum(probs)
    accept, alias = np.ones(n, dtype=np.float64), np.zeros(n, dtype=np.int32)
    share = 1.0 / n
    low = [i for i in range(n) if probs[i] < share]
    high = [i for i in range(n) if not probs[i] < share]
    while low and high:
        lo, hi = low.pop(), high.pop()
        accept[lo], alias[lo] = probs[lo] / share, hi
        probs[hi] = probs[hi] - (share - probs[lo])
        (low if probs[hi] < share else high).append(hi)
    return accept, alias


def _view(succ, tables, neg_accept, neg_alias, n, k):
    order = list(range(n))
    random.shuffle(order)
    walks = np.empty((n, 2), dtype=np.int64)
    for row, v in enumerate(order):
        nbrs = succ[v]
        if nbrs:
            accept, alias = tables[v]
            i = int(np.random.random() * len(accept))
            r = np.random.random()
            walks[row] = v, nbrs[i if r < accept[i] else alias[i]]
        else:
            walks[row] = v, v
    neg = np.empty(n * k, dtype=np.int64)
    for q in range(n * k):
        i = random.randrange(n)
        neg[q] = i if random.random() < neg_accept[i] else neg_alias[i]
    return walks[:, :1].copy(), walks[:, 1:].copy(), neg.reshape(n, k)


def soga_samples(edge_index, n, num_negative):
    """``[(center, positive, negative) of the struct view, the same of the neigh view]`` for the ``n``-node graph
    ``edge_index [2, E]`` (see the module's docstring)."""
    n, k = int(n), int(num_negative)
    if n < 1 or k < 1:
        raise ValueError(f"soga_samples: n >= 1 and num_negative >= 1 expected, got {n} and {k}")
    succ, degree = _digraph(edge_index, n)
    cache = {}
    tables = [cache.setdefault(len(s), _uniform_alias(len(s))) for s in succ]
    neg_accept, neg_alias = _degree_alias(degree)
    # both views walk the same graph and draw their negatives from the struct graph's degrees; the second view simply
    # goes on consuming the two streams
    return [_view(succ, tables, neg_accept, neg_alias, n, k) for _ in range(2)]
