"""The CSR SpMM kernels (csrc/gda_spmm.hip) without a GPU: the float32 emulations that tests/test_gpu_spmm.py compares
the device results with bit for bit, the graphs and inputs both files share, and the conditions those have to meet.

The kernels' contract is an ORDER of operations: a row's sum starts from +0 and takes its entries in CSR order, every
product and every sum rounded to float32 on its own.  The emulations below follow that order with numpy float32 arrays
(numpy never contracts a multiply and an add), one entry position at a time for all rows at once:

  (a) ``walk``           whole rows;
  (b) ``chunked_walk``   rows above a threshold cut into fixed chunks, each partial from +0, the partials added in chunk
                         order from +0 (k_spmm's chunk blocks + k_long_reduce) -- under the synced rule of
                         graph.RowSplit (nothing is cut unless the longest row exceeds twice the threshold) or the
                         deferred one of a transient graph (every row above the threshold);
  (c) ``epilogue``       ``alpha x + beta acc (+ g z)``, then the bias;
  (d) ``interior_*``     the launch chain of gda_spmm_csr_interior_kstep_f32 on a sampled-batch-shaped CSR;
  (e) ``walk64``         the same sums in float64 with ``S = sum |terms|`` per element.

Checked here: (a) is ``oracle.pygda_cpu.propagate`` bit for bit; (a), (b), (c) lie within their derived bounds of float64;
the inputs DISCRIMINATE -- a reversed row, another chunk size, chunks added in reverse and a fused multiply-add each change
bits on the rows made for it, so a kernel that did any of these would fail the bit comparison; the transpose maker
round-trips."""
import functools

import numpy as np
import pytest
import torch

from oracle.pygda_cpu import propagate

F32 = np.float32
EPS = 2.0 ** -24
N_ROWS = 301                      # 301 = 4 * 75 + 1: the last workgroup is partly live at every lane-group width
THRESHOLD = 128                   # graph.SPLIT_THRESHOLD (test_gpu_spmm.py asserts the two agree)
# on both sides of every lane-group width (4 .. 64), of the 4-entry unroll inside a tile, of the chunk threshold and of
# twice the chunk threshold
NAMED_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 67, 127, 128, 129, 130, 255, 256)
SPLIT_LENGTHS = (257, 300, 385)   # the "split" variant: its longest row exceeds 2 x THRESHOLD
SEEDS = {"whole": 11, "split": 12}
CHUNK_SEED = 0                    # features(n, d, CHUNK_SEED): every cut row of either graph tells (b) from (a) at d = 5, 6, 37, 128


class CSR:
    """A raw CSR (int32 ``rowptr``/``colidx``, float32 ``val``) of ``n`` rows and ``n`` columns."""

    def __init__(self, n, rowptr, colidx, val):
        self.n, self.rowptr, self.colidx, self.val = n, rowptr.astype(np.int32), colidx.astype(np.int32), val.astype(F32)

    @property
    def lengths(self):
        return np.diff(self.rowptr.astype(np.int64))

    def rows(self):
        """The row of every entry."""
        return np.repeat(np.arange(self.n), self.lengths)


def transpose(a):
    """The by-source CSR of ``a`` in stable order: the entries of a column in the order ``a`` holds them (by row, then
    by position inside the row)."""
    order = np.argsort(a.colidx, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(a.colidx, minlength=a.n))])
    return CSR(a.n, rowptr, a.rows()[order], a.val[order])


def _from_rows(n, cols, vals):
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    return CSR(n, rowptr, np.concatenate(cols) if rowptr[-1] else np.zeros(0, np.int32),
               np.concatenate(vals) if rowptr[-1] else np.zeros(0, F32))


class Graph:
    """``fwd`` and its host-built transpose ``t``; ``named``: length -> row of the rows with a designed length."""

    def __init__(self, fwd, named, marks):
        self.fwd, self.t, self.named, self.marks, self.n = fwd, transpose(fwd), named, marks, fwd.n


@functools.lru_cache(maxsize=None)
def graph(name):
    """``"whole"``: 301 rows, the NAMED_LENGTHS on rows spread over the matrix, the others 0 .. 13 entries; normal weights
    of both signs with one exact zero; one row that names a column twice in a row; one self reference.  A few hub
    columns collect enough entries for transposed rows of 129 .. 256 entries (whole rows under the synced rule).
    ``"split"``: also rows of 257, 300 and 385 entries, and hub columns beyond 256 entries: both orientations chunk."""
    rng = np.random.default_rng(SEEDS[name])
    split = name == "split"
    lengths = rng.integers(0, 14, N_ROWS)
    named_lengths = NAMED_LENGTHS + (SPLIT_LENGTHS if split else ())
    where = rng.permutation(N_ROWS - 1)[:len(named_lengths)]          # row 300 keeps a random length ...
    lengths[where] = named_lengths
    lengths[N_ROWS - 1] = max(lengths[N_ROWS - 1], 3)                 # ... and is live
    named = {int(L): int(r) for L, r in zip(named_lengths, where)}
    hubs, p_hub = rng.permutation(N_ROWS)[:2], (0.3 if split else 0.08)
    cols, vals = [], []
    for L in lengths:
        c = rng.integers(0, N_ROWS, L)
        c = np.where(rng.random(L) < p_hub, hubs[rng.integers(0, 2, L)], c)
        cols.append(c.astype(np.int32))
        vals.append(rng.standard_normal(L).astype(F32))
    marks = {"zero": (named[17], 9), "repeat": (named[9], 4), "self": (named[5], 2)}
    vals[named[17]][9] = 0.0
    cols[named[9]][4] = cols[named[9]][3]
    cols[named[5]][2] = named[5]
    return Graph(_from_rows(N_ROWS, cols, vals), named, marks)


N_BATCH, N_INT = 320, 60
INTERIOR_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 70)


@functools.lru_cache(maxsize=None)
def batch(kind):
    """A sampled-batch-shaped CSR of 320 rows whose first 60 are interior.  ``"fwd"`` (rows by destination): the interior
    rows have the INTERIOR_LENGTHS and random short ones, columns mixed between interior and leaf -- one row with leaf
    columns only, one with interior columns only --, the leaf rows hold their unit self loop.  ``"bwd"`` (rows by
    source, what the transposed operator walks): interior rows of the same lengths name interior columns only, a leaf row
    holds up to 13 interior columns and its unit self loop.  ``"eye"``: unit self loops only (n_int = 0)."""
    rng = np.random.default_rng({"fwd": 21, "bwd": 22, "eye": 23}[kind])
    cols, vals = [], []
    if kind == "eye":
        return _from_rows(N_BATCH, [np.array([r], np.int32) for r in range(N_BATCH)], [np.ones(1, F32)] * N_BATCH)
    lengths = rng.integers(0, 14, N_INT)
    where = rng.permutation(N_INT)[:len(INTERIOR_LENGTHS) + 2]
    lengths[where[:len(INTERIOR_LENGTHS)]] = INTERIOR_LENGTHS
    leaf_only, int_only = where[-2:]
    lengths[leaf_only], lengths[int_only] = 6, 11
    for r in range(N_INT):
        L = lengths[r]
        ci, cl = rng.integers(0, N_INT, L), rng.integers(N_INT, N_BATCH, L)
        pick = rng.random(L) < 0.5
        if kind == "bwd" or r == int_only:
            pick[:] = True
        elif r == leaf_only:
            pick[:] = False
        cols.append(np.where(pick, ci, cl).astype(np.int32))
        vals.append(rng.standard_normal(L).astype(F32))
    for r in range(N_INT, N_BATCH):
        L = rng.integers(0, 14) if kind == "bwd" else 0
        cols.append(np.concatenate([rng.integers(0, N_INT, L), [r]]).astype(np.int32))
        vals.append(np.concatenate([rng.standard_normal(L), [1.0]]).astype(F32))
    return _from_rows(N_BATCH, cols, vals)


def features(n, d, seed):
    return np.random.default_rng(1000 + seed).standard_normal((n, d)).astype(F32)


def bias_of(d, seed=7):
    return np.random.default_rng(2000 + seed).standard_normal(d).astype(F32)


# ---- the emulations --------------------------------------------------------------------------------------------------------
def _walk(a, x, lo, hi, rows=None, dtype=F32, reverse=False, fused=False, take=None, with_s=False):
    """``acc[r] = (((+0 + w_0 x[c_0]) + w_1 x[c_1]) + ...)`` over the entries ``[lo[r], hi[r])`` of ``a`` for the rows
    ``rows`` (default: all), product and sum rounded to ``dtype`` separately.  ``reverse``: last entry first.  ``fused``:
    the product exact (float64) and one rounding per entry.  ``take``: per-entry mask; a skipped entry adds nothing
    (the kernel adds ``w * 0`` or nothing: the same, the sum is never -0).  ``with_s``: also ``sum |w x|``."""
    rows = np.arange(a.n) if rows is None else np.asarray(rows)
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    acc = np.zeros((len(rows), x.shape[1]), dtype)
    s = np.zeros_like(acc)
    xs, val = x.astype(dtype, copy=False), a.val.astype(dtype)
    for p in range(int((hi - lo).max()) if len(rows) else 0):
        live = np.nonzero(lo + p < hi)[0]
        k = (hi[live] - 1 - p) if reverse else (lo[live] + p)
        if take is not None:
            live, k = live[take[k]], k[take[k]]
        if fused:
            acc[live] = (acc[live].astype(np.float64)
                         + a.val[k, None].astype(np.float64) * x[a.colidx[k]].astype(np.float64)).astype(dtype)
            continue
        term = val[k, None] * xs[a.colidx[k]]
        acc[live] = acc[live] + term
        if with_s:
            s[live] += np.abs(term)
    return (acc, s) if with_s else acc


def walk(a, x, **kw):
    """(a): every row as one walk."""
    return _walk(a, x, a.rowptr[:-1], a.rowptr[1:], **kw)


def walk64(a, x):
    """(e): ``(sum, S)`` in float64."""
    return walk(a, x, dtype=np.float64, with_s=True)


def chunked_rows(a, threshold=THRESHOLD, rule="synced"):
    """Mask of the rows the layout cuts.  Synced (graph.RowSplit): rows above the threshold, and none unless the longest
    row exceeds twice the threshold.  Deferred (a transient graph, counts left on the device): every row above it."""
    L = a.lengths
    if rule == "synced" and (a.n == 0 or L.max() <= 2 * threshold):
        return np.zeros(a.n, bool)
    return L > threshold


def chunked_walk(a, x, threshold=THRESHOLD, rule="synced", reverse_reduce=False):
    """(b): a cut row = its ``threshold``-entry chunks, each summed from +0, added in chunk order from +0; the other rows
    as (a)."""
    cut = chunked_rows(a, threshold, rule)
    start, end = a.rowptr[:-1].astype(np.int64), a.rowptr[1:].astype(np.int64)
    y = _walk(a, x, start, np.where(cut, start, end))
    rows = np.nonzero(cut)[0]
    if not len(rows):
        return y
    n_chunks = -(-(end[rows] - start[rows]) // threshold)
    total = np.zeros((len(rows), x.shape[1]), F32)
    order = range(int(n_chunks.max()))
    for q in (reversed(order) if reverse_reduce else order):
        live = np.nonzero(q < n_chunks)[0]
        lo = start[rows[live]] + q * threshold
        total[live] = total[live] + _walk(a, x, lo, np.minimum(lo + threshold, end[rows[live]]), rows=rows[live])
    y[rows] = total
    return y


def epilogue(acc, x, alpha, beta, z=None, gamma=1.0, gamma_dev=None, bias=None):
    """(c): ``alpha x + beta acc``, two products and a sum; ``+ g z`` with ``g = gamma * gamma_dev`` rounded to float32;
    then the bias."""
    y = F32(alpha) * x + F32(beta) * acc
    if z is not None:
        g = F32(gamma) if gamma_dev is None else F32(gamma) * F32(gamma_dev)
        y = y + g * z
    return y if bias is None else y + bias


def epilogue64(a, x, alpha, beta, z=None, gamma=1.0, gamma_dev=None):
    """``(value, S)`` in float64 with the float32 coefficients the kernel is handed (``g`` exact):
    ``S = |alpha x| + |beta| sum |w x| + |g z|``."""
    acc, s = walk64(a, x)
    al, be = float(F32(alpha)), float(F32(beta))
    y, S = al * x.astype(np.float64) + be * acc, np.abs(al * x.astype(np.float64)) + abs(be) * s
    if z is not None:
        g = float(F32(gamma)) * (1.0 if gamma_dev is None else float(F32(gamma_dev)))
        y, S = y + g * z.astype(np.float64), S + np.abs(g * z.astype(np.float64))
    return y, S


def self_loop_rows(x, bias=None):
    """What a unit-self-loop row computes, ``(+0 + 1 x) + bias``: a -0 becomes +0."""
    y = F32(0.0) + F32(1.0) * x
    return y if bias is None else y + bias


def kstep(a, x, K, bias=None, chunk=None):
    """K full steps of (a) -- or of (b) under the rule ``chunk`` --, the bias in the last."""
    for _ in range(K):
        x = walk(a, x) if chunk is None else chunked_walk(a, x, rule=chunk)
    return x if bias is None else x + bias


def _range_walk(a, n_int, xa, xb, rows, take=None):
    """k_spmm_range on ``rows``: columns below ``n_int`` gather from ``xa``, the others from ``xb``."""
    src = np.concatenate([xa[:n_int], xb[n_int:]])
    rows = np.asarray(rows)
    return _walk(a, src, a.rowptr[rows], a.rowptr[rows + 1], rows=rows, take=take)


def interior_forward(a, n_int, x, K, bias=None, hoist=False):
    """(d) forward.  Without ``hoist`` (no ``sacc`` handed in, or K = 1): K walks over all of an interior row's entries,
    leaf columns read from ``x``.  With it: ``c`` = the row's leaf-column entries in CSR order, once; a step = the
    interior-column entries in order, ``+ c``, ``+ bias`` in the last.  Leaf rows: ``(0 + 1 x) + bias``."""
    y = np.empty_like(x)
    y[n_int:] = self_loop_rows(x[n_int:], bias)
    if n_int == 0:
        return y
    I, leaf_col = np.arange(n_int), a.colidx >= n_int
    hoist = hoist and K >= 2
    if hoist:
        c = _range_walk(a, n_int, x, x, I, take=leaf_col)
    h = x
    for j in range(1, K + 1):
        out = _range_walk(a, n_int, h, x, I, take=~leaf_col) + c if hoist else _range_walk(a, n_int, h, x, I)
        h = out if j < K or bias is None else out + bias
    y[:n_int] = h
    return y


def interior_transposed(a, n_int, x, K):
    """(d) transposed, ``a`` by source: K steps over the interior rows, ``sacc = h_0`` then ``sacc + h_j`` on the way; then
    one pass over the leaf rows, interior columns read ``sacc``, the others (the self loop) ``x``.  ``(y, sacc)``."""
    y = np.empty_like(x)
    if n_int == 0:
        y[:] = _range_walk(a, 0, x, x, np.arange(a.n))
        return y, None
    I, h, sacc = np.arange(n_int), x, None
    for _ in range(K):
        sacc = h[:n_int].copy() if sacc is None else sacc + h[:n_int]
        h = _range_walk(a, n_int, h, x, I)
    y[:n_int] = h
    if n_int < a.n:
        y[n_int:] = _range_walk(a, n_int, sacc, x, np.arange(n_int, a.n))
    return y, sacc


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def rows_differ(a, b):
    """Per row: does any element differ in bits?"""
    return (bits(a) != bits(b)).any(axis=1)


# ---- the graphs are the designed ones --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["whole", "split"])
def test_graph_has_the_designed_rows(name):
    g = graph(name)
    a, L = g.fwd, g.fwd.lengths
    assert a.n == N_ROWS and N_ROWS % 4 == 1 and L[-1] > 0
    want = NAMED_LENGTHS + (SPLIT_LENGTHS if name == "split" else ())
    assert all(L[g.named[w]] == w for w in want) and len(set(g.named.values())) == len(want)
    others = np.delete(L, list(g.named.values()))
    assert others.max() <= 13 and (others == 0).any()
    assert a.colidx.min() >= 0 and a.colidx.max() < N_ROWS and not np.isnan(a.val).any()
    assert (a.val > 0).any() and (a.val < 0).any() and (a.val == 0).sum() == 1
    r, p = g.marks["zero"]
    assert a.val[a.rowptr[r] + p] == 0
    r, p = g.marks["repeat"]
    assert a.colidx[a.rowptr[r] + p] == a.colidx[a.rowptr[r] + p - 1]
    r, p = g.marks["self"]
    assert a.colidx[a.rowptr[r] + p] == r
    Lt = g.t.lengths
    if name == "whole":         # no chunks in either orientation under the synced rule; long whole rows in both
        assert L.max() == 256 and THRESHOLD < Lt.max() <= 2 * THRESHOLD
        assert not chunked_rows(a).any() and not chunked_rows(g.t).any()
        assert chunked_rows(a, rule="deferred").sum() == 4
    else:
        assert L.max() == 385 and Lt.max() > 2 * THRESHOLD
        assert sorted(L[chunked_rows(a)]) == [129, 130, 255, 256, 257, 300, 385] and chunked_rows(g.t).any()


@pytest.mark.parametrize("name", ["whole", "split"])
def test_transpose_round_trips(name):
    g = graph(name)
    a, t = g.fwd, g.t
    assert t.rowptr[-1] == a.rowptr[-1] and np.array_equal(np.bincount(a.colidx, minlength=a.n), t.lengths)
    key = lambda rows, cols, v: sorted(zip(rows.tolist(), cols.tolist(), bits(v).tolist()))
    assert key(a.rows(), a.colidx, a.val) == key(t.colidx, t.rows(), t.val)
    # by-source order is stable: a column's entries by ascending row
    assert all((np.diff(t.colidx[t.rowptr[r]:t.rowptr[r + 1]]) >= 0).all() for r in range(t.n))
    # twice transposed = the rows of `a`, each stably sorted by column; three times = once
    tt, ttt = transpose(t), transpose(transpose(t))
    order = np.lexsort((np.arange(len(a.colidx)), a.colidx, a.rows()))
    assert np.array_equal(tt.rowptr, a.rowptr) and np.array_equal(tt.colidx, a.colidx[order])
    assert same_bits(tt.val, a.val[order])
    assert np.array_equal(ttt.rowptr, t.rowptr) and np.array_equal(ttt.colidx, t.colidx) and same_bits(ttt.val, t.val)
    # and the two orientations are one operator: <A x, y> = <x, A^T y> in float64
    x, y = features(a.n, 3, 1).astype(np.float64), features(a.n, 3, 2).astype(np.float64)
    lhs, rhs = (walk64(a, x)[0] * y).sum(), (x * walk64(t, y)[0]).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(walk64(a, x)[1]) * np.abs(y)).sum()


def test_batches_have_the_designed_shape():
    for kind in ("fwd", "bwd"):
        a = batch(kind)
        L, rows = a.lengths, a.rows()
        assert a.n == N_BATCH and set(INTERIOR_LENGTHS) <= set(L[:N_INT].tolist())
        leaf_col = a.colidx >= N_INT
        if kind == "fwd":
            assert (L[N_INT:] == 1).all() and np.array_equal(a.colidx[rows >= N_INT], np.arange(N_INT, N_BATCH))
            per_row = [set(leaf_col[a.rowptr[r]:a.rowptr[r + 1]].tolist()) for r in range(N_INT)]
            assert {True} in per_row and {False} in per_row and {True, False} in per_row
        else:
            assert not leaf_col[rows < N_INT].any()
            last = a.rowptr[N_INT + 1:] - 1
            assert np.array_equal(a.colidx[last], np.arange(N_INT, N_BATCH)) and L[N_INT:].max() > 8
            assert (leaf_col[rows >= N_INT].sum() == N_BATCH - N_INT)
        assert (a.val[a.colidx == rows][-(N_BATCH - N_INT):] == 1).all()
    e = batch("eye")
    assert np.array_equal(e.colidx, np.arange(N_BATCH)) and (e.val == 1).all()


# ---- (a) is the oracle, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["whole", "split"])
@pytest.mark.parametrize("d", [1, 5, 37, 260])
def test_walk_is_the_oracle_propagate(d, name):
    g = graph(name)
    x = features(g.n, d, d)
    for a in (g.fwd, g.t):
        ei = torch.from_numpy(np.stack([a.colidx.astype(np.int64), a.rows()]))       # edges listed by destination
        ref = propagate(ei, torch.from_numpy(a.val), torch.from_numpy(x)).numpy()
        assert same_bits(walk(a, x), ref)


# ---- (a), (b), (c) against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["whole", "split"])
@pytest.mark.parametrize("d", [5, 37])
def test_walks_lie_within_the_bound_of_float64(d, name):
    g = graph(name)
    x = features(g.n, d, d)
    for a in (g.fwd, g.t):
        ref, S = walk64(a, x)
        bound = (a.lengths[:, None] + 1) * EPS * S
        for y in (walk(a, x), chunked_walk(a, x), chunked_walk(a, x, rule="deferred")):
            err = np.abs(y.astype(np.float64) - ref)
            print(f"{name} d={d}: worst |f32 - f64| / bound = {(err / np.where(bound > 0, bound, 1)).max():.3f}")
            assert (err <= bound).all()


GENERAL = dict(alpha=0.3, beta=1.7, gamma=3.0, gamma_dev=0.37)


@pytest.mark.parametrize("name", ["whole", "split"])
@pytest.mark.parametrize("d", [5, 36])
def test_epilogue_lies_within_the_bound_of_float64(d, name):
    """One rounding per product (L + 3), per sum (L + 2, the first one from +0 exact) and for g: (L + 6) 2^-24 S holds
    with room."""
    g = graph(name)
    x, z = features(g.n, d, d), features(g.n, d, d + 500)
    for a in (g.fwd, g.t):
        for zz in (None, z):
            ref, S = epilogue64(a, x, z=zz, **GENERAL)
            bound = (a.lengths[:, None] + 6) * EPS * S
            for acc in (walk(a, x), chunked_walk(a, x)):
                err = np.abs(epilogue(acc, x, z=zz, **GENERAL).astype(np.float64) - ref)
                assert (err <= bound).all(), (err / bound).max()


# ---- the inputs discriminate -----------------------------------------------------------------------------------------------
D_DISC = 37


@pytest.mark.parametrize("name", ["whole", "split"])
def test_a_reversed_row_changes_bits(name):
    g = graph(name)
    x = features(g.n, D_DISC, 3)
    moved = rows_differ(walk(g.fwd, x), walk(g.fwd, x, reverse=True))
    for L, r in g.named.items():
        assert moved[r] if L >= 33 else (L >= 3 or not moved[r]), L      # up to two entries commute; from 33 on: required


@pytest.mark.parametrize("name", ["whole", "split"])
def test_a_fused_multiply_add_changes_bits(name):
    g = graph(name)
    x = features(g.n, D_DISC, 3)
    moved = rows_differ(walk(g.fwd, x), walk(g.fwd, x, fused=True))
    for L, r in g.named.items():
        assert L < 2 or moved[r], L                       # one entry: a single rounding either way
    assert not moved[g.fwd.lengths < 2].any()


@pytest.mark.parametrize("d", [5, 6, 37, 128])
def test_every_chunked_row_differs_from_its_whole_walk(d):
    """At every width the chunked device cases use: a reduce that ignored the chunks, or chunk blocks that were never
    launched, cannot pass.  The one exception is by construction, not by seed: a row of THRESHOLD + 1 entries is
    ``(0 + p_0) + (0 + w x)`` = ``p_0 + w x``, the whole walk's own last step -- its two forms are the same bits always (that
    row still tells whether its chunks were summed at all)."""
    g, w = graph("split"), graph("whole")
    x = features(g.n, d, CHUNK_SEED)
    for a, rules in ((g.fwd, ("synced", "deferred")), (g.t, ("synced", "deferred")), (w.fwd, ("deferred",))):
        whole = walk(a, x)
        for rule in rules:
            cut = chunked_rows(a, rule=rule)
            moved = rows_differ(whole, chunked_walk(a, x, rule=rule))
            must = cut & (a.lengths != THRESHOLD + 1)
            assert cut.any() and np.array_equal(moved, must), (d, rule, a.lengths[must != moved])
    assert same_bits(walk(w.fwd, x), chunked_walk(w.fwd, x)) and same_bits(walk(w.t, x), chunked_walk(w.t, x))


def test_another_chunk_size_and_a_reversed_reduce_change_bits():
    g = graph("split")
    x = features(g.n, D_DISC, 3)
    a = g.fwd
    ref = chunked_walk(a, x, rule="deferred")
    cut = chunked_rows(a, rule="deferred")
    assert rows_differ(ref, chunked_walk(a, x, threshold=64, rule="deferred"))[cut].all()
    # two chunks commute; from three chunks on the order of the reduce shows
    three = a.lengths > 2 * THRESHOLD
    moved = rows_differ(ref, chunked_walk(a, x, rule="deferred", reverse_reduce=True))
    assert three.sum() == 3 and np.array_equal(moved, three)
    # a chunk that starts one entry late or early (threshold off by one)
    assert rows_differ(ref, chunked_walk(a, x, threshold=THRESHOLD + 1, rule="deferred"))[a.lengths > THRESHOLD + 1].all()


# ---- (d): the chain's variants agree where the code says they do, and differ where it re-associates ---------------------------
@pytest.mark.parametrize("d", [3, 8])
def test_interior_chain_emulations(d):
    a, b = batch("fwd"), batch("bwd")
    x, bias = features(N_BATCH, d, d), bias_of(d)
    for K in (1, 2, 4):
        plain = interior_forward(a, N_INT, x, K, bias)
        assert same_bits(plain, kstep(a, x, K, bias))                      # leaf rows copy, interior rows walk: K full steps
        hoisted = interior_forward(a, N_INT, x, K, bias, hoist=True)
        assert same_bits(hoisted[N_INT:], plain[N_INT:])
        assert same_bits(hoisted, plain) == (K == 1)                       # the hoist re-associates: the GPU case tells them apart
        assert np.allclose(hoisted, plain, rtol=1e-4, atol=1e-5)
        y, sacc = interior_transposed(b, N_INT, x, K)
        full = kstep(b, x, K)
        assert same_bits(y[:N_INT], full[:N_INT]) and np.allclose(y, full, rtol=1e-4, atol=1e-5)
        assert same_bits(y, full) == (K == 1)
        assert same_bits(sacc, x[:N_INT]) == (K == 1)
    # every row interior: K full steps; none: the identity
    assert same_bits(interior_forward(a, N_BATCH, x, 4, bias), kstep(a, x, 4, bias))
    assert same_bits(interior_transposed(b, N_BATCH, x, 4)[0], kstep(b, x, 4))
    e = batch("eye")
    assert same_bits(interior_forward(e, 0, x, 2, bias), kstep(e, x, 2, bias))
    assert same_bits(interior_transposed(e, 0, x, 2)[0], kstep(e, x, 1))
