"""The sparse layer-0 projection (pygda_amd/sparse_features.py) without a GPU: the designed feature matrices, the host
CSRs and the float32 emulations that tests/test_gpu_sparse_features.py compares the device results with bit for bit, and
the conditions those have to meet.

sparse_features.py adds no arithmetic of its own to the CSR SpMM kernels: it ingests a dense ``[n, f]`` matrix into a CSR
of ``N = max(n, f)`` rows (``nonzero`` in row-major order, the ingestion kernel, the edge map), decides per orientation
whether rows are cut into chunks (graph.RowSplit, the synced rule) and calls the kernels on ``n`` or ``f`` of the ``N`` rows.
So its contract is the kernels' (tests/test_spmm_host.py: a row's sum from +0 in CSR order, each product and each sum
rounded on its own; a cut row = its 128-entry partials added in order) on THAT CSR -- built here with numpy:

  sparse_linear            y = chunked_walk(A, W^T)[:n] (+ bias),  gW^T = chunked_walk(A^T, gy)[:f]
  sparse_matmul            the same with the [f, h] weight as stored
  sparse_linear_colmajor   walk(A, W^T)[:n] transposed into [h, round_up(n, 4)], pad columns +0; backward as above from
                           the transposed gradient

The bias gradient is ``gy.sum(0)``: its float32 order belongs to the column-sum kernel, not to this contract, so it is held
to float64 under the bound of any summation order, ``(n - 1) 2^-24 sum |gy|`` (one rounding per addition, n - 1 additions;
``colsum_bound`` gives n 2^-24 for the second-order terms), and exactly where the operands are integers.

Checked here: the matrices have the designed rows and columns (lengths on both sides of the chunk threshold and of twice it
in BOTH orientations, an empty document, an unused word); the split rule cuts exactly the designed rows; the emulations lie
within the derived bound of the float64 dense product; the inputs DISCRIMINATE -- every cut row (but the 129-entry ones)
has other bits chunked than whole at every width the GPU file uses; and with 0/1 values and small integer operands every
order gives the float64 product exactly, so a dropped or doubled entry shows with certainty."""
import functools

import numpy as np
import pytest

from pygda_amd import graph as G
from pygda_amd import sparse_features as SF
from tests import test_spmm_host as H

F32 = np.float32
COUNTS = (0, 1, 127, 128, 129, 255, 256, 257, 384, 385)   # both sides of SPLIT_THRESHOLD = 128 and of twice it
N_NAMED = len(COUNTS)                                     # documents 0 .. 9 and words 0 .. 9 carry the counts
ALL_DOCS_WORD = N_NAMED                                   # word 10: every document from 10 on
BACKGROUND = 0.01
VARIANTS = ("none", "t_only", "both")
VALUES = ("binary", "real")
SHAPES = ((641, 700), (900, 400))                         # f > n with n % 4 == 1; n > f
COLMAJOR_SHAPES = tuple((n, 700) for n in (640, 641, 642, 643))
WIDTHS = (5, 6, 128, 130)                                 # sparse_linear
MATMUL_WIDTHS = (6, 128)
COLMAJOR_WIDTHS = (8, 128)
SEED = 5
# rows the synced rule cuts: (forward, transposed)
CUT_ROWS = {"none": (0, 0), "t_only": (0, 7), "both": (6, 7)}


def caps(variant):
    """``(document cap, word cap)`` on the designed counts."""
    return {"both": (None, None), "t_only": (256, None), "none": (256, 256)}[variant]


def doc_counts(variant):
    cap = caps(variant)[0]
    return tuple(c if cap is None else min(c, cap) for c in COUNTS)


def word_counts(n, variant):
    """Words 0 .. 9 and the all-documents word."""
    cap = caps(variant)[1]
    return tuple(c if cap is None else min(c, cap) for c in COUNTS + (n - N_NAMED,))


@functools.lru_cache(maxsize=None)
def design(n, f, variant, values, seed=SEED):
    """Dense float32 ``[n, f]``.  Document ``i < 10`` has ``COUNTS[i]`` words, all from words >= 11; word ``j < 10`` occurs
    in ``COUNTS[j]`` documents, all from documents >= 10; word 10 occurs in every document from 10 on; the block
    ``[10:, 11:]`` is Bernoulli(0.01).  So document 0 and word 0 are empty, and the block ``[:10, :11]`` is.  ``"t_only"``
    caps the document counts at 256 (the forward side stays whole, X^T chunks: real data), ``"none"`` both sides -- the
    all-documents word included: the longest row is exactly 256 and the synced rule cuts nothing.  ``"binary"``: 0/1;
    ``"real"``: the pattern times standard normal draws."""
    rng = np.random.default_rng(seed)
    pat = np.zeros((n, f), bool)
    pat[N_NAMED:, N_NAMED + 1:] = rng.random((n - N_NAMED, f - N_NAMED - 1)) < BACKGROUND
    for i, c in enumerate(doc_counts(variant)):
        pat[i, rng.choice(np.arange(N_NAMED + 1, f), c, replace=False)] = True
    for j, c in enumerate(word_counts(n, variant)):
        pat[rng.choice(np.arange(N_NAMED, n), c, replace=False), j] = True
    draws = rng.standard_normal((n, f)).astype(F32)
    x = np.where(pat, draws if values == "real" else F32(1.0), F32(0.0))     # (a product would leave -0 off the pattern)
    assert np.array_equal(x != 0, pat) and not H.bits(x)[~pat].any()
    x.setflags(write=False)
    return x


class HostCSR:
    """What ``SparseFeatures(x)`` has to hold: ``fwd`` (rows = documents, entries by ascending word: ``np.nonzero`` in
    row-major order) and ``t`` (rows = words, entries by ascending document: the stable transpose), both embedded in
    ``N = max(n, f)`` rows, and ``t_to_fwd``: the position in ``fwd`` of every entry of ``t``."""

    def __init__(self, x, val=None):
        self.n, self.f = x.shape
        self.N = max(x.shape)
        rows, cols = np.nonzero(x)
        self.nnz = len(rows)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=self.N))])
        self.fwd = H.CSR(self.N, rowptr, cols, x[rows, cols] if val is None else val)
        self.t = H.transpose(self.fwd)
        self.t_to_fwd = np.argsort(self.fwd.colidx, kind="stable").astype(np.int32)

    def with_values(self, val):
        """The same pattern carrying ``val`` (forward order) -- explicit zeros stay stored."""
        out = HostCSR.__new__(HostCSR)
        out.n, out.f, out.N, out.nnz = self.n, self.f, self.N, self.nnz
        out.fwd = H.CSR(self.N, self.fwd.rowptr, self.fwd.colidx, np.asarray(val, F32))
        out.t = H.transpose(out.fwd)
        out.t_to_fwd = self.t_to_fwd
        return out

    def dense(self, transposed=False):
        """The ``[N, N]`` matrix either CSR describes, as ``[row, column]`` (no entry is stored twice)."""
        a = self.t if transposed else self.fwd
        m = np.zeros((self.N, self.N), F32)
        m[a.rows(), a.colidx] = a.val
        return m


@functools.lru_cache(maxsize=None)
def host_csr(n, f, variant, values):
    return HostCSR(design(n, f, variant, values))


def operands(n, f, h, values):
    """``(W [h, f], gy [n, h], bias [h])``: ``default_rng(h)`` standard normal draws with ``"real"`` values, integers in
    [-8, 8] with ``"binary"`` ones (every sum below 2^24: exact in any order)."""
    rng = np.random.default_rng(h)
    if values == "real":
        draw = lambda *s: rng.standard_normal(s).astype(F32)
    else:
        draw = lambda *s: rng.integers(-8, 9, s).astype(F32)
    return draw(h, f), draw(n, h), draw(h)


# ---- the emulations --------------------------------------------------------------------------------------------------------
def emu_forward(c, wt, bias=None, chunk=True):
    """``X wt (+ bias)`` for the gathered operand ``wt [f, h]``: ``[n, h]``."""
    y = (H.chunked_walk(c.fwd, wt, rule="synced") if chunk else H.walk(c.fwd, wt))[:c.n]
    return y if bias is None else y + bias


def emu_weight_grad(c, gy):
    """``X^T gy``: ``[f, h]``."""
    return H.chunked_walk(c.t, np.ascontiguousarray(gy, F32), rule="synced")[:c.f]


def emu_colmajor(c, wt):
    """``(X wt)^T`` as ``[h, round_up(n, 4)]`` from WHOLE rows (the transposed-output kernel never chunks), pad +0."""
    n_pad = (c.n + 3) // 4 * 4
    yT = np.zeros((wt.shape[1], n_pad), F32)
    yT[:, :c.n] = H.walk(c.fwd, wt)[:c.n].T
    return yT


@functools.lru_cache(maxsize=None)
def reference(n, f, variant, values, h, with_bias=False):
    """``(y, gW^T, gb64)`` of ``sparse_linear`` on the design with ``operands(n, f, h, values)``, computed once and never
    written to.  ``gb64``: the float64 column sum of ``gy``."""
    c = host_csr(n, f, variant, values)
    w, gy, bias = operands(n, f, h, values)
    out = (emu_forward(c, np.ascontiguousarray(w.T), bias if with_bias else None), emu_weight_grad(c, gy),
           gy.astype(np.float64).sum(0))
    for a in out:
        a.setflags(write=False)
    return out


def colsum_bound(gy):
    """``|fl(sum) - sum| <= (n - 1) u sum |gy| + O(u^2)`` for any order of the n - 1 additions; ``n u`` covers the rest."""
    return gy.shape[0] * H.EPS * np.abs(gy.astype(np.float64)).sum(0)


# ---- the designs are the designed ones -------------------------------------------------------------------------------------
ALL_SHAPES = SHAPES + tuple(s for s in COLMAJOR_SHAPES if s not in SHAPES)


def test_the_thresholds_are_the_library_s():
    assert H.THRESHOLD == G.SPLIT_THRESHOLD == 128
    assert min(COUNTS[2:]) == H.THRESHOLD - 1 and {H.THRESHOLD + 1, 2 * H.THRESHOLD, 2 * H.THRESHOLD + 1} <= set(COUNTS)
    assert all(f >= SF.MIN_WIDTH for _, f in ALL_SHAPES)
    assert SHAPES[0][1] > SHAPES[0][0] and SHAPES[0][0] % 4 == 1 and SHAPES[1][0] > SHAPES[1][1]
    assert sorted(n % 4 for n, _ in COLMAJOR_SHAPES) == [0, 1, 2, 3]


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,f", ALL_SHAPES)
def test_design_has_the_designed_rows_and_columns(n, f, variant, values):
    x = design(n, f, variant, values)
    pat = x != 0
    assert x.shape == (n, f) and x.dtype == F32 and not np.isnan(x).any()
    assert tuple(pat[:N_NAMED].sum(1)) == doc_counts(variant)
    assert tuple(pat[:, :N_NAMED + 1].sum(0)) == word_counts(n, variant)
    assert not pat[:N_NAMED, :N_NAMED + 1].any()            # the named documents use words >= 11 only, and vice versa
    assert not pat[0].any() and not pat[:, 0].any()         # truly empty: document 0, word 0
    if variant != "none":
        assert pat[N_NAMED:, ALL_DOCS_WORD].all()
    density = pat.mean()
    assert 0.015 <= density <= 0.025 and density <= SF.DENSITY_THRESHOLD
    # the background stays far below the threshold: only designed rows and columns are long
    assert pat[N_NAMED:].sum(1).max() <= 40 and pat[:, N_NAMED + 1:].sum(0).max() <= 40
    if values == "binary":
        assert set(np.unique(x)) == {0.0, 1.0}
    else:
        assert (x[pat] > 0).any() and (x[pat] < 0).any()
        assert np.array_equal(pat, design(n, f, variant, "binary") != 0)      # one pattern, two sets of values
    print(f"({n}, {f}) {variant} {values}: density {density:.4f}, longest background document "
          f"{pat[N_NAMED:].sum(1).max()}, word {pat[:, N_NAMED + 1:].sum(0).max()}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,f", ALL_SHAPES)
def test_host_csr_is_the_matrix_in_both_orientations(n, f, variant):
    x = design(n, f, variant, "real")
    c = host_csr(n, f, variant, "real")
    assert c.N == max(n, f) and c.nnz == int((x != 0).sum()) == c.fwd.rowptr[-1] == c.t.rowptr[-1]
    full = np.zeros((c.N, c.N), F32)
    full[:n, :f] = x
    assert H.same_bits(c.dense(False), full) and H.same_bits(c.dense(True), full.T)
    assert (c.fwd.lengths[n:] == 0).all() and (c.t.lengths[f:] == 0).all()
    for a in (c.fwd, c.t):                                   # strictly ascending inside a row: row-major, stable
        inner = np.diff(a.colidx.astype(np.int64))[np.diff(a.rows()) == 0]
        assert (inner > 0).all()
    # the edge map: entry k of the transposed CSR is entry t_to_fwd[k] of the forward one
    assert sorted(c.t_to_fwd.tolist()) == list(range(c.nnz))
    assert H.same_bits(c.t.val, c.fwd.val[c.t_to_fwd])
    assert np.array_equal(c.t.colidx, c.fwd.rows()[c.t_to_fwd]) and np.array_equal(c.t.rows(), c.fwd.colidx[c.t_to_fwd])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,f", ALL_SHAPES)
def test_the_synced_rule_cuts_the_designed_rows(n, f, variant):
    c = host_csr(n, f, variant, "real")
    cut_f, cut_t = H.chunked_rows(c.fwd), H.chunked_rows(c.t)
    assert (int(cut_f.sum()), int(cut_t.sum())) == CUT_ROWS[variant]
    assert sorted(c.fwd.lengths[cut_f]) == ([129, 255, 256, 257, 384, 385] if variant == "both" else [])
    assert sorted(c.t.lengths[cut_t]) == ([] if variant == "none" else [129, 255, 256, 257, 384, 385, n - N_NAMED])
    assert (np.nonzero(cut_f)[0] < N_NAMED).all() and (np.nonzero(cut_t)[0] <= ALL_DOCS_WORD).all()
    longest = max(c.fwd.lengths.max(), c.t.lengths.max())
    assert longest == (256 if variant == "none" else n - N_NAMED)
    if variant == "none":                                    # rows beyond the threshold that stay whole
        assert (c.fwd.lengths > H.THRESHOLD).sum() == 6 and (c.t.lengths > H.THRESHOLD).sum() == 7


# ---- the emulations against the float64 dense product ----------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,f", SHAPES)
def test_emulations_lie_within_the_bound_of_the_float64_dense_product(n, f, variant):
    """One rounding per product and per sum but the first: ``|emulation - X W^T| <= (L + 1) 2^-24 S`` per element,
    ``S = |X| |W|^T`` (test_walks_lie_within_the_bound_of_float64); ``L + 2`` and ``S + |bias|`` with the bias.  A cut row
    has one more sum than rows (the reduce starts from +0: exact) -- covered."""
    x = design(n, f, variant, "real").astype(np.float64)
    c = host_csr(n, f, variant, "real")
    worst = 0.0
    for h in WIDTHS:
        w, gy, bias = operands(n, f, h, "real")
        w64, gy64 = w.astype(np.float64), gy.astype(np.float64)
        y, gwt, _ = reference(n, f, variant, "real", h)
        yb = reference(n, f, variant, "real", h, True)[0]
        S = np.abs(x) @ np.abs(w64).T
        L = c.fwd.lengths[:n, None]
        cases = (("y", y, x @ w64.T, (L + 1) * H.EPS * S),
                 ("y + bias", yb, x @ w64.T + bias, (L + 2) * H.EPS * (S + np.abs(bias))),
                 ("gW^T", gwt, x.T @ gy64, (c.t.lengths[:f, None] + 1) * H.EPS * (np.abs(x).T @ np.abs(gy64))))
        for what, got, ref, bound in cases:
            err = np.abs(got.astype(np.float64) - ref)
            ratio = (err / np.where(bound > 0, bound, 1)).max()
            worst = max(worst, ratio)
            print(f"({n}, {f}) {variant} h={h} {what}: worst |emulation - f64| {err.max():.3g} on values up to "
                  f"{np.abs(ref).max():.3g}, / bound = {ratio:.3f}")
            assert (err <= bound).all(), what
        if variant != "both":                                # the column-major hand-over: the same sums, transposed
            yT = emu_colmajor(c, np.ascontiguousarray(w.T))
            assert H.same_bits(yT[:, :n].T, y) and not H.bits(yT[:, n:]).any()
    print(f"({n}, {f}) {variant}: worst |emulation - f64| / bound = {worst:.3f}")


def test_bias_gradient_bound_holds_for_sequential_and_pairwise_sums():
    """The bound the device bias gradient is held to, on two float32 orders a column-sum kernel could take."""
    for n, h in ((641, 130), (900, 5)):
        gy = operands(n, 700, h, "real")[1]
        seq = np.zeros(h, F32)
        for r in range(n):
            seq = seq + gy[r]
        pair = gy.copy()
        while len(pair) > 1:
            if len(pair) % 2:
                pair = np.concatenate([pair, np.zeros((1, h), F32)])
            pair = pair[0::2] + pair[1::2]
        ref = gy.astype(np.float64).sum(0)
        for got in (seq, pair[0], gy.sum(0, dtype=F32)):
            assert (np.abs(got.astype(np.float64) - ref) <= colsum_bound(gy)).all()


# ---- the inputs discriminate -----------------------------------------------------------------------------------------------
def cut_rows_that_differ(a, x):
    """``(cut rows, of which differ in bits between the chunked and the whole walk, lengths of those that do not)``."""
    cut = H.chunked_rows(a)
    moved = H.rows_differ(H.walk(a, x), H.chunked_walk(a, x, rule="synced"))
    assert not moved[~cut].any()
    return int(cut.sum()), int(moved[cut].sum()), sorted(a.lengths[cut & ~moved].tolist())


@pytest.mark.parametrize("h", WIDTHS)
@pytest.mark.parametrize("n,f", SHAPES)
def test_every_cut_row_differs_from_its_whole_walk(n, f, h):
    """A reduce that ignored the chunks, chunk blocks that were never launched or a split decision taken the other way
    cannot pass the bit comparison: 5 of the 6 forward and 6 of the 7 transposed cut rows change bits -- all but the
    129-entry ones, which cannot (test_spmm_host.test_every_chunked_row_differs_from_its_whole_walk)."""
    w, gy, _ = operands(n, f, h, "real")
    c = host_csr(n, f, "both", "real")
    assert cut_rows_that_differ(c.fwd, np.ascontiguousarray(w.T)) == (6, 5, [H.THRESHOLD + 1])
    assert cut_rows_that_differ(c.t, gy) == (7, 6, [H.THRESHOLD + 1])
    c = host_csr(n, f, "t_only", "real")
    assert cut_rows_that_differ(c.fwd, np.ascontiguousarray(w.T)) == (0, 0, [])
    assert cut_rows_that_differ(c.t, gy) == (7, 6, [H.THRESHOLD + 1])


@pytest.mark.parametrize("h", COLMAJOR_WIDTHS)
@pytest.mark.parametrize("n,f", COLMAJOR_SHAPES)
def test_cut_rows_differ_at_the_colmajor_shapes(n, f, h):
    gy = operands(n, f, h, "real")[1]
    assert cut_rows_that_differ(host_csr(n, f, "t_only", "real").t, gy) == (7, 6, [H.THRESHOLD + 1])


ULP_WIDTH = 128          # one ulp of one value survives the 127 sums behind it in few columns only: a wide gradient shows it


def one_ulp_off(c):
    """``(k, forward values)``: ``k`` = the first entry of the second chunk of the all-documents word in the transposed
    CSR, its value one ulp up."""
    k = int(c.t.rowptr[ALL_DOCS_WORD]) + H.THRESHOLD
    val = c.fwd.val.copy()
    val[c.t_to_fwd[k]] = np.nextafter(val[c.t_to_fwd[k]], F32(np.inf))
    return k, val


def test_one_ulp_in_one_stored_value_moves_one_column_only():
    """What the GPU file's self-check does on the device: that entry one ulp up changes ``gW[:, 10]`` and nothing else."""
    n, f = SHAPES[0]
    c = host_csr(n, f, "t_only", "real")
    gy = operands(n, f, ULP_WIDTH, "real")[1]
    assert c.t.lengths[ALL_DOCS_WORD] == n - N_NAMED > 2 * H.THRESHOLD
    k, val = one_ulp_off(c)
    off = c.with_values(val)
    assert (H.bits(off.t.val) != H.bits(c.t.val)).sum() == 1 and abs(int(H.bits(off.t.val)[k]) - int(H.bits(c.t.val)[k])) == 1
    ref, got = emu_weight_grad(c, gy), emu_weight_grad(off, gy)
    moved = H.rows_differ(ref, got)
    assert np.array_equal(np.nonzero(moved)[0], [ALL_DOCS_WORD])
    print(f"one ulp: {(H.bits(ref) != H.bits(got)).sum()} of {ULP_WIDTH} elements of gW[:, {ALL_DOCS_WORD}] differ")


# ---- binary values, integer operands: every order is exact -----------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,f", SHAPES)
def test_binary_integer_products_are_exact(n, f, variant):
    x = design(n, f, variant, "binary")
    c = host_csr(n, f, variant, "binary")
    for h in WIDTHS:
        w, gy, bias = operands(n, f, h, "binary")
        assert np.abs(w).max() <= 8 and np.abs(gy).max() <= 8 and (w == np.round(w)).all()
        y64 = x.astype(np.float64) @ w.astype(np.float64).T
        g64 = x.astype(np.float64).T @ gy.astype(np.float64)
        assert (np.abs(x) @ np.abs(w).T).max() + 8 < 2 ** 24 and (np.abs(x).T @ np.abs(gy)).max() < 2 ** 24
        assert np.array_equal((x @ w.T).astype(np.float64), y64) and np.array_equal((x.T @ gy).astype(np.float64), g64)
        y, gwt, gb = reference(n, f, variant, "binary", h)
        # (a -0 cannot arise: every sum starts from +0)
        assert H.same_bits(y, y64.astype(F32)) and H.same_bits(gwt, g64.astype(F32))
        assert H.same_bits(reference(n, f, variant, "binary", h, True)[0], (y64 + bias).astype(F32))
        assert H.same_bits(gy.sum(0, dtype=F32), gb.astype(F32)) and np.abs(gy).sum(0).max() < 2 ** 24
