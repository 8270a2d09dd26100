"""The CSR SpMM kernels (csrc/gda_spmm.hip) on the MI355X against the float32 emulations of tests/test_spmm_host.py, BIT FOR
BIT (int32 views: signed zeros count), at every instantiation the file dispatches to.  The graphs are handed to CSRGraph
as raw CSRs, so the row lengths (on both sides of every lane-group width, of the 4-entry unroll, of the chunk threshold
and of twice the threshold) and the weights are exactly the designed ones; such a graph is neither static nor sampled and
takes the launch chain.

Which width reaches which instantiation is read off ``dispatch`` / ``dispatch_range`` / the ``tout`` entry (fresh
allocations, ld = d; it cannot be observed from outside):

  k_spmm<G, VEC>, plain (test_every_width_whole_rows) and with the epilogue (test_epilogue_*, the width marked *)
    (4,1)  d = 1, 3*       (4,2)  d = 2, 6*        (4,4)  d = 4, 16*
    (8,1)  d = 5, 7*       (8,2)  d = 10, 14*      (8,4)  d = 20*, 32
    (16,1) d = 9, 15*      (16,2) d = 18, 30*      (16,4) d = 36*, 64
    (32,1) d = 17, 31*     (32,2) d = 34, 62*      (32,4) d = 68, 128*, 252
    (64,1) d = 33, 65*, 129  (64,2) d = 66, 130*   (64,4) d = 256, 260*
  (65, 129, 130, 260: a second pass of the column-chunk loop, partly filled.)  Lowered VEC by leading dimension or
  base pointer at d = 128 (test_leading_dimensions_and_base_pointers): (32,4) -> (64,2) -> (64,1); at d = 6: (4,2) -> (8,1).
  Chunk blocks and k_long_reduce, plain and epilogue: test_chunked_rows (d = 5, 6, 128), test_epilogue_* on the split graph.

  k_spmm<G, VEC, false, TOUT> (test_transposed_output)
    (4,4) d = 8    (8,4) d = 24    (16,4) d = 40    (32,4) d = 72    (64,4) d = 256
    (4,1) d = 3    (8,1) d = 6     (16,1) d = 13    (32,1) d = 29    (64,1) d = 70

  k_spmm_range<G, VEC> and k_rows_copy_bias (test_interior_chain)
    (4,4) d = 8    (8,4) d = 24    (16,4) d = 40    (32,4) d = 72    (64,4) d = 260
    (4,1) d = 3    (8,1) d = 6     (16,1) d = 13    (32,1) d = 29    (64,1) d = 70
"""
import functools

import numpy as np
import pytest
import torch

from pygda_amd import _lib, ops
from pygda_amd.graph import SPLIT_THRESHOLD, CSRGraph, build_csr
from tests import test_spmm_host as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A                       # a finite float no sum of these inputs produces

WHOLE_WIDTHS = {(4, 1): (1, 3), (8, 1): (5, 7), (16, 1): (9, 15), (32, 1): (17, 31), (64, 1): (33, 65, 129),
                (4, 2): (2, 6), (8, 2): (10, 14), (16, 2): (18, 30), (32, 2): (34, 62), (64, 2): (66, 130),
                (4, 4): (4, 16), (8, 4): (20, 32), (16, 4): (36, 64), (32, 4): (68, 128, 252), (64, 4): (256, 260)}
EPILOGUE_WIDTHS = {(4, 1): 3, (8, 1): 7, (16, 1): 15, (32, 1): 31, (64, 1): 65, (4, 2): 6, (8, 2): 14, (16, 2): 30,
                   (32, 2): 62, (64, 2): 130, (4, 4): 16, (8, 4): 20, (16, 4): 36, (32, 4): 128, (64, 4): 260}
VEC4_WIDTHS = {(4, 4): 8, (8, 4): 24, (16, 4): 40, (32, 4): 72}
VEC1_WIDTHS = {(4, 1): 3, (8, 1): 6, (16, 1): 13, (32, 1): 29, (64, 1): 70}
TOUT_WIDTHS = {**VEC4_WIDTHS, (64, 4): 256, **VEC1_WIDTHS}
RANGE_WIDTHS = {**VEC4_WIDTHS, (64, 4): 260, **VEC1_WIDTHS}


def predicted(d, vecs=(4, 2, 1)):
    """``(G, VEC)`` as ``dispatch`` picks it for ld = d and 16-byte-aligned bases (``vecs``: the widths the entry knows)."""
    for vec in vecs:
        if d % vec == 0:
            lanes = d // vec
            if vec == 4:                      # the 16-byte form keeps 32 lanes up to 63 of them busy
                return (64 if lanes >= 64 else next((g for g in (32, 16, 8) if lanes > g // 2), 4)), 4
            return next((g for g in (64, 32, 16, 8) if lanes > g // 2), 4), vec


def test_the_tables_name_every_instantiation():
    """The tables above against the thresholds of ``dispatch``, restated in ``predicted``: 15 + 10 + 10, none missing."""
    assert H.THRESHOLD == SPLIT_THRESHOLD
    for (table, vecs) in ((WHOLE_WIDTHS, (4, 2, 1)), (EPILOGUE_WIDTHS, (4, 2, 1)), (TOUT_WIDTHS, (4, 1)), (RANGE_WIDTHS, (4, 1))):
        assert set(table) == {(g, v) for g in (4, 8, 16, 32, 64) for v in vecs}
        for key, ds in table.items():
            assert all(predicted(d, vecs) == key for d in (ds if isinstance(ds, tuple) else (ds,))), key


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy()


def assert_bits(got, want, what):
    g, w = bits(got), H.bits(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert not len(bad), f"{what}: {len(bad)} of {g.size} elements differ in bits, first at {tuple(bad[0])}"


@functools.lru_cache(maxsize=None)
def device_graph(name, transient=False):
    """The host graph as a CSRGraph, its arrays uploaded as they are."""
    h = H.graph(name)
    nnz = int(h.fwd.rowptr[-1])
    g = CSRGraph(h.n, nnz, dev(h.fwd.rowptr), dev(h.fwd.colidx), dev(h.fwd.val), dev(h.t.rowptr), dev(h.t.colidx),
                 dev(h.t.val))
    g._nnz, g.transient = nnz, transient
    return g


def host_csr(name, transposed):
    return H.graph(name).t if transposed else H.graph(name).fwd


@functools.lru_cache(maxsize=None)
def ref_walk(name, transposed, d, seed, rule=None):
    """(a) -- or (b) under ``rule`` -- of ``features(n, d, seed)``, computed once and never written to."""
    a = host_csr(name, transposed)
    x = H.features(a.n, d, seed)
    if rule is not None and not H.chunked_rows(a, rule=rule).any():
        return ref_walk(name, transposed, d, seed)
    y = H.walk(a, x) if rule is None else H.chunked_walk(a, x, rule=rule)
    y.setflags(write=False)
    return y


# ---- 1. every k_spmm instantiation, whole rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("d", sorted(d for ds in WHOLE_WIDTHS.values() for d in ds))
def test_every_width_whole_rows(d, transposed):
    g = device_graph("whole")
    bias = H.bias_of(d)
    y = ops.spmm_kstep(g, dev(H.features(g.num_nodes, d, d)), 1, dev(bias), transposed)
    assert_bits(y, ref_walk("whole", transposed, d, d) + bias, f"d={d} transposed={transposed}")


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("d", [5, 6, 128])                       # one width per VEC: the ping-pong parity of an odd K
def test_three_steps(d, transposed):
    g, a = device_graph("whole"), host_csr("whole", transposed)
    x, bias = H.features(a.n, d, d), H.bias_of(d)
    assert_bits(ops.spmm_kstep(g, dev(x), 3, dev(bias), transposed), H.kstep(a, x, 3, bias), f"K=3 d={d}")
    assert_bits(ops.spmm_kstep(g, dev(x), 2, None, transposed), H.kstep(a, x, 2), f"K=2 d={d}")


def test_through_build_csr():
    """Ingestion in the loop: the edge list of the designed graph, weights as they are, comes out as the designed CSR in
    both orientations (stable order), and aggregates to the same bits."""
    h = H.graph("whole")
    ei = dev(np.stack([h.fwd.colidx.astype(np.int64), h.fwd.rows()]))
    g = build_csr(ei, h.n, dev(h.fwd.val), False, False, False, "col")
    nnz = int(h.fwd.rowptr[-1])
    for got, want in ((g.rowptr, h.fwd.rowptr), (g.colidx[:nnz], h.fwd.colidx), (g.t_rowptr, h.t.rowptr),
                      (g.t_colidx[:nnz], h.t.colidx)):
        assert np.array_equal(got.cpu().numpy(), want)
    assert_bits(g.val[:nnz], h.fwd.val, "val")
    assert_bits(g.t_val[:nnz], h.t.val, "t_val")
    for transposed in (False, True):
        y = ops.spmm_kstep(g, dev(H.features(h.n, 33, 33)), 1, None, transposed)
        assert_bits(y, ref_walk("whole", transposed, 33, 33), f"build_csr transposed={transposed}")


# ---- 2. chunked rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transient", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("d", [5, 6, 128])
def test_chunked_rows(d, transposed, transient):
    """Synced: rows above 128 entries are cut because the longest exceeds 256.  Transient: counts stay on the device, the
    launch is sized by capacities.  Either way a cut row is its 128-entry partials added in order; test_spmm_host.py shows
    that this differs in bits from the whole walk on every cut row (but the 129-entry one), from a reversed reduce and
    from any other chunk size."""
    rule = "deferred" if transient else "synced"
    g, a = device_graph("split", transient), host_csr("split", transposed)
    assert (g.split(transposed).counts is not None) == transient
    bias = H.bias_of(d)
    y = ops.spmm_kstep(g, dev(H.features(a.n, d, H.CHUNK_SEED)), 1, dev(bias), transposed)
    cut = H.chunked_rows(a, rule=rule)
    assert cut.any()
    assert_bits(y[dev(~cut)], (ref_walk("split", transposed, d, H.CHUNK_SEED) + bias)[~cut], "whole rows")
    assert_bits(y, ref_walk("split", transposed, d, H.CHUNK_SEED, rule) + bias, f"d={d} {rule}")


def test_transient_graph_below_twice_the_threshold():
    """The deferred rule cuts the 129 .. 256 rows that the synced rule leaves whole."""
    g, a = device_graph("whole", True), host_csr("whole", False)
    d = 6
    assert H.chunked_rows(a, rule="deferred").sum() == 4 and not H.chunked_rows(a).any()
    y = ops.spmm_kstep(g, dev(H.features(a.n, d, H.CHUNK_SEED)), 1, None, False)
    assert_bits(y, ref_walk("whole", False, d, H.CHUNK_SEED, "deferred"), "deferred")


# ---- 3. the epilogue -----------------------------------------------------------------------------------------------------
EXACT = [dict(alpha=1.0, beta=-1.0), dict(alpha=-1.0, beta=0.5), dict(alpha=0.0, beta=2.0),
         dict(alpha=0.5, beta=2.0, z=True, gamma=-1.0), dict(alpha=2.0, beta=-1.0, z=True, gamma=0.5, gamma_dev=2.0)]


def run_axpby(g, x, z, transposed, alpha, beta, gamma=1.0, gamma_dev=None):
    return ops.spmm_axpby(g, dev(x), alpha, beta, None if z is None else dev(z), gamma,
                          None if gamma_dev is None else dev(np.array([gamma_dev], np.float32)), transposed)


@pytest.mark.parametrize("name", ["whole", "split"])
@pytest.mark.parametrize("d", sorted(EPILOGUE_WIDTHS.values()))
def test_epilogue_with_exact_coefficients(d, name):
    """Coefficients that are powers of two: every product of the epilogue is exact, so a contracted multiply-add gives the
    bits of a separate one and the whole result is fixed: (c) on top of (a) -- of (b) where the split graph is cut."""
    g = device_graph(name)
    for transposed in (False, True):
        a = host_csr(name, transposed)
        x, z = H.features(a.n, d, d), H.features(a.n, d, d + 500)
        acc = ref_walk(name, transposed, d, d, "synced")
        for c in EXACT:
            c = dict(c)
            zz = z if c.pop("z", False) else None
            y = run_axpby(g, x, zz, transposed, **c)
            assert_bits(y, H.epilogue(acc, x, z=zz, **c), f"{name} d={d} transposed={transposed} {c}")


@pytest.mark.parametrize("name", ["whole", "split"])
@pytest.mark.parametrize("d", sorted(EPILOGUE_WIDTHS.values()))
def test_epilogue_with_general_coefficients(d, name):
    """alpha = 0.3, beta = 1.7, g = 3 * 0.37: the compiler may contract, so the yardstick is float64 under the derived
    bound |gpu - f64| <= (L + 6) 2^-24 S, S = |alpha x| + |beta| sum |w x| + |g z| -- one rounding per product (L + 3),
    per sum (L + 2) and for g."""
    g = device_graph(name)
    for transposed in (False, True):
        a = host_csr(name, transposed)
        x, z = H.features(a.n, d, d), H.features(a.n, d, d + 500)
        for zz, gd in ((None, None), (z, None), (z, H.GENERAL["gamma_dev"])):
            c = dict(H.GENERAL, gamma_dev=gd)
            y = run_axpby(g, x, zz, transposed, **c).double().cpu().numpy()
            ref, S = H.epilogue64(a, x, z=zz, **c)
            bound = (a.lengths[:, None] + 6) * H.EPS * S
            err = np.abs(y - ref)
            print(f"{name} d={d} transposed={transposed} z={zz is not None} gamma_dev={gd}: worst |gpu - f64| / bound = "
                  f"{(err / np.where(bound > 0, bound, 1)).max():.3f}")
            assert (err <= bound).all()


# ---- 4. the column-major hand-over ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("d", sorted(TOUT_WIDTHS.values()))
def test_transposed_output(d, transposed):
    """gda_spmm_csr_tout_f32 never chunks: every row of the split graph is a whole walk, written as column ``row`` of
    ``yT [d, ldyT]``; the columns from ``n`` on keep their bits."""
    g, a = device_graph("split"), host_csr("split", transposed)
    rp, ci, va = (g.t_rowptr, g.t_colidx, g.t_val) if transposed else (g.rowptr, g.colidx, g.val)
    n, bias = a.n, H.bias_of(d)
    x = dev(H.features(n, d, d))
    want = (ref_walk("split", transposed, d, d) + bias).T
    for ld in (304, 333):
        yT = torch.full((d, ld), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        _lib.call("gda_spmm_csr_tout_f32", rp, ci, va, n, d, x, d, yT, ld, dev(bias), _lib.stream())
        assert_bits(yT[:, :n], want, f"d={d} ldyT={ld}")
        assert (bits(yT[:, n:]) == SENTINEL).all(), f"d={d} ldyT={ld}: a column beyond n was written"


# ---- 5. leading dimensions and base pointers -----------------------------------------------------------------------------
class Window:
    """An ``[n, d]`` window (leading dimension ``ld``, ``shift`` floats off a 256-byte-aligned base) of a sentinel-filled
    buffer with slack on both sides."""
    PAD = 64

    def __init__(self, n, d, ld, shift, fill=None):
        self.n, self.d, self.ld = n, d, ld
        self.buf = torch.full((2 * self.PAD + n * ld,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0 and (4 * self.PAD) % 16 == 0
        self.off = self.PAD + shift
        self.base = self.buf[self.off:]
        self.rows = self.base[:n * ld].view(n, ld)
        if fill is not None:
            self.rows[:, :d] = dev(fill)

    def outside_untouched(self):
        got = self.buf.clone().view(torch.int32)
        got[self.off:self.off + self.n * self.ld].view(self.n, self.ld)[:, :self.d] = SENTINEL
        return bool((got == SENTINEL).all())


# (ldx, ldy, x shift, y shift, tmp shift): what dispatch has to lower VEC for -- or must not
LD_CASES = {"ld=132": (132, 132, 0, 0, 0), "ld=130": (130, 130, 0, 0, 0), "ld=131": (131, 131, 0, 0, 0),
            "x+1": (128, 128, 1, 0, 0), "x+2": (128, 128, 2, 0, 0), "y+1": (128, 128, 0, 1, 0),
            "y+2,tmp+1": (128, 128, 0, 2, 1), "ldx=130,ldy=132": (130, 132, 0, 0, 0), "x+4": (132, 128, 4, 0, 0)}


@pytest.mark.parametrize("case", sorted(LD_CASES))
def test_leading_dimensions_and_base_pointers(case):
    """d = 128 takes 16-byte accesses only if every leading dimension is a multiple of 4 floats and every base 16-byte
    aligned, 8-byte ones under the same condition at 2 floats / 8 bytes, else scalar ones.  A predicate that let a wide
    access through would not fault here: it would read the neighbouring columns or write them -- so the result has to be
    (a) bit for bit and every float outside the windows of y and tmp has to keep its bits."""
    ldx, ldy, sx, sy, st = LD_CASES[case]
    g, a = device_graph("whole"), host_csr("whole", False)
    n, d = a.n, 128
    x, bias = H.features(n, d, d), H.bias_of(d)
    for K in ((1, 2, 3) if case in ("ld=130", "y+2,tmp+1") else (1,)):
        X, Y, T = Window(n, d, ldx, sx, x), Window(n, d, ldy, sy), Window(n, d, ldy, st)
        _lib.call("gda_spmm_csr_split_f32", g.rowptr, g.colidx, g.val, n, d, K, X.base, ldx, Y.base, ldy,
                  T.base if K > 1 else None, dev(bias), None, _lib.stream())
        want = ref_walk("whole", False, d, d) + bias if K == 1 else H.kstep(a, x, K, bias)
        assert_bits(Y.rows[:, :d], want, f"{case} K={K}")
        assert Y.outside_untouched() and T.outside_untouched(), f"{case} K={K}: a float outside the window was written"
        assert_bits(X.rows[:, :d], x, "x")
        if K > 1:
            assert_bits(T.rows[:, :d], H.kstep(a, x, K - 1), f"{case} K={K}: tmp holds step K - 1")


def test_narrow_rows_with_an_odd_leading_dimension():
    g, a = device_graph("whole"), host_csr("whole", False)
    n, d, ld = a.n, 6, 7
    x = H.features(n, d, d)
    for K in (1, 2):
        X, Y, T = Window(n, d, ld, 0, x), Window(n, d, ld, 0), Window(n, d, ld, 0)
        _lib.call("gda_spmm_csr_split_f32", g.rowptr, g.colidx, g.val, n, d, K, X.base, ld, Y.base, ld,
                  T.base if K > 1 else None, None, None, _lib.stream())
        assert_bits(Y.rows[:, :d], H.kstep(a, x, K), f"d=6 ld=7 K={K}")
        assert Y.outside_untouched() and T.outside_untouched()


# (ldx, ldy, ldz, x shift, y shift, z shift)
Z_CASES = {"z aligned": (128, 128, 128, 0, 0, 0), "ldz=131": (128, 128, 131, 0, 0, 0), "ldz=130": (128, 128, 130, 0, 0, 0),
           "z+2": (128, 128, 128, 0, 0, 2), "z+1": (128, 128, 132, 0, 0, 1), "ld=130,z+2": (130, 130, 128, 0, 0, 2),
           "y+1": (128, 128, 128, 0, 1, 0)}


@pytest.mark.parametrize("case", sorted(Z_CASES))
def test_epilogue_leading_dimensions_and_base_pointers(case):
    ldx, ldy, ldz, sx, sy, sz = Z_CASES[case]
    g, a = device_graph("whole"), host_csr("whole", False)
    n, d = a.n, 128
    x, z = H.features(n, d, d), H.features(n, d, d + 500)
    X, Y, Z = Window(n, d, ldx, sx, x), Window(n, d, ldy, sy), Window(n, d, ldz, sz, z)
    _lib.call("gda_spmm_csr_axpby_f32", g.rowptr, g.colidx, g.val, n, d, X.base, ldx, Y.base, ldy, 0.5, -2.0, Z.base, ldz,
              0.5, dev(np.array([2.0], np.float32)), None, _lib.stream())
    want = H.epilogue(ref_walk("whole", False, d, d), x, 0.5, -2.0, z, 0.5, 2.0)
    assert_bits(Y.rows[:, :d], want, case)
    assert Y.outside_untouched(), f"{case}: a float outside the window was written"


# ---- 6. the interior chain -----------------------------------------------------------------------------------------------
def run_interior(a, n_int, x, K, transposed, bias=None, with_sacc=False):
    """gda_spmm_csr_interior_kstep_f32 itself (no LDS plan, ``sacc`` in the test's hands): ``(y, sacc)``; both start as
    sentinels."""
    n, d = x.shape

    def sentinel(rows):
        return torch.full((max(rows, 1), d), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)

    y, tmp = sentinel(n), sentinel(n_int)
    sacc = sentinel(n_int) if with_sacc or transposed else None
    _lib.call("gda_spmm_csr_interior_kstep_f32", dev(a.rowptr), dev(a.colidx), dev(a.val), n, n_int, d, K, int(transposed),
              dev(x), y, tmp if K > 1 else None, sacc, None if bias is None else dev(bias), _lib.stream())
    return y, sacc


@pytest.mark.parametrize("d", sorted(RANGE_WIDTHS.values()))
def test_interior_chain(d):
    """Forward without ``sacc``: K full steps of (a).  Forward with ``sacc`` (K >= 2): the leaf columns' part formed once,
    a step = interior columns in order, + c, + bias -- other bits than the plain chain (test_spmm_host.py), so the two
    are told apart.  Transposed: the steps, the running sum of their inputs and the leaves' one pass."""
    fwd, bwd = H.batch("fwd"), H.batch("bwd")
    x = H.features(H.N_BATCH, d, d)
    for K in (1, 2, 4):
        for bias in (None, H.bias_of(d)):
            y, _ = run_interior(fwd, H.N_INT, x, K, False, bias)
            assert_bits(y, H.kstep(fwd, x, K, bias), f"forward d={d} K={K} bias={bias is not None}")
            y, _ = run_interior(fwd, H.N_INT, x, K, False, bias, with_sacc=True)
            assert_bits(y, H.interior_forward(fwd, H.N_INT, x, K, bias, hoist=True), f"hoisted d={d} K={K}")
        y, sacc = run_interior(bwd, H.N_INT, x, K, True)
        want_y, want_sacc = H.interior_transposed(bwd, H.N_INT, x, K)
        assert_bits(y, want_y, f"transposed d={d} K={K}")
        assert_bits(sacc, want_sacc, f"transposed d={d} K={K}: the running sum")


@pytest.mark.parametrize("d", [6, 40])
def test_interior_chain_without_interior_and_without_leaves(d):
    x, bias = H.features(H.N_BATCH, d, d), H.bias_of(d)
    eye, fwd, bwd = H.batch("eye"), H.batch("fwd"), H.batch("bwd")
    y, _ = run_interior(eye, 0, x, 2, False, bias, with_sacc=True)             # n_int = 0: the leaves' copy alone
    assert_bits(y, H.self_loop_rows(x, bias), "n_int=0 forward")
    assert_bits(y, H.kstep(eye, x, 2, bias), "n_int=0 forward = two full steps")
    y, _ = run_interior(eye, 0, x, 2, True)
    assert_bits(y, H.interior_transposed(eye, 0, x, 2)[0], "n_int=0 transposed")
    n = H.N_BATCH                                                              # n_int = n_rows: no leaf pass
    for K in (1, 3):
        y, _ = run_interior(fwd, n, x, K, False, bias)
        assert_bits(y, H.kstep(fwd, x, K, bias), f"n_int=n forward K={K}")
        y, _ = run_interior(fwd, n, x, K, False, bias, with_sacc=True)
        assert_bits(y, H.interior_forward(fwd, n, x, K, bias, hoist=True), f"n_int=n hoisted K={K}")
        y, sacc = run_interior(bwd, n, x, K, True)
        want_y, want_sacc = H.interior_transposed(bwd, n, x, K)
        assert_bits(y, want_y, f"n_int=n transposed K={K}")
        assert_bits(sacc, want_sacc, f"n_int=n transposed K={K}: the running sum")


# ---- 7. two runs, the same bits ------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    d = 36
    whole, split, transient = device_graph("whole"), device_graph("split"), device_graph("split", True)
    x, z, bias = dev(H.features(H.N_ROWS, d, d)), dev(H.features(H.N_ROWS, d, d + 500)), dev(H.bias_of(d))
    xb = H.features(H.N_BATCH, d, d)

    def tout():
        yT = torch.zeros(d, 304, device=DEV)
        _lib.call("gda_spmm_csr_tout_f32", split.rowptr, split.colidx, split.val, H.N_ROWS, d, x, d, yT, 304, bias,
                  _lib.stream())
        return yT

    families = {
        "whole rows": lambda: ops.spmm_kstep(whole, x, 3, bias, False),
        "chunked": lambda: ops.spmm_kstep(split, x, 1, bias, True),
        "chunked, deferred": lambda: ops.spmm_kstep(transient, x, 1, bias, False),
        "epilogue": lambda: ops.spmm_axpby(split, x, 0.3, 1.7, z, 1.11),
        "tout": tout,
        "interior forward": lambda: run_interior(H.batch("fwd"), H.N_INT, xb, 4, False, None, with_sacc=True)[0],
        "interior transposed": lambda: run_interior(H.batch("bwd"), H.N_INT, xb, 4, True)[0],
    }
    for name, run in families.items():
        first, second = run(), run()
        assert np.array_equal(bits(first), bits(second)), name
