"""The sparse layer-0 projection (pygda_amd/sparse_features.py) on the MI355X against the float32 emulations of
tests/test_sparse_features_host.py, BIT FOR BIT (int32 views: signed zeros count).  tests/test_gpu_spmm.py holds the raw
kernels to their order of operations on square graphs uploaded as raw CSRs; this file holds what lies between a dense
feature matrix and those kernels: ``nonzero`` + the ingestion kernel over ``max(n, f)`` nodes + the edge map, the
rectangular calls on ``n`` or ``f`` of those rows, the split decision per orientation (the designed matrices have rows on
both sides of the chunk threshold and of twice it in BOTH orientations: the hub rows of ``X^T`` are cut), the three
autograd wrappers, dropout on the stored non-zeros, the registry, and the modules that route into it.

Matrices are registered the way the library does it (``Data(...).to``, ``maybe_register``).  Nothing here rests on a number
measured on the device: the host file ties the emulations to the float64 dense product, shows that every cut row (but the
129-entry ones) has other bits chunked than whole at every width used here, and that the 0/1 cases are exact in any order.
The one quantity whose float32 order is not part of this contract, the bias gradient (the column-sum kernel, torch's own
sum behind ``_InputLinear``), is held to float64 under the bound of any summation order, and exactly in the 0/1 cases."""
import functools

import numpy as np
import pytest
import torch

import pygda_amd.nn
from pygda_amd import sparse_features as SF
from pygda_amd.data import Data
from pygda_amd.nn.dgsda_base import _InputLinear
from tests import test_spmm_host as H
from tests import test_sparse_features_host as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.tensor(np.asarray(a), device=DEV)           # (a copy: the shared host arrays are read-only)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy()


def assert_bits(got, want, what):
    g, w = bits(got), H.bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape}, expected {w.shape}"
    bad = np.argwhere(g != w)
    assert not len(bad), (f"{what}: {len(bad)} of {g.size} elements differ in bits, first at {tuple(bad[0].tolist())}, "
                          f"in rows {sorted(set(bad[:, 0].tolist()))[:12]}")


@functools.lru_cache(maxsize=None)
def registered(n, f, variant, values):
    """``(data, sf)``: the design on the device as ``Data.to`` leaves it.  The cache keeps the tensor alive: the registry
    holds a weak reference."""
    x = torch.from_numpy(S.design(n, f, variant, values).copy())
    d = Data(x=x, edge_index=torch.tensor([[0, 1], [1, 0]]), y=torch.zeros(n, dtype=torch.long)).to(DEV)
    sf = SF.lookup(d.x)
    assert sf is not None and d.x.is_contiguous()
    return d, sf


def operands(n, f, h, values):
    w, gy, bias = S.operands(n, f, h, values)
    return dev(w), dev(gy), dev(bias)


def check_bias_grad(gb, n, f, h, values, what):
    """``gy.sum(0)``: exact with integer operands; else float64 under the bound of any order of float32 additions."""
    gy = S.operands(n, f, h, values)[1]
    ref = gy.astype(np.float64).sum(0)
    got = host(gb).astype(np.float64)
    assert got.shape == ref.shape, what
    if values == "binary":
        assert np.array_equal(got, ref), what
    else:
        assert (np.abs(got - ref) <= S.colsum_bound(gy)).all(), what


# ---- 1. ingestion --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("n,f", S.SHAPES)
def test_ingestion(n, f, variant):
    """The dense matrix comes out as the host CSR in both orientations -- entries of a document by ascending word, of a
    word by ascending document --, the edge map is the stable argsort, and either orientation reports long rows exactly
    where the synced rule cuts."""
    _, sf = registered(n, f, variant, "real")
    c = S.host_csr(n, f, variant, "real")
    g, N, nnz = sf.graph, max(n, f), c.nnz
    assert (sf.n, sf.f, sf.nnz) == (n, f, nnz) and g.num_nodes == N and g.nnz == nnz
    for got, want, what in ((g.rowptr[:N + 1], c.fwd.rowptr, "rowptr"), (g.colidx[:nnz], c.fwd.colidx, "colidx"),
                            (g.t_rowptr[:N + 1], c.t.rowptr, "t_rowptr"), (g.t_colidx[:nnz], c.t.colidx, "t_colidx"),
                            (g.t_to_fwd[:nnz], c.t_to_fwd, "t_to_fwd")):
        assert got.dtype == torch.int32 and np.array_equal(host(got), want), what
    assert_bits(g.val[:nnz], c.fwd.val, "val")
    assert_bits(g.t_val[:nnz], c.t.val, "t_val")
    assert sf.t_map.dtype == torch.int64 and np.array_equal(host(sf.t_map), c.t_to_fwd)
    for transposed, a in ((False, c.fwd), (True, c.t)):
        sp, cut = g.split(transposed), H.chunked_rows(a)
        assert sp.counts is None and sp.threshold == H.THRESHOLD
        assert sp.n_long == cut.sum() == S.CUT_ROWS[variant][transposed]
        assert (sp.struct(8) is None) == (not cut.any())
        if cut.any():
            assert sorted(host(sp.long_rows[:sp.n_long]).tolist()) == np.nonzero(cut)[0].tolist()
            assert sp.n_chunks == int((-(-a.lengths[cut] // H.THRESHOLD)).sum())
        else:
            assert sp.n_chunks == 0


# ---- 2. sparse_linear ----------------------------------------------------------------------------------------------------
def run_linear(weight, sf, gy, bias=None):
    """``(y, weight.grad, bias.grad)`` of one forward and backward pass."""
    weight.grad = None
    if bias is not None:
        bias.grad = None
    y = SF.sparse_linear(weight, sf, bias=bias)
    y.backward(gy)
    return y.detach(), weight.grad, None if bias is None else bias.grad


@pytest.mark.parametrize("values", S.VALUES)
@pytest.mark.parametrize("h", S.WIDTHS)
@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("n,f", S.SHAPES)
def test_sparse_linear(n, f, variant, h, values):
    _, sf = registered(n, f, variant, values)
    w, gy, b = operands(n, f, h, values)
    want_y, want_gwt, _ = S.reference(n, f, variant, values, h)
    want_yb = S.reference(n, f, variant, values, h, True)[0]
    for with_bias in (False, True):
        what = f"({n}, {f}) {variant} {values} h={h} bias={with_bias}"
        weight = torch.nn.Parameter(w.clone())
        bias = torch.nn.Parameter(b.clone()) if with_bias else None
        y, gw, gb = run_linear(weight, sf, gy, bias)
        assert_bits(y, want_yb if with_bias else want_y, f"{what}: y")
        assert_bits(gw.t(), want_gwt, f"{what}: gW^T")
        # named: the empty document, the unused word, the gradient's layout
        assert_bits(y[0], host(b) if with_bias else np.zeros(h, np.float32), f"{what}: the empty document's row")
        assert not bits(gw[:, 0]).any(), f"{what}: the unused word's gradient column is not +0"
        assert gw.shape == weight.shape == (h, f) and gw.stride() == weight.stride() == (1, h), what
        assert_bits(weight, host(w), f"{what}: the weight's values after the re-layout")
        if with_bias:
            check_bias_grad(gb, n, f, h, values, f"{what}: gb")
        y2, gw2, gb2 = run_linear(weight, sf, gy, bias)
        assert np.array_equal(bits(y), bits(y2)) and np.array_equal(bits(gw), bits(gw2)), f"{what}: two runs differ"
        assert gb is None or np.array_equal(bits(gb), bits(gb2)), f"{what}: two runs differ in gb"
        if values == "binary":                   # every sum is an integer below 2^24: the float64 dense product, exactly
            x64 = S.design(n, f, variant, values).astype(np.float64)
            y64 = x64 @ host(w).astype(np.float64).T + (host(b).astype(np.float64) if with_bias else 0.0)
            assert np.array_equal(host(y).astype(np.float64), y64), f"{what}: y against float64"
            assert np.array_equal(host(gw).astype(np.float64), host(gy).astype(np.float64).T @ x64), f"{what}: gW against float64"


# ---- 3. sparse_matmul ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", S.VALUES)
@pytest.mark.parametrize("h", S.MATMUL_WIDTHS)
@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("n,f", S.SHAPES)
def test_sparse_matmul(n, f, variant, h, values):
    """The ``[f, h]`` weight as stored: the same sums as ``sparse_linear`` of its transpose."""
    _, sf = registered(n, f, variant, values)
    w, gy, _ = operands(n, f, h, values)
    want_y, want_gw, _ = S.reference(n, f, variant, values, h)
    what = f"({n}, {f}) {variant} {values} h={h}"
    weight = torch.nn.Parameter(w.t().contiguous())
    runs = []
    for _ in range(2):
        weight.grad = None
        y = SF.sparse_matmul(sf, weight)
        y.backward(gy)
        runs.append((y.detach(), weight.grad))
    y, gw = runs[0]
    assert_bits(y, want_y, f"{what}: y")
    assert gw.shape == (f, h) and gw.is_contiguous() and weight.is_contiguous(), what
    assert_bits(gw, want_gw, f"{what}: gW")
    assert not bits(y[0]).any() and not bits(gw[0]).any(), f"{what}: the empty document / the unused word"
    assert np.array_equal(bits(y), bits(runs[1][0])) and np.array_equal(bits(gw), bits(runs[1][1])), f"{what}: two runs differ"
    if values == "binary":
        x64 = S.design(n, f, variant, values).astype(np.float64)
        assert np.array_equal(host(y).astype(np.float64), x64 @ host(w).astype(np.float64).T), what
        assert np.array_equal(host(gw).astype(np.float64), x64.T @ host(gy).astype(np.float64)), what


# ---- 4. sparse_linear_colmajor -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", S.VALUES)
@pytest.mark.parametrize("h", S.COLMAJOR_WIDTHS)
@pytest.mark.parametrize("variant", ["none", "t_only"])
@pytest.mark.parametrize("n,f", S.COLMAJOR_SHAPES)
def test_sparse_linear_colmajor(n, f, variant, h, values):
    """Whole forward rows: the projection writes ``[h, round_up(n, 4)]`` itself, pad columns +0.  The gradient arrives in
    that layout; what its pad columns hold is not read.  On ``"t_only"`` the weight gradient walks cut rows."""
    from pygda_amd.ops import ColMajor
    _, sf = registered(n, f, variant, values)
    w, gy, _ = operands(n, f, h, values)
    want_y, want_gwt, _ = S.reference(n, f, variant, values, h)
    what = f"({n}, {f}) {variant} {values} h={h}"
    n_pad = (n + 3) // 4 * 4
    weight = torch.nn.Parameter(w.clone())
    out = SF.sparse_linear_colmajor(weight, sf)
    assert isinstance(out, ColMajor) and out.n == n and out.shape == (n, h)
    assert out.t.shape == (h, n_pad) and out.t.is_contiguous(), what
    assert_bits(out.t[:, :n], want_y.T, f"{what}: the live columns")
    assert not bits(out.t[:, n:]).any(), f"{what}: a pad column is not +0"
    assert_bits(out.dense(), want_y, f"{what}: dense()")
    gT = torch.full((h, n_pad), 3.0, device=DEV)
    gT[:, :n] = gy.t()
    (gw,) = torch.autograd.grad(out.t, weight, gT)
    assert gw.shape == (h, f) and gw.stride() == weight.stride() == (1, h), what
    assert_bits(gw.t(), want_gwt, f"{what}: gW^T")
    assert not bits(gw[:, 0]).any(), f"{what}: the unused word's gradient column is not +0"
    if values == "binary":
        x64 = S.design(n, f, variant, values).astype(np.float64)
        assert np.array_equal(host(out.t[:, :n]).astype(np.float64), host(w).astype(np.float64) @ x64.T), what
        assert np.array_equal(host(gw).astype(np.float64), host(gy).astype(np.float64).T @ x64), what


@pytest.mark.parametrize("n,f", S.COLMAJOR_SHAPES)
def test_sparse_linear_colmajor_declines_long_documents(n, f):
    _, sf = registered(n, f, "both", "real")
    for h in S.COLMAJOR_WIDTHS:
        weight = torch.nn.Parameter(operands(n, f, h, "real")[0])
        assert SF.sparse_linear_colmajor(weight, sf) is None
        assert weight.is_contiguous()


# ---- 5. dropout on the stored non-zeros ----------------------------------------------------------------------------------
def densify(rowptr, colidx, val_bits, N, transposed):
    """The ``[document, word]`` matrix of int32 value bits a CSR describes (no entry stored twice)."""
    rows = np.repeat(np.arange(N), np.diff(rowptr[:N + 1].astype(np.int64)))
    m = np.zeros((N, N), np.int32)
    if transposed:
        m[colidx, rows] = val_bits
    else:
        m[rows, colidx] = val_bits
    return m


@pytest.mark.parametrize("p", [0.5, 0.25])
@pytest.mark.parametrize("variant", ["t_only", "both"])
@pytest.mark.parametrize("n,f", S.SHAPES)
def test_dropout_on_the_stored_values(n, f, variant, p):
    _, sf = registered(n, f, variant, "real")
    c = S.host_csr(n, f, variant, "real")
    g, N, nnz = sf.graph, max(n, f), c.nnz
    torch.manual_seed(1234)
    val, t_val = sf.dropped_values(p)
    assert val.shape == t_val.shape == (nnz,) and val.dtype == t_val.dtype == torch.float32
    v = host(val)
    kept = v != 0                                                 # (no stored value is zero)
    scaled = c.fwd.val.astype(np.float64) / (1.0 - p)
    if p == 0.5:
        assert np.array_equal(v[kept].astype(np.float64), scaled[kept])
    else:                                                         # 1 / (1 - p) and the product are rounded: 2 x 2^-24 < 1e-6
        assert (np.abs(v[kept] - scaled[kept]) <= 1e-6 * np.abs(scaled[kept])).all()
    # "keep" and not "drop": at p = 0.25 three quarters stay, within five standard deviations
    share = kept.mean()
    assert abs(share - (1.0 - p)) <= 5 * np.sqrt(p * (1 - p) / nnz), f"kept share {share:.4f} at p = {p}"
    # the two value arrays describe one matrix
    fwd = densify(host(g.rowptr), host(g.colidx[:nnz]), bits(val), N, False)
    tr = densify(host(g.t_rowptr), host(g.t_colidx[:nnz]), bits(t_val), N, True)
    assert np.array_equal(fwd, tr), "the forward and the transposed values describe different matrices"
    assert np.array_equal((fwd & 0x7FFFFFFF) != 0, densify(c.fwd.rowptr, c.fwd.colidx, kept.astype(np.int32), N, False) != 0)
    # and the product with them is the emulation on the CSR that carries them (dropped entries stay stored, as +-0)
    d = c.with_values(v)
    assert np.array_equal(H.bits(d.t.val), bits(t_val))
    for h in (6, 128):
        w, gy, b = operands(n, f, h, "real")
        weight, bias = torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
        y = SF._SparseLinear.apply(weight, sf, (val, t_val), bias)
        gw, gb = torch.autograd.grad(y, [weight, bias], gy)
        assert_bits(y, S.emu_forward(d, np.ascontiguousarray(host(w).T), host(b)), f"p={p} h={h}: y")
        assert_bits(gw.t(), S.emu_weight_grad(d, host(gy)), f"p={p} h={h}: gW^T")
        check_bias_grad(gb, n, f, h, "real", f"p={p} h={h}: gb")


def test_sparse_linear_draws_a_fresh_mask_per_call():
    """``sparse_linear(dropout=p)`` is ``_SparseLinear`` on ``dropped_values(p)`` drawn from the generator's state."""
    n, f = S.SHAPES[0]
    _, sf = registered(n, f, "t_only", "real")
    w, gy, _ = operands(n, f, 6, "real")
    weight = torch.nn.Parameter(w.clone())
    torch.manual_seed(77)
    y = SF.sparse_linear(weight, sf, dropout=0.5)
    (gw,) = torch.autograd.grad(y, weight, gy)
    y_next = SF.sparse_linear(weight, sf, dropout=0.5)
    torch.manual_seed(77)
    val, t_val = sf.dropped_values(0.5)
    d = S.host_csr(n, f, "t_only", "real").with_values(host(val))
    assert_bits(y, S.emu_forward(d, np.ascontiguousarray(host(w).T)), "y")
    assert_bits(gw.t(), S.emu_weight_grad(d, host(gy)), "gW^T")
    assert not np.array_equal(bits(y), bits(y_next))


# ---- 6. the comparison sees an error -------------------------------------------------------------------------------------
def test_the_comparison_sees_one_ulp_in_one_transposed_value(capsys):
    """One stored value of the transposed CSR one ulp off -- the first entry of the second chunk of the all-documents word
    -- fails the bit comparison of ``gW``, in that word's column and nowhere else; the forward pass does not read it."""
    n, f = S.SHAPES[0]
    h = S.ULP_WIDTH
    _, sf = registered(n, f, "t_only", "real")
    c = S.host_csr(n, f, "t_only", "real")
    k, off_val = S.one_ulp_off(c)
    g = sf.graph
    t_val = g.t_val.clone()
    t_val[k] = torch.nextafter(t_val[k], torch.tensor(float("inf"), device=DEV))
    changed = np.nonzero(bits(t_val[:c.nnz]) != H.bits(c.t.val))[0]
    assert changed.tolist() == [k] and np.array_equal(bits(t_val[:c.nnz]), H.bits(c.with_values(off_val).t.val))
    w, gy, _ = operands(n, f, h, "real")
    weight = torch.nn.Parameter(w.clone())
    y = SF._SparseLinear.apply(weight, sf, (g.val, t_val), None)
    (gw,) = torch.autograd.grad(y, weight, gy)
    want_y, want_gwt, _ = S.reference(n, f, "t_only", "real", h)
    assert_bits(y, want_y, "y")
    with pytest.raises(AssertionError) as caught:
        assert_bits(gw.t(), want_gwt, "gW^T with one value one ulp off")
    with capsys.disabled():
        print(f"\n{caught.value}")
    assert f"in rows [{S.ALL_DOCS_WORD}]" in str(caught.value)
    differ = (bits(gw.t()) != H.bits(want_gwt)).any(axis=1)
    assert np.nonzero(differ)[0].tolist() == [S.ALL_DOCS_WORD]
    assert_bits(gw.t(), S.emu_weight_grad(c.with_values(off_val), host(gy)), "gW^T against the emulation of the changed CSR")


# ---- 7. the registry -----------------------------------------------------------------------------------------------------
def test_registry_knows_the_very_tensor_only():
    n, f = S.SHAPES[0]
    x = dev(S.design(n, f, "t_only", "real"))
    nnz = int((x != 0).sum())
    sf = SF.maybe_register(x)
    assert sf is not None and SF.lookup(x) is sf and SF.maybe_register(x) is sf and sf.nnz == nnz
    assert SF.lookup(x.clone()) is None
    rows = x[:n - 1]
    assert rows.data_ptr() == x.data_ptr() and rows.is_contiguous() and SF.lookup(rows) is None
    assert SF.lookup(x.view(n, f)) is None                       # another tensor object on the same memory
    assert x[0, 0] == 0
    x[0, 0] = 2.5                                                # the empty document's unused word
    assert SF.lookup(x) is None                                  # edited in place: the CSR is stale
    sf2 = SF.maybe_register(x)
    assert sf2 is not None and sf2 is not sf and SF.lookup(x) is sf2 and sf2.nnz == nnz + 1
    g = sf2.graph
    assert host(g.rowptr[:2]).tolist() == [0, 1] and int(g.colidx[0]) == 0 and float(g.val[0]) == 2.5
    assert host(g.t_rowptr[:2]).tolist() == [0, 1] and int(g.t_colidx[0]) == 0 and float(g.t_val[0]) == 2.5
    # never sparse: narrow, not contiguous, differentiated, dense
    narrow = dev(S.design(n, f, "t_only", "real")[:, :255].copy())
    assert SF.maybe_register(narrow) is None and SF.lookup(narrow) is None
    assert SF.maybe_register(dev(S.design(n, f, "t_only", "real")[:, :256].copy())) is not None
    strided = dev(S.design(n, f, "t_only", "real").T.copy()).t()
    assert strided.shape == (n, f) and not strided.is_contiguous()
    assert SF.maybe_register(strided) is None and SF.lookup(strided) is None
    leaf = dev(S.design(n, f, "t_only", "real")).requires_grad_()
    assert SF.maybe_register(leaf) is None and SF.lookup(leaf) is None


def test_registry_density_threshold():
    """``DENSITY_THRESHOLD`` itself is sparse; one more non-zero is dense."""
    n, f = 50, 300
    at = int(SF.DENSITY_THRESHOLD * n * f)
    assert at / (n * f) == SF.DENSITY_THRESHOLD and (at + 1) / (n * f) > SF.DENSITY_THRESHOLD
    flat = np.zeros(n * f, np.float32)
    flat[np.random.default_rng(0).permutation(n * f)[:at + 1]] = 1.0
    over = dev(flat.reshape(n, f))
    assert SF.maybe_register(over) is None and SF.lookup(over) is None
    flat[np.nonzero(flat)[0][0]] = 0.0
    exactly = dev(flat.reshape(n, f))
    sf = SF.maybe_register(exactly)
    assert sf is not None and sf.nnz == at and SF.lookup(exactly) is sf


# ---- 8. the modules route into it ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", ["Linear", "PropGCNConv", "_InputLinear"])
@pytest.mark.parametrize("n,f", S.SHAPES)
def test_module_routes(n, f, module):
    h = 6
    d, sf = registered(n, f, "t_only", "real")
    w, gy, b = operands(n, f, h, "real")
    want_y, want_gwt, _ = S.reference(n, f, "t_only", "real", h)
    want_yb = S.reference(n, f, "t_only", "real", h, True)[0]
    if module == "Linear":
        m = pygda_amd.nn.Linear(f, h, bias=False).to(DEV)
        weight, bias, run = m.weight, None, lambda: m(d.x)
    elif module == "PropGCNConv":
        m = pygda_amd.nn.PropGCNConv(f, h).to(DEV)
        weight, bias, run = m.lin.weight, m.bias, lambda: m(d.x, d.edge_index, 0)
    else:
        m = _InputLinear(f, h).to(DEV)
        weight, bias, run = m.weight, m.bias, lambda: m(d.x, dropout=0.0)
    with torch.no_grad():
        weight.copy_(w)
        if bias is not None:
            bias.copy_(b)
    y = run()
    assert y.shape == (n, h)
    y.backward(gy)
    assert_bits(y, want_y if bias is None else want_yb, f"{module}: y")       # (a bias added afterwards: the same one sum)
    assert weight.grad.shape == (h, f) and weight.stride() == (1, h)
    assert_bits(weight.grad.t(), want_gwt, f"{module}: gW^T")
    assert_bits(weight, host(w), f"{module}: the weight's values")
    if bias is not None:
        check_bias_grad(bias.grad, n, f, h, "real", f"{module}: gb")
