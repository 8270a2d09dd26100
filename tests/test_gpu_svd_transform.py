"""GPU: svd_transform on the device (csrc/gda_svd.hip, pygda_amd/utils/svd_transform.py) against float64.

One bound throughout (tests/test_gpu_cwgcn._close): |gpu - f64| <= 8 |fp32 baseline - f64| + 2e-6 max|f64|.  The kernels'
baselines are the same products in torch fp32 on the dense matrix; the transform's truth is the float64 run of the
reference's estimator (tests/test_svd_device_host.reference_transform), its fp32 baseline the host path (sklearn, live)
at N = 257 and the float32 run of the same yardstick at N = 1031.  Every device result is produced twice and has to
come back with the same bits."""
import functools

import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from pygda_amd.data import Data, to_undirected
from pygda_amd.utils import svd_transform
from pygda_amd.utils.svd_transform import laplacian_dense
from tests import test_svd_device_host as H
from tests.test_gpu_cwgcn import _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0
WIDTHS = (1, 64, 110, 1010)
LEAD = 8                                     # the separated leading directions of the quirky graphs


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def small_graph(n, directed):
    if n == 1:
        return torch.zeros(2, 1, dtype=torch.int64)                             # its self loop only: L = [[0]]
    if n == 63:
        return H.quirky(63, (30, 21), directed=directed, seed=5)
    return H.graph("dir257" if directed else "sym257")


def padded(n, w, gen, fill=SENTINEL):
    """A [n, w] panel inside a sentinel-filled [n, ld] block."""
    block = torch.full((n, ops.svd_panel_ld(w) + 4), fill)
    block[:, :w] = torch.randn(n, w, generator=gen)
    return block


# ---- (1) the operator -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_lap_apply_and_moments_vs_float64(n, directed):
    """L X, L^T X and the column moments of both at every width, into padded panels whose pad columns keep their
    sentinel.  At N = 257 hub 0 (more than 2 x SVD_SPLIT_THRESHOLD entries) goes through the chunked rows."""
    ei = small_graph(n, directed)
    L32 = torch.from_numpy(laplacian_dense(ei, n))
    op = ops.SvdLaplacian(ei.to(DEV), n)
    assert op.threshold == ops.SVD_SPLIT_THRESHOLD == 32
    for transposed in (False, True):
        n_long, n_chunks = op.split_counts(transposed)
        assert (n_long >= 1 and n_chunks >= 3) if n == 257 else n_long == 0
    gen = torch.Generator().manual_seed(n)
    for w in WIDTHS:
        xb = padded(n, w, gen)
        x = xb[:, :w]
        xd = xb.to(DEV)
        for transposed in (False, True):
            A32 = L32.T if transposed else L32
            f64, f32 = A32.double() @ x.double(), A32 @ x
            outs = []
            for _ in range(2):
                yb = torch.full_like(xd, SENTINEL)
                y = op.apply(xd[:, :w], transposed=transposed, out=yb[:, :w])
                assert y.data_ptr() == yb.data_ptr() and bool((yb[:, w:] == SENTINEL).all()), (w, transposed)
                outs.append(yb[:, :w].cpu())
            assert same_bits(*outs), (w, transposed)
            _close(outs[0], f32, f64, f"lap/{n}/{w}/{transposed}")
            m0, m1 = op.moments(xd[:, :w], transposed=transposed), op.moments(xd[:, :w], transposed=transposed)
            assert m0.dtype == torch.float64 and m0.shape == (2, w) and bool((m0 == m1).all())
            _close(m0[0], f32.sum(0), f64.sum(0), f"lap-sum/{n}/{w}/{transposed}")
            _close(m0[1], (f32 * f32).sum(0), (f64 * f64).sum(0), f"lap-sumsq/{n}/{w}/{transposed}")
        assert bool((xd.cpu() == xb).all())                                      # the input, pad included, is intact
    fresh = op.apply(xd[:, :w])                                                  # without `out`: a panel of its own
    assert fresh.shape == (n, w) and (n == 1 or fresh.stride(0) == ops.svd_panel_ld(w))
    _close(fresh.cpu(), L32 @ x, L32.double() @ x.double(), f"lap/{n}/{w}/fresh")


def test_lap_refusals_come_before_a_launch():
    ei = H.graph("sym257").to(DEV)
    with pytest.raises(IndexError, match="must lie in"):
        ops.SvdLaplacian(ei, 200)
    op = ops.SvdLaplacian(ei, 257)
    x = torch.zeros(257, 8, device=DEV)
    with pytest.raises(_lib.GdaError, match="status -5"):
        op.apply(x, out=x)                                                       # y aliases x
    with pytest.raises(ValueError):
        op.apply(torch.zeros(100, 8, device=DEV))
    with pytest.raises(_lib.GdaError):
        op.apply(torch.zeros(257, 8))                                            # a host tensor


# ---- (2) the Gram matrix --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 110, 1010])
@pytest.mark.parametrize("n", [1, 63, 4099])
def test_gram_vs_float64(n, w):
    """Y^T Y for columns of mixed magnitude (1e-3 .. 1e3), ragged widths, N no multiple of the row tile and (N = 4099)
    more than one row slab; G == G^T and two runs agree bit for bit; Y's pad columns are never used."""
    gen = torch.Generator().manual_seed(100 * n + w)
    yb = padded(n, w, gen, fill=float("nan"))
    yb[:, :w] *= 10.0 ** (torch.rand(w, generator=gen) * 6 - 3)
    y = yb[:, :w]
    f64, f32 = y.double().T @ y.double(), y.T @ y
    yd = yb.to(DEV)
    g0, g1 = ops.svd_gram(yd[:, :w]), ops.svd_gram(yd[:, :w])
    assert g0.shape == (w, w) and same_bits(g0, g1) and same_bits(g0, g0.T)
    assert bool(torch.isfinite(g0).all())
    _close(g0, f32, f64, f"gram/{n}/{w}")
    if n == 63 and w > 1:                                                        # rows that are not 16-byte aligned
        off = ops.svd_gram(yd[:, 1:w])
        _close(off, y[:, 1:].T @ y[:, 1:], f64[1:, 1:], f"gram/{n}/{w}/unaligned")
        assert same_bits(off, off.T)
    into = torch.full((w, w + 3), SENTINEL, device=DEV)                          # a padded output keeps its pad
    ops.svd_gram(yd[:, :w], out=into[:, :w])
    assert same_bits(into[:, :w], g0) and bool((into[:, w:] == SENTINEL).all())


def test_panel_matmul_vs_float64():
    """The tall-times-small product of the orthonormalisation on padded panels (gda_gemm_f32, NN), 1010 wide."""
    gen = torch.Generator().manual_seed(3)
    n, w = 300, 1010
    yb, r = padded(n, w, gen), torch.randn(w, w, generator=gen)
    outb = torch.full((n, ops.svd_panel_ld(w)), SENTINEL, device=DEV)
    ops.svd_panel_matmul(yb.to(DEV)[:, :w], r.to(DEV), outb[:, :w])
    assert bool((outb[:, w:] == SENTINEL).all())
    _close(outb[:, :w], yb[:, :w] @ r, yb[:, :w].double() @ r.double(), "panel_matmul")


# ---- (3) the transform ----------------------------------------------------------------------------------------------
def data_of(ei, n):
    return Data(x=torch.zeros(n, 1), edge_index=ei, y=torch.zeros(n, dtype=torch.int64))


@functools.lru_cache(maxsize=None)
def truth(name, n):
    return H.reference_transform(H.graph(name), n)


def bound(e_gpu, e_ref, scale, name, slack=2e-6):
    print(f"{name}: gpu {e_gpu:.3e}  fp32 baseline {e_ref:.3e}  scale {scale:.3e}")
    assert e_gpu <= 8 * e_ref + slack * scale, f"{name}: {e_gpu:.3e} > 8 x {e_ref:.3e} + {slack} x {scale:.3e}"


@pytest.mark.parametrize("name,n", [("sym257", 257), ("dir257", 257), ("sym1031", 1031)])
def test_transform_vs_float64(name, n, tmp_path):
    ei = H.graph(name)
    k = 100 if n < 1000 else 1000
    val64, vec64, L64 = truth(name, n)
    if n < 1000:                                                                 # the host path, live
        h = svd_transform(data_of(ei, n))
        val32, vec32 = h.eival.double().numpy(), h.eivec.double().numpy()
    else:                                                                        # the yardstick in float32
        val32, vec32, _ = H.reference_transform(ei, n, np.float32)
        val32, vec32 = val32.astype(np.float64), vec32.astype(np.float64)
    d = svd_transform(data_of(ei, n), str(tmp_path) + "/", device=DEV)
    assert d.eival.device.type == "cuda" and d.eival.dtype == torch.float32 and d.eival.shape == (k,)
    assert d.eivec.device.type == "cuda" and d.eivec.dtype == torch.float32 and d.eivec.shape == (k, n)
    assert d.eivec.is_contiguous()
    val, vec = d.eival.double().cpu().numpy(), d.eivec.double().cpu().numpy()
    _close(val, val32, val64, f"{name}/eival")
    _close(vec[:LEAD], vec32[:LEAD], vec64[:LEAD], f"{name}/leading rows")      # sign included: the flip rule
    eye = np.eye(k)
    bound(np.abs(vec @ vec.T - eye).max(), np.abs(vec32 @ vec32.T - eye).max(), 1.0, f"{name}/max|V V^T - I|")
    P64 = vec64.T @ vec64
    bound(np.linalg.norm(vec.T @ vec - P64), np.linalg.norm(vec32.T @ vec32 - P64), np.linalg.norm(P64),
          f"{name}/projector")
    again = np.sqrt(np.var(L64 @ vec.T, axis=0))                                 # eival is sqrt(var(L V^T)) of the RETURNED rows
    np.testing.assert_allclose(val, again, rtol=1e-5)
    # the v-based sign rule on every row, and the files
    top = np.abs(vec).argmax(1)
    assert (vec[np.arange(k), top] > 0).all()
    assert torch.equal(torch.load(str(tmp_path) + "/eival.pt"), d.eival.cpu())
    assert torch.equal(torch.load(str(tmp_path) + "/eivec.pt"), d.eivec.cpu())
    assert torch.load(str(tmp_path) + "/eivec.pt").device.type == "cpu"
    if n < 1000:
        d2 = svd_transform(data_of(ei, n), device=DEV)
        assert same_bits(d.eival, d2.eival) and same_bits(d.eivec, d2.eivec)


def test_transform_twice_is_bit_identical_at_1031():
    ei = H.graph("sym1031")
    a, b = svd_transform(data_of(ei, 1031), device=DEV), svd_transform(data_of(ei, 1031), device=DEV)
    assert same_bits(a.eival, b.eival) and same_bits(a.eivec, b.eivec)


def test_breakdown_raises_and_leaves_nothing_behind():
    ei, n = H.breakdown_graph()
    d = data_of(ei, n)
    with pytest.raises(_lib.GdaError, match="broke down"):
        svd_transform(d, device=DEV)
    assert getattr(d, "eival", None) is None and getattr(d, "eivec", None) is None
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(9)
    good = data_of(to_undirected(torch.randint(0, 150, (2, 600), generator=gen), 150), 150)
    svd_transform(good, device=DEV)                                              # the next call works
    assert good.eivec.shape == (100, 150) and bool(torch.isfinite(good.eivec).all() and torch.isfinite(good.eival).all())


def test_out_of_range_indices_are_build_csr_s_error():
    d = data_of(torch.tensor([[0, 300], [1, 2]]), 257)
    with pytest.raises(IndexError, match="must lie in"):
        svd_transform(d, device=DEV)


# ---- (4) SpecReg on device-made bases ---------------------------------------------------------------------------------
def test_specreg_with_ppmi_view_and_device_svd_transform_runs():
    """The fit of tests/test_gpu_parity.test_specreg_with_ppmi_view_and_svd_transform_runs on bases made on the device."""
    gen = torch.Generator().manual_seed(9)

    def domain(n):
        ei = to_undirected(torch.randint(0, n, (2, 4 * n), generator=gen), n)
        return Data(x=(torch.rand(n, 12, generator=gen) < 0.2).float(), edge_index=ei,
                    y=torch.randint(0, 3, (n,), generator=gen))

    s, t = domain(150), domain(120)
    svd_transform(s, device=DEV); svd_transform(t, device=DEV)
    assert s.eivec.shape == (100, 150) and t.eivec.shape == (100, 120) and s.eivec.is_cuda
    m = pygda_amd.models.SpecReg(12, 8, 3, num_layers=2, thr_smooth=0.1, thr_mfr=0.1, device=DEV, epoch=2, verbose=0)
    torch.manual_seed(2)
    m.fit(s, t)
    logits, labels = m.predict(t)
    assert logits.shape == (120, 3) and torch.isfinite(logits).all()
