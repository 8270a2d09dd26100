"""CPU: the public surface of ``svd_transform(..., device=)``, the argument validation of the gda_svd_* entry points
(status codes come back before anything touches a device), and the yardstick of tests/test_gpu_svd_transform.py: a numpy
statement of the reference's randomized SVD on the dense Laplacian in a chosen precision, and the test graphs."""
import ctypes
import functools
import importlib
import inspect

import numpy as np
import pytest
import torch

from pygda_amd import _lib
from pygda_amd.data import Data
from pygda_amd.utils import svd_transform as public_svd_transform

S = importlib.import_module("pygda_amd.utils.svd_transform")    # (the package attribute of that name is the function)

NULL, SIZE, WORKSPACE, UNSUPPORTED, ALIAS = -1, -2, -3, -4, -5


# ------------------------------------------------------------------------------------------------ test graphs --
def quirky(n, hubs, directed=False, seed=0, random_per_node=3):
    """``edge_index`` [2, E] int64: a ring, ``random_per_node * n`` random edges, hubs (node ``h`` gets ``hubs[h]``
    distinct neighbours: distinct large degrees), five duplicated pairs, two self loops; node ``n - 1`` stays isolated.
    Undirected unless ``directed`` (then only the ring and the hub spokes are kept in both directions)."""
    rng = np.random.RandomState(seed)
    m = n - 1                                             # nodes 0 .. m-1 are connected, m is isolated
    src = [np.arange(m)]
    dst = [(np.arange(m) + 1) % m]
    nh = len(hubs)                                        # random edges keep off the hubs: their degrees stay apart
    a, b = rng.randint(nh, m, random_per_node * n), rng.randint(nh, m, random_per_node * n)
    src.append(a[a != b]); dst.append(b[a != b])          # (the two self loops are added below)
    extra_s, extra_d = [], []
    for h, deg in enumerate(hubs):
        nb = rng.choice(np.arange(len(hubs), m), size=deg, replace=False)
        extra_s.append(np.full(deg, h)); extra_d.append(nb)
    s, d = np.concatenate(src), np.concatenate(dst)
    hs, hd = np.concatenate(extra_s), np.concatenate(extra_d)
    if directed:                                          # the random edges one way only
        ring = m
        s = np.concatenate([s, d[:ring], hs, hd])
        d = np.concatenate([d, s[:ring], hd, hs])
    else:
        s, d = np.concatenate([s, d, hs, hd]), np.concatenate([d, s, hd, hs])
    dup = rng.choice(len(s), size=5, replace=False)       # duplicates: counted on the diagonal, once off it
    s, d = np.concatenate([s, s[dup], [3, 7]]), np.concatenate([d, d[dup], [3, 7]])      # ... and two self loops
    return torch.from_numpy(np.stack([s, d]).astype(np.int64))


HUBS_257 = (90, 82, 74, 66, 58, 50, 43, 36)
HUBS_1031 = (200, 181, 163, 146, 130, 112, 90, 70)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "sym257":
        return quirky(257, HUBS_257, seed=1)
    if name == "dir257":
        return quirky(257, HUBS_257, directed=True, seed=2)
    if name == "sym1031":
        return quirky(1031, HUBS_1031, seed=3, random_per_node=10)
    raise KeyError(name)


def breakdown_graph():
    """N = 150: a ring with chords over 80 nodes, 70 isolated nodes -- the Laplacian's rank (79) is below k + 10."""
    a = np.arange(80)
    s = np.concatenate([a, a])
    d = np.concatenate([(a + 1) % 80, (a + 7) % 80])
    return torch.from_numpy(np.stack([np.concatenate([s, d]), np.concatenate([d, s])]).astype(np.int64)), 150


# -------------------------------------------------------------------------------------------------- yardstick --
def reference_transform(edge_index, n, dtype=np.float64):
    """The reference's estimator (sklearn ``TruncatedSVD(k, n_iter=20, random_state=42)`` on the dense Laplacian) with
    every product, QR and SVD in ``dtype``: ``(eival [k], eivec [k, n], L)``.  The normaliser of the power iteration is
    a QR (sklearn's LU keeps the same span)."""
    L = S.laplacian_dense(edge_index, n).astype(dtype)
    k = S.n_components(n)
    Q = np.concatenate([b for _, b in S.draw_q0(n, k + S.OVERSAMPLES)]).astype(dtype)
    for _ in range(S.N_ITER):
        Q = np.linalg.qr(L @ Q)[0]
        Q = np.linalg.qr(L.T @ Q)[0]
    Q = np.linalg.qr(L @ Q)[0]
    _, _, Vt = np.linalg.svd(Q.T @ L, full_matrices=False)
    Vt = Vt[:k]
    top = np.argmax(np.abs(Vt), axis=1)                   # svd_flip(u_based_decision=False): first index on ties
    Vt = Vt * np.sign(Vt[np.arange(k), top])[:, None]
    eival = np.sqrt(np.var(L @ Vt.T, axis=0))
    return eival.astype(dtype), Vt.astype(dtype), L


def test_quirky_graphs_are_what_the_gpu_tests_assume():
    for name, n, hubs in (("sym257", 257, HUBS_257), ("dir257", 257, HUBS_257), ("sym1031", 1031, HUBS_1031)):
        ei = graph(name)
        r, c = ei[0].numpy(), ei[1].numpy()
        assert (r == c).sum() == 2                                              # two self loops
        pairs = r[r != c].astype(np.int64) * n + c[r != c]
        assert len(pairs) - len(np.unique(pairs)) >= 5                          # duplicated pairs
        assert not ((r == n - 1) | (c == n - 1)).any()                          # one isolated node
        L = S.laplacian_dense(ei, n)
        sym = np.array_equal(L, L.T)
        assert sym == (not name.startswith("dir"))
        off = (L < 0).sum(1)
        assert all(off[h] >= hubs[h] for h in range(8)) and off[0] > 2 * 32     # hub 0 is cut into chunks
        sv = np.linalg.svd(L.astype(np.float64), compute_uv=False)
        assert (sv[:8] / sv[1:9]).min() > 1.05, sv[:9]                          # eight separated leading directions
        k = S.n_components(n)
        assert sv[k + S.OVERSAMPLES - 1] > 1e-2 * sv[0]                         # full rank where it is needed
    ei, n = breakdown_graph()
    assert np.linalg.matrix_rank(S.laplacian_dense(ei, n).astype(np.float64)) == 79


def test_q0_in_row_chunks_is_the_reference_stream():
    whole = np.random.RandomState(42).normal(size=(77, 13)).astype(np.float32)
    for rows in (1, 5, 76, 77, 1000):
        got = np.concatenate([b for _, b in S.draw_q0(77, 13, chunk_rows=rows)])
        assert np.array_equal(got, whole), rows
    assert [r0 for r0, _ in S.draw_q0(10, 3, chunk_rows=4)] == [0, 4, 8]


def test_yardstick_agrees_with_the_host_path():
    """At N = 257 the float64 yardstick and sklearn's float32 run describe the same bases."""
    ei = graph("sym257")
    d = public_svd_transform(Data(x=torch.zeros(257, 1), edge_index=ei, y=torch.zeros(257, dtype=torch.int64)))
    eival, eivec, _ = reference_transform(ei, 257)
    np.testing.assert_allclose(d.eival.numpy(), eival, rtol=2e-5)
    lead = d.eivec.numpy()[:8].astype(np.float64)
    assert ((lead * eivec[:8]).sum(1) > 0.9999).all()                           # same directions, same signs
    P0, P1 = d.eivec.numpy().astype(np.float64), eivec
    assert np.linalg.norm(P0.T @ P0 - P1.T @ P1) < 1e-3


# ------------------------------------------------------------------------------------------ the public keyword --
def test_keyword_default_and_alias():
    sig = inspect.signature(public_svd_transform)
    assert list(sig.parameters) == ["data", "processed_paths", "device"]
    assert sig.parameters["device"].default is None and sig.parameters["processed_paths"].default is None
    import pygda.utils
    assert pygda.utils.svd_transform is public_svd_transform is S.svd_transform


def test_device_none_is_the_host_path(tmp_path):
    from sklearn.decomposition import TruncatedSVD
    gen = torch.Generator().manual_seed(4)
    n = 130
    ei = torch.randint(0, n, (2, 700), generator=gen)
    d = Data(x=torch.zeros(n, 1), edge_index=ei, y=torch.zeros(n, dtype=torch.int64))
    public_svd_transform(d, str(tmp_path) + "/", device=None)
    pca = TruncatedSVD(n_components=100, n_iter=20, random_state=42).fit(S.laplacian_dense(ei, n))
    assert d.eival.device.type == "cpu" and d.eival.dtype == torch.float32 and d.eivec.shape == (100, n)
    assert torch.equal(d.eival, torch.tensor(pca.explained_variance_ ** 0.5, dtype=torch.float32))
    assert torch.equal(d.eivec, torch.tensor(pca.components_, dtype=torch.float32))
    assert torch.equal(torch.load(str(tmp_path) + "/eival.pt"), d.eival)
    assert torch.equal(torch.load(str(tmp_path) + "/eivec.pt"), d.eivec)


def test_too_few_nodes_for_the_device_path_names_the_host_path():
    n = 109                                                                     # k + 10 = 110
    d = Data(x=torch.zeros(n, 1), edge_index=torch.zeros(2, 0, dtype=torch.int64), y=torch.zeros(n, dtype=torch.int64))
    with pytest.raises(ValueError, match="host path"):
        public_svd_transform(d, device="cuda:0")                                # refused before any device is touched
    d = Data(x=torch.zeros(1005, 1), edge_index=torch.zeros(2, 0, dtype=torch.int64),
             y=torch.zeros(1005, dtype=torch.int64))
    with pytest.raises(ValueError, match="device=None"):
        public_svd_transform(d, device="cuda:0")                                # k = 1000 from 1000 nodes on


def test_cholesky_factor_trusts_shifts_and_refuses():
    rng = np.random.RandomState(0)
    A = torch.from_numpy(rng.normal(size=(50, 12)))
    R, shifted = S.cholesky_factor(A.T @ A, True)
    assert not shifted and torch.allclose(R.T @ R, A.T @ A) and bool((R == R.triu()).all())
    B = A.clone()
    B[:, 5] = B[:, 4]                                                           # rank 11
    R, shifted = S.cholesky_factor(B.T @ B, True)
    assert shifted and bool(torch.isfinite(R).all())
    with pytest.raises(_lib.GdaError, match="broke down"):
        S.cholesky_factor(B.T @ B, False)
    with pytest.raises(_lib.GdaError, match="broke down"):
        S.cholesky_factor(torch.full((3, 3), float("nan"), dtype=torch.float64), True)
    with pytest.raises(_lib.GdaError, match="broke down"):
        S.cholesky_factor(torch.zeros(3, 3, dtype=torch.float64), True)


# ------------------------------------------------------------------------------------------------ ABI refusals --
def P(addr):
    return ctypes.c_void_p(addr)


# distinct non-NULL dummies, 16-byte aligned: validation comes first, nothing is dereferenced
RP, CI, DG, X, Y, WS, G, MO, LR, LP, CL = (P(0x1000 * k) for k in range(1, 12))


def split(threshold=32, n_long=1, n_chunks=3, long_rows=LR, long_chunk_ptr=LP, chunk_long=CL, counts=None):
    return ctypes.byref(_lib.RowSplitStruct(threshold, n_long, n_chunks, long_rows.value if long_rows else None,
                                            long_chunk_ptr.value if long_chunk_ptr else None,
                                            chunk_long.value if chunk_long else None, None,
                                            counts.value if counts else None))


def apply(rp=RP, ci=CI, dg=DG, n=100, w=110, x=X, ldx=128, y=Y, ldy=128, sp=None, ws=None, ws_bytes=0):
    return _lib.lib().gda_svd_lap_apply_f32(rp, ci, dg, n, w, x, ldx, y, ldy, sp, ws, ws_bytes, None)


def moments(rp=RP, ci=CI, dg=DG, n=100, w=110, x=X, ldx=128, out=MO, sp=None, ws=WS, ws_bytes=1 << 40):
    return _lib.lib().gda_svd_lap_moments_f32(rp, ci, dg, n, w, x, ldx, out, sp, ws, ws_bytes, None)


def gram(y=Y, ldy=128, n=100, w=110, g=G, ldg=110, ws=WS, ws_bytes=1 << 40):
    return _lib.lib().gda_svd_gram_f32(y, ldy, n, w, g, ldg, ws, ws_bytes, None)


def test_lap_apply_validates_its_arguments():
    for missing in ("rp", "dg", "x", "y"):
        assert apply(**{missing: None}) == NULL, missing
    assert apply(n=-1) == SIZE and apply(w=-1) == SIZE and apply(n=1 << 31) == SIZE
    assert apply(ldx=109) == SIZE and apply(ldy=109) == SIZE                   # ld < w
    assert apply(y=X) == ALIAS
    assert apply(w=4097, ldx=4097, ldy=4097) == UNSUPPORTED
    assert apply(n=0, rp=None, dg=None, x=None, y=None) == 0 and apply(w=0, x=None, y=None) == 0    # nothing to do
    # a split layout: its arrays, its sizes, and the chunk partials' workspace
    assert apply(sp=split(long_rows=None)) == NULL and apply(sp=split(chunk_long=None)) == NULL
    assert apply(sp=split(long_chunk_ptr=None)) == NULL
    assert apply(sp=split(threshold=0)) == SIZE and apply(sp=split(n_long=4, n_chunks=3)) == SIZE
    assert apply(sp=split(counts=P(0x9000))) == UNSUPPORTED
    need = _lib.lib().gda_svd_lap_workspace_bytes(100, 110, 1, 3, 0)
    assert need == 3 * 110 * 4 + 8                                              # rounded up to 16 bytes
    assert apply(sp=split()) == WORKSPACE and apply(sp=split(), ws=WS, ws_bytes=need - 1) == WORKSPACE
    assert apply(sp=split(), ws=P(0x6004), ws_bytes=need) == UNSUPPORTED


def test_lap_moments_validates_its_arguments():
    for missing in ("rp", "dg", "x", "out"):
        assert moments(**{missing: None}) == NULL, missing
    assert moments(n=-1) == SIZE and moments(w=-3) == SIZE and moments(ldx=64) == SIZE
    assert moments(out=X) == ALIAS
    assert moments(w=5000, ldx=5000) == UNSUPPORTED
    assert moments(sp=split(long_rows=None)) == NULL and moments(sp=split(threshold=-1)) == SIZE
    L = _lib.lib()
    need = L.gda_svd_lap_workspace_bytes(100, 110, 0, 0, 1)
    assert need == 25 * 4 * 2 * 110 * 8                                        # 25 row blocks of 4 waves, two float64 sums each
    assert moments(ws=None, ws_bytes=0) == WORKSPACE and moments(ws_bytes=need - 1) == WORKSPACE
    assert moments(ws=P(0x6008), ws_bytes=need) == UNSUPPORTED
    assert moments(w=0, x=None, out=None) == 0


def test_gram_validates_its_arguments():
    assert gram(y=None) == NULL and gram(g=None) == NULL
    assert gram(n=-1) == SIZE and gram(w=-1) == SIZE
    assert gram(ldy=109) == SIZE and gram(ldg=109) == SIZE                     # ld < w
    assert gram(g=Y) == ALIAS
    assert gram(w=4097, ldy=4097, ldg=4097) == UNSUPPORTED
    need = _lib.lib().gda_svd_gram_workspace_bytes(100, 110)
    assert need == 3 * 64 * 64 * 4                                             # one slab, three tiles on and below the diagonal
    assert gram(ws=None, ws_bytes=0) == WORKSPACE and gram(ws_bytes=need - 1) == WORKSPACE
    assert gram(ws=P(0x6004), ws_bytes=need) == UNSUPPORTED
    assert gram(w=0, y=None, g=None) == 0


def test_workspace_size_functions():
    L = _lib.lib()
    assert L.gda_svd_lap_workspace_bytes(0, 110, 0, 0, 0) == 0 and L.gda_svd_lap_workspace_bytes(100, 0, 0, 0, 1) == 0
    assert L.gda_svd_lap_workspace_bytes(100, 110, 0, 0, 0) == 0               # no hubs, nothing stored on the side
    # moments: the row blocks are capped at 512, so the partials stop growing with the graph
    big = L.gda_svd_lap_workspace_bytes(10 ** 6, 1010, 0, 0, 1)
    assert big == L.gda_svd_lap_workspace_bytes(10 ** 7, 1010, 0, 0, 1) == 512 * 4 * 2 * 1010 * 8
    # narrow panels: 8 lanes per row, 32 rows per block
    assert L.gda_svd_lap_workspace_bytes(64, 1, 0, 0, 1) == 2 * 32 * 2 * 1 * 8
    # hubs: chunk partials in front, and partials of the long-row pass behind
    assert L.gda_svd_lap_workspace_bytes(100, 110, 2, 7, 1) == 7 * 110 * 4 + 8 + (27 * 4 + 4) * 2 * 110 * 8
    assert L.gda_svd_gram_workspace_bytes(0, 110) == 0 and L.gda_svd_gram_workspace_bytes(5, 4097) == 0
    assert L.gda_svd_gram_workspace_bytes(1, 1) == 64 * 64 * 4
    # 1010 columns: 16 x 17 / 2 tiles, at most 2048 / 136 = 15 row slabs
    assert L.gda_svd_gram_workspace_bytes(10 ** 5, 1010) == 15 * 136 * 64 * 64 * 4
    assert L.gda_svd_gram_workspace_bytes(4099, 110) == 17 * 3 * 64 * 64 * 4


def test_ops_constants_match_the_header():
    from pygda_amd import ops
    assert ops.SVD_SPLIT_THRESHOLD == 32 and ops.SVD_MAX_WIDTH == 4096
    assert ops.svd_panel_ld(110) == 128 and ops.svd_panel_ld(1010) == 1024 and ops.svd_panel_ld(1) == 32
