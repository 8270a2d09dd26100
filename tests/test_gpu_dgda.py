"""DGDA on the MI355X: the kernels of csrc/gda_dgda.hip against float64 -- the bit-adjacency GEMM (forward and as its own
backward) over word and tile edges, the all-pairs reconstruction loss with labels from the bit tile --, the
manipulated adjacency (reproducible per (seed, step), symmetric, diagonal set, degrees and label sum equal to the
popcounts, density within 5 standard deviations of what the rule predicts), the 3-epoch fit against the reference's own
run, eager against captured, one full-size epoch without an N x N float buffer, and DeepWalk's walks.

Every comparison uses test_gpu_asn.py's rule |gpu - f64| <= 8 |fp32 torch - f64| + slack max|f64|.
Slack and what was observed on the MI355X (largest |gpu - f64| / max|f64| of a group; the fp32 torch error was of the
same size in every case, so the 8 x term alone would have held nearly everywhere):
- bit GEMM, forward, dh and dbias: slack 2e-6 (three bf16 terms carry 24 bits, the accumulation is fp32: the class of an
  fp32 product in another order); observed 1.7e-7 over the 22 cases, at most 0.06 of the limit;
- reconstruction loss and dz: slack 1e-5, test_gpu_asn.py's for the same kernel family; observed 5.0e-7, at most 0.04 of
  the limit;
- the 3-epoch fit: losses slack 1e-5, observed 6.8e-8; final parameters and both predict calls slack 1e-4 (three epochs
  of Adam steps amplify a last-bit difference), observed 1.3e-6 and 2.0e-7, at most 0.012 of the limit."""
import numpy as np
import pytest
import torch

import pygda_amd
from pygda_amd import _lib, ops
from pygda_amd.data import Data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(gpu, f32, f64, name, slack):
    """|gpu - f64| <= 8 |fp32 torch - f64| + slack max|f64|."""
    gpu, f32, f64 = (np.asarray(v.detach().double().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
                     for v in (gpu, f32, f64))
    e_gpu, e_ref = np.abs(gpu - f64).max(), np.abs(f32 - f64).max()
    scale = max(np.abs(f64).max(), 1e-30)
    lim = 8 * e_ref + slack * scale
    print(f"[dgda] {name}: gpu {e_gpu:.3e} fp32-torch {e_ref:.3e} rel {e_gpu / scale:.3e} limit {lim:.3e}")
    assert e_gpu <= lim, f"{name}: |gpu - f64| = {e_gpu:.3e} > {lim:.3e} (fp32 torch {e_ref:.3e})"


def _sym01(n, density, seed):
    """A random symmetric 0/1 matrix with a zero row (node 1, when n > 2) and an unset diagonal."""
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(n, n, generator=g) < density).float().tril(-1)
    if n > 2:
        a[1, :] = 0
        a[:, 1] = 0
    return (a + a.t()).to(DEV)


def _bitadj_ref(dense, h, bias, dtype):
    n = dense.size(0)
    b = (dense + 2 * torch.eye(n, device=DEV)).to(dtype)           # the set diagonal bit at weight 2
    dis = b.sum(1).pow(-0.5)
    h = h.detach().to(dtype).requires_grad_(True)
    bias = bias.detach().to(dtype).requires_grad_(True)
    out = dis[:, None] * (b @ (dis[:, None] * h)) + bias
    return out, h, bias


@pytest.mark.parametrize("n,c", [(n, c) for n in (1, 31, 33, 70, 131) for c in (1, 30, 200, 896)]
                         + [(1000, 30), (1000, 896)])
def test_bit_gemm_against_float64_forward_and_as_its_backward(n, c):
    dense = _sym01(n, 0.1 if n > 40 else 0.4, 7 * n + c)
    bits = ops.dgda_pack_bits(dense)
    full = dense.clone()
    full.fill_diagonal_(1.0)
    assert torch.equal(bits.dense(), full)
    assert torch.equal(bits.deg, full.sum(1) + 1)                   # popcount + 1: the diagonal at weight 2
    torch.manual_seed(n * 31 + c)
    h = torch.randn(n, c, device=DEV, requires_grad=True)
    bias = torch.randn(c, device=DEV, requires_grad=True)
    w = torch.randn(n, c, device=DEV)
    out = ops.dgda_bit_propagate(h, bits, bias)
    gh, gb = torch.autograd.grad((out * w).sum(), [h, bias])
    refs = {}
    for dtype in (torch.float64, torch.float32):
        o, hr, br = _bitadj_ref(dense, h, bias, dtype)
        refs[dtype] = (o.detach(), *torch.autograd.grad((o * w.to(dtype)).sum(), [hr, br]))
    for got, a, b, name in zip((out, gh, gb), refs[torch.float32], refs[torch.float64], ("out", "dh", "dbias")):
        _close(got, a, b, f"bit-gemm {name} n={n} c={c}", 2e-6)
    assert torch.equal(out, ops.dgda_bit_propagate(h, bits, bias))          # one accumulation order


def test_bit_gemm_takes_leading_dimensions_and_rejects_what_it_does_not_cover():
    n, c = 70, 30
    dense = _sym01(n, 0.2, 3)
    bits = ops.dgda_pack_bits(dense)
    wide = torch.randn(n, 48, device=DEV)
    out = torch.full((n, 40), 7.0, device=DEV)
    _lib.call("gda_dgda_bitadj_gemm_f32", bits.bits, n, bits.dis, wide, 48, c, None, out, 40, _lib.stream())
    assert torch.equal(out[:, :c], ops.dgda_bit_propagate(wide[:, :c].contiguous(), bits)) and (out[:, c:] == 7).all()
    with pytest.raises(ValueError):
        ops.dgda_bit_propagate(torch.zeros(n + 1, c, device=DEV), bits)
    with pytest.raises(ValueError):
        ops.dgda_recon_loss(torch.zeros(n, ops.DGDA_MAX_K + 1, device=DEV), bits)
    with pytest.raises(ValueError):
        ops.DgdaBits(ops.DGDA_MAX_N + 1, "cpu")


def _recon_ref(z, dense, pw, norm, dtype):
    n = dense.size(0)
    z = z.detach().to(dtype).requires_grad_(True)
    y = (dense + 2 * torch.eye(n, device=DEV)).to(dtype)             # nadj + I: diagonal 2
    x = z @ z.t()
    f = (1 - y) * x + (1 + (pw - 1) * y) * (torch.log1p(torch.exp(-x.abs())) + torch.clamp(-x, min=0))
    loss = norm * f.mean()
    (g,) = torch.autograd.grad(loss, z)
    return loss.detach(), g


@pytest.mark.parametrize("n", [1, 33, 131, 270, 1000])       # 270: ragged, chunks of 3 and 2 tiles, last tile one word
@pytest.mark.parametrize("k", [2, 10, 30, 64, 128])             # every padded width: 8, 16, 32, 64, 128
def test_recon_bits_against_float64(n, k):
    dense = _sym01(n, 0.1 if n > 40 else 0.4, 5 * n + k)
    bits = ops.dgda_pack_bits(dense)
    n_lab, pw, norm, _ = bits.scal.tolist()
    tot, lab = float(n * n), float(dense.sum()) + 2 * n                      # sum(bits) + N with the diagonal set
    assert n_lab == lab and abs(pw - (tot - lab) / lab) <= 1e-6 * abs(pw)
    assert abs(norm - tot / (2 * (tot - lab))) <= 1e-6 * abs(norm)
    torch.manual_seed(n * 131 + k)
    z = (torch.randn(n, k, device=DEV) * (1.5 / k ** 0.5)).requires_grad_(True)
    loss = ops.dgda_recon_loss(z, bits)
    (dz,) = torch.autograd.grad(loss, z)
    l64, g64 = _recon_ref(z, dense, pw, norm, torch.float64)
    l32, g32 = _recon_ref(z, dense, pw, norm, torch.float32)
    _close(loss, l32, l64, f"recon loss n={n} k={k}", 1e-5)
    _close(dz, g32, g64, f"recon dz n={n} k={k}", 1e-5)
    assert torch.equal(dz, torch.autograd.grad(ops.dgda_recon_loss(z, bits), z)[0])


# ------------------------------------------------------------------------------------------- manipulation --
def _edges(n, seed):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n, (2 * n,), generator=g), torch.randint(0, n, (2 * n,), generator=g)
    keep = (src != 1) & (dst != 1)
    src, dst = src[keep], dst[keep]
    src, dst = torch.cat([src, dst, src[:3], torch.tensor([0, n - 1, 2])]), \
        torch.cat([dst, src, dst[:3], torch.tensor([0, 2, n - 1])])           # undirected, duplicates, a self loop
    return torch.stack([src, dst])


def _manip(labels, step, drop=0.1, add=0.1):
    dev = torch.device(DEV)
    ops.dropout_state.counter(dev).fill_(step)
    ops.dropout_state.site = 0
    return ops.dgda_manip_bits(labels, drop, add)


def test_manipulated_bits_are_reproducible_symmetric_and_counted():
    n = 1000
    ei = _edges(n, 5).to(DEV)
    labels = ops.AsnLabels(ei, n)
    a, b, c = _manip(labels, 3), _manip(labels, 3), _manip(labels, 4)
    assert torch.equal(a.bits, b.bits) and not torch.equal(a.bits, c.bits)
    d = a.dense()
    assert torch.equal(d, d.t()) and torch.equal(d.diagonal(), torch.ones(n, device=DEV))
    assert (a.bits.view(-1, a.words)[:, -1] >> (n % 32) == 0).all()         # nothing past column N - 1
    assert torch.equal(a.deg, d.sum(1) + 1) and torch.allclose(a.dis, (d.sum(1) + 1).rsqrt(), rtol=1e-6)
    n_lab, pw, norm, _ = a.scal.tolist()
    lab, tot = float(d.sum()) + n, float(n * n)
    assert n_lab == lab and abs(pw - (tot - lab) / lab) <= 1e-6 * pw and abs(norm - tot / (2 * (tot - lab))) <= 1e-6
    # the density the rule predicts from p_drop, p_add and the edge counts (tests/test_dgda_host.py checks the
    # prediction itself against the dense restatement of drop_edges)
    from tests.test_dgda_host import predicted_bits
    adj = labels.dense()
    mean, std = predicted_bits(adj, 0.1, ops.dgda_p_add(labels, 0.1))
    assert abs(float(d.sum()) - mean) <= 5 * std, (float(d.sum()), mean, std)
    # the rule's corners: nothing added and everything dropped leaves the duplicate edges and the diagonal
    low = torch.tril(adj, -1)
    kept = _manip(labels, 1, drop=1.0, add=0.0).dense().cpu()
    want = (low >= 2).float()
    assert torch.equal(kept, want + want.t() + torch.eye(n))
    assert torch.equal(_manip(labels, 1, drop=0.0, add=0.0).dense().cpu(),
                       ((low > 0) | (low > 0).t()).float() + torch.eye(n))
    dense99 = _manip(labels, 1, drop=0.3, add=0.99)                          # p_add = 0.99 sparsity: nearly all pairs
    mean, std = predicted_bits(adj, 0.3, ops.dgda_p_add(labels, 0.99))
    assert abs(float(dense99.dense().sum()) - mean) <= 5 * std


# ---------------------------------------------------------------------------------------------------- fits --
def test_fit3_against_the_reference_bounded_by_its_float64_run():
    from tests.conftest import load_golden
    from tests.test_dgda_host import _fixture_pair, fixture_model
    g = load_golden("dgda_fit3")
    s, t = _fixture_pair(g)
    m = fixture_model(g, DEV)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
    torch.manual_seed(int(g["init_seed"]))
    m.fit(s, t)
    _close(np.array([l for l, _ in log]), g["losses"], g["f64/losses"], "fit losses", 1e-5)
    assert [a for _, a in log] == list(g["accs"])
    for k, v in m.dgda.state_dict().items():
        _close(v, g["final/" + k], g["f64/final/" + k], k, 1e-4)
    for key in ("tgt_logits_1", "tgt_logits_2"):
        lo, _ = m.predict(s)
        _close(lo, g[key], g["f64/" + key], key, 1e-4)


def _pair(seed, ns=60, nt=45, f=20, c=3):
    def graph(n, s):
        gen = torch.Generator().manual_seed(s)
        return Data(x=torch.rand(n, f, generator=gen), edge_index=_edges(n, s), y=torch.randint(0, c, (n,), generator=gen))
    return graph(ns, seed), graph(nt, seed + 1)


def test_eager_and_captured_fits_are_bit_identical():
    s, t = _pair(12)
    gen = torch.Generator().manual_seed(2)
    emb = (torch.randn(60, 8, generator=gen), torch.randn(45, 8, generator=gen))

    def run(graph):
        m = pygda_amd.models.DGDA(20, 16, 3, dec_dim=8, d_dim=4, y_dim=6, m_dim=5, device=DEV, epoch=7, verbose=0,
                                  lr=1e-2, dropout=0.1, use_hip_graph=graph, epochs_per_graph=3, pretrained_emb=emb)
        log = []
        m.epoch_hook = lambda e, l, a, sec: log.append((l, a))
        torch.manual_seed(0)
        ops.dropout_state.counter(torch.device(DEV)).zero_()
        m.fit(s, t)
        lo, _ = m.predict(t)
        return log, lo, [p.detach().clone() for p in m.dgda.parameters()]

    le, oe, pe = run(False)
    lc, oc, pc = run(True)
    assert len(le) == 7 and le == lc
    assert torch.equal(oe, oc) and all(torch.equal(a, b) for a, b in zip(pe, pc))
    assert len({l for l, _ in le}) == 7                                   # fresh noise and masks every epoch


def test_one_full_size_epoch_at_acm_dblp_shapes_without_an_nxn_float_buffer():
    from bench import make_cfg_a
    src, tgt = make_cfg_a(seed=7, ns=9360, es=15556, nt=5484, et=8117)
    for d in (src, tgt):
        n = d.x.size(0)
        if int(d.edge_index.max()) + 1 != n:
            d.edge_index = torch.cat([d.edge_index, torch.tensor([[n - 1, 0], [0, n - 1]])], 1)
    src, tgt = (Data(x=d.x.to(DEV), edge_index=d.edge_index.to(DEV), y=d.y.to(DEV)) for d in (src, tgt))
    ns, nt, hid, dims, dec, c = 9360, 5484, 64, (16, 32, 16), 32, 5
    gen = torch.Generator().manual_seed(1)
    emb = (torch.randn(ns, 128, generator=gen).to(DEV), torch.randn(nt, 128, generator=gen).to(DEV))
    m = pygda_amd.models.DGDA(src.x.size(1), hid, c, dec_dim=dec, d_dim=dims[0], y_dim=dims[1], m_dim=dims[2],
                              dropout=0.1, device=DEV, epoch=1, verbose=0, pretrained_emb=emb)
    log = []
    m.epoch_hook = lambda e, l, a, sec: log.append(l)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    ws_before = {k: v.numel() for k, v in _lib._ws_cache.items()}
    base0 = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m.fit(src, tgt)                       # the first fit also allocates the kernel workspaces (cached from here on)
    torch.cuda.synchronize()
    grow_first = torch.cuda.max_memory_allocated() - base0
    ws_new = [v.numel() for k, v in _lib._ws_cache.items() if v.numel() > ws_before.get(k, 0)]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m.fit(src, tgt)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    # What a fit allocates, per node row in floats: the encoder's eight [N, hid] tensors (two products and their sum,
    # two aggregations, two activations, one projection), the heads' projection and aggregation [N, W], W = 2 L wide,
    # their mu / lv copies (W) and KLD gradients (W), z and eps (2 L), the entropy's three [N, L], the decoder's three
    # [N, L] and two [N, dec], the domain head (at most L), the classifier (2 L + 3 C).  The backward holds at most one
    # gradient per forward tensor (x 2), both domains' graphs are alive together (ns + nt rows), only one pass at a
    # time.  Beside the rows: the bit matrices and their degrees, and 64 MiB for the parameters, Adam's state, the
    # stacked weights and the CSR structures.
    L = sum(dims)
    cols = 8 * hid + 4 * (2 * L) + 11 * L + 2 * dec + 3 * c
    bound = 2 * cols * 4 * (ns + nt) + sum(n * ((n + 31) // 32) * 4 + 12 * n for n in (ns, nt)) + (64 << 20)
    assert bound < ns * ns * 4                                     # the bound would not admit one N x N float array
    assert len(log) == 2 and all(np.isfinite(v) for v in log)
    print(f"[dgda] full size: first fit {grow_first / 2**20:.1f} MiB (workspaces {sum(ws_new) / 2**20:.1f} MiB), "
          f"second fit {grow / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB, N x N floats {ns * ns * 4 / 2**20:.1f} MiB")
    assert grow < bound, f"the epoch allocated {grow / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB"
    # the first fit: the same buffers plus the workspaces it allocated or enlarged, each sized by its *_workspace_bytes
    # call; none of them is as large as one N x N float array (other trainers' cached scratch is not DGDA's business)
    assert grow_first < bound + sum(ws_new), f"the first fit allocated {grow_first / 2**20:.1f} MiB"
    assert all(v < ns * ns * 4 for v in ws_new), [v >> 20 for v in ws_new]
    logits, _ = m.predict(tgt)
    assert logits.shape == (nt, c) and torch.isfinite(logits).all()


# ------------------------------------------------------------------------------------------------ DeepWalk --
def test_walks_follow_edges_and_the_pretraining_loss_falls():
    from pygda_amd.nn import DWPretrain
    # two 160-cliques and node 320 without edges: three batches per epoch, so five epochs are 15 optimiser steps and
    # the fall of the loss (about 0.3) is well above the sampling noise of the negatives (about 0.05 per epoch)
    a = torch.combinations(torch.arange(160)).t()
    ei = torch.cat([a, a.flip(0), a + 160, (a + 160).flip(0)], 1)
    d = Data(x=torch.zeros(321, 1, device=DEV), edge_index=ei.to(DEV), y=torch.zeros(321, dtype=torch.long, device=DEV))
    torch.manual_seed(0)
    p = DWPretrain(d, epoch=5, embedding_dim=8, walk_length=8, context_size=4, walks_per_node=4, verbose=False)
    start = torch.arange(321, device=DEV).repeat(3)
    w = p.walks(start)
    assert w.shape == (963, 8) and torch.equal(w[:, 0], start)
    dense = torch.zeros(321, 321, dtype=torch.bool, device=DEV)
    dense[ei[0], ei[1]] = True
    moving = start != 320
    assert dense[w[moving, :-1], w[moving, 1:]].all() and (w[~moving] == 320).all()
    assert len(torch.unique(w[:, 1:])) == 321 and (w[:160] < 160).all()              # every node is reached, no clique is left
    losses = [p.train() for _ in range(5)]
    assert losses[-1] < losses[0]
    assert p.get_embedding().shape == (321, 8) and p.get_embedding().is_cuda
