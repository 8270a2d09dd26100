"""torch.autograd wrappers over the C ABI (include/gda_hip.h).  PyTorch supplies device
memory, the stream and autograd plumbing; every numeric kernel named here is ours."""
import ctypes
import weakref

import os as _os

import torch

from . import _lib, profiler
from .graph import CSRGraph, build_csr


def _f32c(t, name):
    _lib.require_gpu_tensor(t, name)
    if t.dtype != torch.float32:
        raise _lib.GdaError(f"{name}: the aggregation path computes in fp32, got {t.dtype}")
    return t.contiguous()


# ------------------------------------------------- the activation's backward in its producer's epilogue --
# dropout(relu(.)) needs, going backwards, only its own OUTPUT y: gx = (y > 0) * g / (1 - p).  When the gradient g of y has
# exactly one producer and that producer is one of ours, it can apply the mask while it stores g -- the activation's own
# backward launch and one [rows, d] round trip through HBM disappear (cfg-S: ~0.2 ms of a 2.5 ms step).  Protocol: an
# activation that is willing hands its output a GradSink (buffer for the masked gradient, y, p); a sink-aware producer
# (`gemm(GEMM_NN, ..., sink=)`, the one-pass MMD's scatter) writes the MASKED gradient into `sink.buf`, sets `written` and
# returns that buffer; the activation's backward recognises its own buffer and passes it on untouched.  A gradient from a
# producer that wrote no sink arrives as an ordinary gradient and takes the ordinary kernel.  ONLY sound when y has a
# single consumer: a second, sink-unaware consumer's gradient would be summed onto an already masked one and masked
# again -- `GradSink.mine` raises when a written sink meets another tensor.  So sinks are handed out only inside
# `grad_sinks()`, which the A2GNN trainer opens around its sampled step, where every activation output feeds exactly one op.
GRAD_SINKS = True        # tests/test_gpu_sampler.py turns it off for its reference
_sinks_on = False
sink_hits = 0            # activation backward launches that a producer's epilogue made unnecessary (tests read it)


class grad_sinks:
    """``with grad_sinks():`` -- activations created inside may hand out GradSinks (see above)."""

    def __enter__(self):
        global _sinks_on
        self.prev, _sinks_on = _sinks_on, GRAD_SINKS
        return self

    def __exit__(self, *exc):
        global _sinks_on
        _sinks_on = self.prev
        return False


class GradSink:
    __slots__ = ("buf", "y", "p", "written")

    def __init__(self, buf, y, p):
        # (an ALIAS of y, not y itself: y carries this sink as an attribute, and a tensor <-> sink reference cycle would
        # keep every eager step's activations alive until the cyclic collector runs -- which the training loops switch off)
        self.buf, self.y, self.p, self.written = buf, y.detach(), float(p), False

    def mine(self, g):
        """Is ``g`` the masked gradient a producer left in this sink?  (consumes the flag)

        A sink that WAS written while ``g`` is some other tensor means the activation's output had a second consumer (or
        autograd copied the gradient): ``g`` then holds the already masked and 1 / (1 - p)-scaled buffer summed with
        something else, and the ordinary backward would mask and scale that part a second time.  That is an error, not
        a miss."""
        global sink_hits
        written, self.written = self.written, False
        if not written:
            return False
        if g is None or g.data_ptr() != self.buf.data_ptr() or g.shape != self.buf.shape:
            raise _lib.GdaError(
                f"GradSink {tuple(self.buf.shape)} (p = {self.p}): a producer stored this activation's masked gradient in "
                "the sink, but the gradient that arrived is another tensor -- the activation's output has a second consumer "
                "(or its gradient was copied), and masking it again would scale the sink's part by 1 / (1 - p) twice.  "
                "Inside ops.grad_sinks() every activation output must feed exactly one op")
        sink_hits += 1
        return True


def sink_of(t):
    return getattr(t, "_gda_grad_sink", None) if torch.is_tensor(t) else None


def _offer_sink(y, p, buf=None, wanted=True):
    """Attach a sink to the activation output ``y`` when sinks are on and the activation's input wants a gradient."""
    if _sinks_on and wanted and y.is_cuda and y.dim() == 2 and y.size(1) % 4 == 0 and y.is_contiguous():
        y._gda_grad_sink = GradSink(torch.empty_like(y) if buf is None else buf, y, p)
        return y._gda_grad_sink
    return None


def masked_dgrad(gy, weight, sink):
    """``sink.buf <- (sink.y > 0) * (gy @ weight) / (1 - p)`` in the product's epilogue when the kernel takes the shape,
    else product + activation backward as two launches; either way the sink is written."""
    gy, weight = _f32c(gy, "gy"), _f32c(weight, "weight")
    (M, K), (K2, N) = gy.shape, weight.shape
    L = _lib.lib()
    st = L.gda_gemm_nn_mask_f32(M, N, K, gy, K, weight, N, sink.buf, N, sink.y, N, sink.p,
                                _lib.stream()) if (M == sink.buf.size(0) and N == sink.buf.size(1)) else -1
    if st != 0:
        gx = gemm(GEMM_NN, gy, weight)
        _lib.call("gda_relu_dropout_bwd_f32", gx, sink.y, sink.buf, gx.numel(), sink.p, _lib.stream())
    sink.written = True
    return sink.buf


# ------------------------------------------------------ source classification loss --
class _SoftmaxNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        x = _f32c(logits, "logits")
        _lib.require_gpu_tensor(labels, "labels", torch.int64)
        if x.dim() != 2 or labels.dim() != 1 or labels.numel() != x.size(0):
            raise ValueError(f"logits [N, C] and labels [N] expected, got {tuple(x.shape)} and {tuple(labels.shape)}")
        n, c = x.shape
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        stats = torch.empty(2, dtype=torch.float64, device=x.device)       # {loss, #(argmax == label)}: the epoch log
        ws, _ = _lib.scratch("gda_softmax_nll_workspace_bytes", x.device, "ce")
        # a batch padded to a static capacity (pygda_amd/sampled_graph.py) tags its labels with the DEVICE count of its
        # real rows: the loss is their mean, the rows behind them get zero gradients
        ctx.nv = nv = getattr(labels, "_gda_valid_rows", None)
        _lib.call("gda_softmax_nll_fwd_nv_f32", x, c, labels.contiguous(), n, c, nv, loss, stats, ws, ws.numel(),
                  _lib.stream())
        global _ce_stats
        # weak references + version counters: the entry pins neither the [rows, C] logits nor the labels of a sampled
        # batch (the eager loop never looks it up), and a tensor that died -- whose storage may since have been handed
        # to another one -- or was written to can never match
        _ce_stats = (weakref.ref(logits), weakref.ref(labels), n, stats, logits._version, labels._version)
        ctx.save_for_backward(x, labels)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        x, labels = ctx.saved_tensors
        n, c = x.shape
        gx = torch.empty_like(x)
        gl = gl.reshape(1).to(torch.float32).contiguous()
        _lib.call("gda_softmax_nll_bwd_nv_f32", x, c, labels.contiguous(), n, c, ctx.nv, gl, gx, c, _lib.stream())
        return gx, None


_ce_stats = None


def ce_stats_for(logits, labels):
    """``[loss, number of correct argmax predictions]`` (float64, device) left by the LAST softmax_nll call if it
    was made on exactly these logits and labels, else None.  Lets a trainer's epoch log line (loss, source
    micro-F1) ride on the loss kernel instead of an argmax / compare / sum / cast / stack chain."""
    global _ce_stats
    hit, _ce_stats = _ce_stats, None              # consumed by the first look-up: a later loss computed some other
    if hit is None:                                                                         # way never sees it
        return None
    lg, lb = hit[0](), hit[1]()
    if (lg is not None and lb is not None and hit[2] == logits.size(0) and lg.shape == logits.shape
            and lg.data_ptr() == logits.data_ptr() and lb.data_ptr() == labels.data_ptr()
            and lg._version == hit[4] and lb._version == hit[5]):
        return hit[3]
    return None


def softmax_nll(logits, labels):
    """``F.nll_loss(F.log_softmax(logits, dim=1), labels)`` (mean over rows) in one pass each way."""
    return _SoftmaxNLL.apply(logits, labels)


def source_ce(logits, labels):
    """The trainers' source loss line (pygda/models/a2gnn.py:182): fused kernel for device logits with
    up to 64 classes, the torch composition otherwise."""
    if logits.is_cuda and logits.dim() == 2 and logits.size(1) <= 64 and logits.dtype == torch.float32:
        return softmax_nll(logits, labels)
    import torch.nn.functional as F
    return F.nll_loss(F.log_softmax(logits, dim=1), labels)


class _SoftmaxEntropy(torch.autograd.Function):
    """``mean_i sum_c -q log q``, ``q = clamp(softmax(logits_i), lo, 1)`` (gda_softmax_entropy_{fwd,bwd}_f32)."""

    @staticmethod
    def forward(ctx, logits, lo):
        x = _f32c(logits, "logits")
        n, c = x.shape
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        ws, _ = _lib.scratch("gda_softmax_nll_workspace_bytes", x.device, "entropy")
        _lib.call("gda_softmax_entropy_fwd_f32", x, c, n, c, float(lo), loss, ws, ws.numel(), _lib.stream())
        ctx.save_for_backward(x)
        ctx.lo = float(lo)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        (x,) = ctx.saved_tensors
        n, c = x.shape
        gx = torch.empty_like(x)
        gl = gl.reshape(1).to(torch.float32).contiguous()
        _lib.call("gda_softmax_entropy_bwd_f32", x, c, n, c, ctx.lo, gl, gx, c, _lib.stream())
        return gx, None


def softmax_entropy(logits, clamp_min=1e-9):
    """UDAGCN's target entropy term (pygda/models/udagcn.py:193-197): ``p = clamp(softmax(logits, -1), min, 1.0)``,
    ``mean(sum(-p log p, -1))`` -- one row kernel each way for device logits with up to 64 classes, the reference's
    composition otherwise."""
    if (logits.is_cuda and logits.dim() == 2 and 0 < logits.size(1) <= 64 and logits.size(0) > 0
            and logits.dtype == torch.float32):
        return _SoftmaxEntropy.apply(logits, clamp_min)
    import torch.nn.functional as F
    p = torch.clamp(F.softmax(logits, dim=-1), min=clamp_min, max=1.0)
    return torch.mean(torch.sum(-p * torch.log(p), dim=-1))


# --------------------------------------------------------- tall-skinny GEMMs (MFMA) --
GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2


def gemm_raw(mode, M, N, K, a, lda, b, ldb, c, ldc, name="dense_projection"):
    """gda_gemm_f32 on explicit leading dimensions (column-major activations are row-major matrices of the
    transposed shape with a padded leading dimension)."""
    L = _lib.lib()
    need = L.gda_gemm_workspace_bytes(mode, M, N, K)
    ws = _lib.workspace(need, c.device, "gemm") if need else None
    with profiler.region(name, 1, 4 * (M * K + N * K + M * N), 2 * M * N * K):
        _lib.call("gda_gemm_f32", mode, M, N, K, a, lda, b, ldb, c, ldc, ws, ws.numel() if ws is not None else 0,
                  _lib.stream())
    return c


TALL_ROWS = 32768    # node counts from here on: the tall kernels


# the weight gradient gy^T x with one workgroup per row slab (k_tall_wgrad) from 4 k rows on: at cfg-A's stacked source rows
# (18,720) the 64 x 64-tile kernel's 64 slabs took 27 us on the tail of the step, the slab kernel 2 - 3 % off the step; the
# target's 5,484 rows give another 2 % (same box, ms/step: 32768 -> 0.4355 / 0.4338, 8192 -> 0.4271 / 0.4348, 4096 -> 0.4252 / 0.4128)
TALL_WGRAD_ROWS = 4096


def _tall_shape(mode, M, N, K, a, b):
    """The envelope of gda_gemm_tall_f32 (csrc/gda_gemm.hip): sampled sub-graphs (10^5 rows and more) against a weight
    whose extents are 128 or 256."""
    if mode == GEMM_TN:          # gW = gy^T x: `a` = gy [rows, 128], reduction over the rows; 16-byte row loads of both
        return (M == 128 and N in (128, 256) and K >= TALL_WGRAD_ROWS and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0)
    return M >= TALL_ROWS and N in (128, 256) and K in (128, 256) and a.data_ptr() % 16 == 0


SKINNY_ROWS = 2048   # the classifier projection's vector kernels from here on


def _skinny_shape(mode, M, N, K, a, b, c_ld):
    """The envelope of gda_gemm_skinny_f32: the classifier projection (at most 8 classes).  Round 5: from citation size
    on, not only at sampled-batch row counts -- a 64 x 64 matrix-core tile is 92 % padding for 5 classes, and on the
    64 x 64-tile kernel the classifier's weight gradient (9,360 rows -> a 5 x 128 result) was a 22 us kernel on the tail of
    the cfg-A step."""
    wide = (32, 64, 128, 256)
    al = lambda t: t.data_ptr() % 16 == 0
    if mode == GEMM_NT:
        return M >= SKINNY_ROWS and N <= 8 and K in wide and al(a)
    if mode == GEMM_NN:
        return M >= SKINNY_ROWS and K <= 8 and N in wide and al(b)
    return K >= SKINNY_ROWS and M <= 8 and N in wide and al(b)


def gemm(mode, a, b, bias=None, colsum=None):
    """fp32 product on the matrix cores (include/gda_hip.h: gda_gemm_ex_f32 / gda_gemm_tall_f32), no autograd.
    NT: ``a [M,K] @ b [N,K]^T`` (+ ``bias [N]`` in the epilogue); NN: ``a [M,K] @ b [K,N]``;
    TN: ``a [K,M]^T @ b [K,N]`` (``colsum [M]`` receives ``a.sum(0)``, the bias gradient beside the weight's)."""
    a, b = _f32c(a, "a"), _f32c(b, "b")
    if mode == GEMM_NT:
        (M, K), (N, K2) = a.shape, b.shape
    elif mode == GEMM_NN:
        (M, K), (K2, N) = a.shape, b.shape
    else:
        (K, M), (K2, N) = a.shape, b.shape
    if K != K2:
        raise ValueError(f"inner dimensions differ: {tuple(a.shape)} x {tuple(b.shape)} (mode {mode})")
    c = torch.empty(M, N, dtype=torch.float32, device=a.device)
    L = _lib.lib()
    tall = _tall_shape(mode, M, N, K, a, b)
    skinny = not tall and _skinny_shape(mode, M, N, K, a, b, N)
    need = (L.gda_gemm_tall_workspace_bytes if tall else L.gda_gemm_skinny_workspace_bytes if skinny
            else L.gda_gemm_workspace_bytes)(mode, M, N, K)
    ws = _lib.workspace(need, a.device, "gemm") if need else None
    name = ("dense_projection", "dense_projection_dgrad", "dense_projection_wgrad")[mode]
    with profiler.region(f"{name}[{K}x{N}]" if mode != GEMM_TN else f"{name}[{M}x{N}]", 1,
                         4 * (a.numel() + b.numel() + c.numel()), 2 * M * N * K):
        _lib.call("gda_gemm_tall_f32" if tall else "gda_gemm_skinny_f32" if skinny else "gda_gemm_ex_f32",
                  mode, M, N, K, a, a.size(1), b, b.size(1), c, N, bias, colsum,
                  ws, ws.numel() if ws is not None else 0, _lib.stream())
    return c


# --------------------------------------------------------------------------- SpMM --
aggregated_edges = 0     # running count of nnz(A_hat) over every aggregation launched (bench bookkeeping;
                         # only maintained while the profiler is on: it costs a cached-nnz lookup)
aggregation_log = None   # or a list: (graph or _Nnz, K) per aggregation call, nnz resolved later (no sync in the loop)


class _Nnz:
    """What the log keeps of a graph whose entry count is already known on the host (every batch of the device
    sampler): the number, not the graph -- a logged graph object pins its batch's CSR buffers for as long as the log
    lives, ~13 MB per sampled step that the caching allocator then has to hipMalloc afresh (1.7 device allocations per
    step inside bench.py's timed cfg-S region, one of them now and then 30 ms long)."""
    __slots__ = ("nnz", "tag")

    def __init__(self, nnz, tag=None):
        self.nnz, self.tag = nnz, tag


def _logged(graph):
    return (_Nnz(graph._nnz, getattr(graph, "tag", None))
            if getattr(graph, "_nnz", None) is not None and getattr(graph, "transient", False) else graph)

kstep_paths = None       # or a dict: which kernel ran the K >= 3 aggregation calls ("lds-one-launch" / "launch-chain"),
                         # counted per call while the profiler is on (bench.py: config.kstep_aggregation_path)


def _note_path(name, K):
    if kstep_paths is not None and profiler.enabled and K >= 3:
        kstep_paths[name] = kstep_paths.get(name, 0) + 1


INTERIOR_KSTEP = True     # tests/test_gpu_sampler.py turns these two off for its references
INTERIOR_HOIST = True


def _launch_kstep_interior(graph, x, K, bias, transposed, y):
    """K steps on a sampled batch whose rows ``[n_interior, n)`` hold their unit self loop only: the interior rows are
    recomputed per step, the leaves are finished in one pass (csrc/gda_spmm.hip, "sampled sub-graphs")."""
    rp, ci, va = (graph.t_rowptr, graph.t_colidx, graph.t_val) if transposed else (graph.rowptr, graph.colidx, graph.val)
    n, d = x.shape
    n_int = graph.n_interior
    plan = _interior_lds_plan(graph, x, y, K, transposed)
    if aggregation_log is not None:
        # (graph, K) = the K full aggregations the call stands for (SURVEY 8d's reference-equivalent count); third
        # element = the entries whose multiply-add this call really EXECUTES.  One-launch path: every entry of the batch
        # once (the leaf columns' contribution / the leaves' final pass, the leaf rows' unit self loops as one copy) + the
        # T off-diagonal and n_int diagonal entries of the interior block in each of the other K - 1 steps.  Launch
        # chain: its K steps walk every entry of the interior rows (skipped ones stay in the chain as w * 0).
        nnz_h, T = getattr(graph, "_nnz", None), getattr(graph, "iplan_T", None)
        executed = None
        if nnz_h is not None:
            executed = (nnz_h + (int(K) - 1) * (T + n_int) if (plan is not None and T is not None)
                        else int(K) * (nnz_h - (n - n_int)) + (n - n_int))
        aggregation_log.append((_logged(graph), int(K), executed, "interior-lds" if plan is not None else "interior-rows"))
    _note_path("interior-lds" if plan is not None else "interior-rows", int(K))
    if profiler.enabled:
        # `bytes`: what the call itself has to move -- forward K interior steps + one copy of the leaf rows; transposed K
        # interior steps + one pass over every entry for the leaves.  `alg_equiv_bytes`: SURVEY 8(d)'s algorithmic
        # bytes of the K full aggregations the call stands for.
        global aggregated_edges
        aggregated_edges += int(K) * graph.nnz
        nnz, n_leaf, row = graph.nnz, n - n_int, 4 * d
        # compulsory bytes: a step reads every distinct row its entries name at most once (<= n rows; the transposed
        # interior steps name interior rows only), the index arrays, and writes its own rows
        hoist = INTERIOR_HOIST and not transposed and K >= 2 and n_int > 0
        alg = K * (nnz * 8 + (n + 1) * 4 + 2 * n * d * 4)
        if plan is not None:
            # the one-launch path: the step loop never leaves LDS; HBM / L2 see the index arrays once, the leaf rows
            # once (forward: gathered for c; transposed: written), and the interior block crossing the column-major
            # staging (in: x_I and c or g_I; out: y_I, and the summed step inputs when transposed)
            real = nnz * 8 + (min(nnz, n) if not transposed else n_int) * row + 6 * n_int * row + 2 * n_leaf * row
            ctx = profiler.region(f"interior_lds_f32[d={d}]", 4 if transposed else 3, real, K * 2 * nnz * d,
                                  alg_equiv_bytes=alg, step_loop_launches=1)
        else:
            if transposed:
                real = K * (3 * n_int * row) + nnz * 8 + n_int * row + 2 * n_leaf * row
            elif hoist:   # one pass over the leaf columns, then K steps that gather interior rows and add the constant
                real = (nnz * 8 + min(nnz, n) * row + n_int * row) + K * (nnz * 8 + 3 * n_int * row + (n_int + 1) * 4) \
                    + 2 * n_leaf * row
            else:
                real = K * (nnz * 8 + min(nnz, n) * row + n_int * row + (n_int + 1) * 4) + 2 * n_leaf * row
            # launches: forward = K (+ 1 with the hoisted leaf term) of k_spmm_range + ONE k_rows_copy_bias; transposed =
            # K + 1 of k_spmm_range (`copy_launches` lets the bench price the call with rocprofv3's per-kernel averages)
            ctx = profiler.region(f"spmm_interior_f32[d={d}]", K + (2 if hoist else 1), real, K * 2 * nnz * d,
                                  alg_equiv_bytes=alg, copy_launches=0 if transposed else 1)
    else:
        ctx = profiler.region("", 0)
    if plan is not None:
        # ONE launch for the K steps (csrc/gda_interior.inc): 3 launches per call forward, 4 transposed, whatever K is
        # sized for the LARGEST interior block the kernel takes, not for this batch's: a scratch that grows with every
        # record-size batch is a hipMalloc (tens of milliseconds) in the middle of a training step
        ws, nbytes = _lib.scratch("gda_interior_kstep_lds_workspace_bytes", x.device, "interior_lds",
                                  _interior_lds_limits()[0], d)
        with ctx:
            _lib.call("gda_interior_kstep_lds_f32", rp, ci, va, n, n_int, d, int(K), int(bool(transposed)), plan, x, y,
                      bias, ws, nbytes, _lib.stream())
        return
    tmp = torch.empty(n_int, d, dtype=torch.float32, device=x.device) if K > 1 and n_int else None
    # transposed: the running sum of the step inputs; forward (K >= 2): the leaf columns' contribution, formed once
    want_sacc = transposed or (INTERIOR_HOIST and K >= 2)
    sacc = torch.empty(n_int, d, dtype=torch.float32, device=x.device) if want_sacc and n_int else None
    with ctx:
        _lib.call("gda_spmm_csr_interior_kstep_f32", rp, ci, va, n, n_int, d, int(K), int(bool(transposed)), x, y, tmp,
                  sacc, bias, _lib.stream())


INTERIOR_LDS_MIN_K = 3


def _interior_lds_plan(graph, x, y, K, transposed):
    """The device plan of this direction when the K interior steps of a sampled batch run as one launch
    (csrc/gda_interior.inc), else None: the device sampler built a valid plan for the direction,
    the width is one the kernel takes (a multiple of 4, one workgroup per column up to 128), K is worth it."""
    plans = getattr(graph, "iplan", None)
    if plans is None or K < INTERIOR_LDS_MIN_K or not INTERIOR_HOIST:      # hoist off = the chain's bit-exact row sums asked for
        return None
    plan = plans[1 if transposed else 0]
    n_int, d = graph.n_interior, x.size(1)
    if plan is None or not n_int or d % 4 or d > _interior_lds_limits()[1] or n_int > _interior_lds_limits()[0]:
        return None
    if x.data_ptr() % 16 or y.data_ptr() % 16:
        return None
    return plan


_il_limits = None


def _interior_lds_limits():
    global _il_limits
    if _il_limits is None:
        L = _lib.lib()
        _il_limits = (int(L.gda_interior_max_rows()), int(L.gda_interior_max_width()))
    return _il_limits


def _takes_interior_path(graph, x, bias, transposed):
    """The ONE predicate for "these K steps run on the interior-rows kernel" (it needs no ping-pong buffer):
    used by the launcher and by every caller that decides whether to allocate one."""
    return bool(INTERIOR_KSTEP and graph.n_interior is not None
                and 2 * graph.n_interior <= x.size(0) and x.is_contiguous() and (bias is None or not transposed))


def _launch_kstep(graph, x, K, bias, transposed, y, tmp):
    if _takes_interior_path(graph, x, bias, transposed):
        return _launch_kstep_interior(graph, x, K, bias, transposed, y)
    if tmp is None and K > 1:          # a caller that expected the interior path (which needs no ping-pong buffer)
        tmp = torch.empty_like(x)
    rp, ci, va = (graph.t_rowptr, graph.t_colidx, graph.t_val) if transposed else \
                 (graph.rowptr, graph.colidx, graph.val)
    n, d = x.shape
    _note_path("launch-chain", int(K))
    if aggregation_log is not None:
        aggregation_log.append((_logged(graph), int(K)))
    if profiler.enabled:      # algorithmic bytes per launch: nnz*(4+4) + (N+1)*4 + 2*N*d*4
        global aggregated_edges
        aggregated_edges += int(K) * graph.nnz
        nbytes = K * (graph.nnz * 8 + (n + 1) * 4 + 2 * n * d * 4)
        ctx = profiler.region(f"spmm_csr_f32[d={d}]", K, nbytes, K * 2 * graph.nnz * d)
    else:
        ctx = profiler.region("", 0)
    sp = graph.split(transposed).struct(d)         # None unless the graph has hub rows (> SPLIT_THRESHOLD entries)
    with ctx:
        _lib.call("gda_spmm_csr_split_f32", rp, ci, va, n, d, int(K), x, d, y, d, tmp, bias,
                  ctypes.byref(sp) if sp is not None else None, _lib.stream())


def _launch_kstep_lds(graph, plan, slots, x, K, bias, transposed, y, x_colmajor=False, y_colmajor=False,
                      colsum=None):
    """All K steps in one launch on the LDS-resident kernel (csrc/gda_kstep.hip): same sums, bit for bit.
    Column-major operands are ``[d, round_up(n, 4)]`` tensors and skip the transposition on their side."""
    n = graph.num_nodes
    d = x.size(0) if x_colmajor else x.size(1)
    if aggregation_log is not None:
        aggregation_log.append((graph, int(K)))
    if profiler.enabled:
        global aggregated_edges
        aggregated_edges += int(K) * graph.nnz
        _note_path("lds-one-launch", int(K))
        # `bytes`: SURVEY 8(d)'s algorithmic bytes of the K aggregations the launch stands for; `hbm_bytes`: what the
        # kernel itself moves (the plan per workgroup + one read and one write of the activations); `lds_bytes`:
        # the words its step loops gather out of LDS (slot-program entries incl. padding x columns x K)
        ctx = profiler.region(f"kstep_lds_f32[d={d},K={int(K)}]", 1,
                              K * (graph.nnz * 8 + (n + 1) * 4 + 2 * n * d * 4), K * 2 * graph.nnz * d,
                              hbm_bytes=plan.numel() + 2 * n * d * 4,
                              lds_bytes=4 * 1024 * (slots & 0xff) * 4 * d * int(K))
    else:
        ctx = profiler.region("", 0)
    n_pad = (n + 3) // 4 * 4
    ws = _lib.workspace(2 * d * n_pad * 4, x.device, "kstep")
    if profiler.enabled:
        # the same three launches as separate C calls, so that the K-step kernel itself is bracketed by the
        # HIP events (roofline: algorithmic bytes of K aggregations / its own duration)
        wsf = ws.view(torch.float32)
        xT, yT = (x if x_colmajor else wsf[:d * n_pad]), (y if y_colmajor else wsf[d * n_pad:2 * d * n_pad])
        if not x_colmajor:
            with profiler.region(f"transpose[{n}x{d}]", 1, 8 * n * d, 0):
                _lib.call("gda_transpose_f32", x, d, xT, n_pad, n, d, _lib.stream())
        with ctx:
            _lib.call("gda_kstep_lds_colmajor_f32", plan, slots, n, d, int(K), xT, n_pad, yT, n_pad, bias, colsum,
                      _lib.stream())
        if not y_colmajor:
            with profiler.region(f"transpose[{n}x{d}]", 1, 8 * n * d, 0):
                _lib.call("gda_transpose_f32", yT, n_pad, y, d, d, n, _lib.stream())
        return
    _lib.call("gda_kstep_lds_f32", plan, slots, n, d, int(K), x, n_pad if x_colmajor else d, int(x_colmajor), y,
              n_pad if y_colmajor else d, int(y_colmajor), bias, colsum, ws, _lib.stream())


def spmm_kstep(graph: CSRGraph, x, K=1, bias=None, transposed=False):
    """``A_hat^K @ x (+ bias)`` without autograd (ping-pong buffers), K launches -- one launch on the LDS-resident kernel
    for the static graph of a full-batch loader at citation size.

    Built, measured, removed: K // 2 launches of a cached ``A_hat * A_hat`` for static graphs -- +4 % epochs/s at cfg-A
    at the price of the bit-exact edge-order sums and a lower per-launch roofline fraction (profiles/HISTORY.md)."""
    from .graph import KSTEP_LDS, KSTEP_LDS_MIN_K
    x = _f32c(x, "x")
    if x.dim() != 2 or x.size(0) != graph.num_nodes:
        raise ValueError(f"x must be [num_nodes={graph.num_nodes}, d], got {tuple(x.shape)}")
    y = torch.empty_like(x)
    b = None if bias is None else _f32c(bias, "bias")
    if KSTEP_LDS and K >= KSTEP_LDS_MIN_K and graph.static:
        hit = graph.kstep_plan(transposed)       # static full-batch graphs at citation size: one launch
        if hit is not None:
            _launch_kstep_lds(graph, hit[0], hit[1], x, K, b, transposed, y)
            return y
    interior = _takes_interior_path(graph, x, b, transposed)
    _launch_kstep(graph, x, K, b, transposed, y, torch.empty_like(x) if K > 1 and not interior else None)
    return y


class ColMajor:
    """A ``[n, d]`` activation held column-major as ``t [d, round_up(n, 4)]`` -- the layout the LDS-resident
    K-step kernel computes in.  Produced by :func:`propagate` (``colmajor_out=True``) for its one consumer:
    :func:`relu_dropout`, whose kernel transposes on the fly, or the next projection where that applies the activation
    itself (:func:`act_tall_linear_colmajor`, :func:`act_skinny_linear`); ``dense()`` gives the ordinary tensor."""
    __slots__ = ("t", "n")

    def __init__(self, t, n):
        self.t, self.n = t, n

    def detach(self):
        return ColMajor(self.t.detach(), self.n)

    @property
    def shape(self):
        return torch.Size((self.n, self.t.size(0)))

    def size(self, k=None):
        return self.shape if k is None else self.shape[k]

    def dense(self):
        return self.t[:, :self.n].t().contiguous()


def lds_kstep_plan(graph, K, transposed=False):
    """``(plan, slots)`` when ``K`` aggregation steps over ``graph`` run on the one-launch LDS kernel."""
    from .graph import KSTEP_LDS, KSTEP_LDS_MIN_K
    if not KSTEP_LDS or K < KSTEP_LDS_MIN_K or not graph.static:
        return None
    return graph.kstep_plan(transposed)


class _TallLinearT(torch.autograd.Function):
    """``h = x W^T`` handed over COLUMN-MAJOR (``hT [out, round_up(n, 4)]``) to the K-step kernel: the same
    matrix-core kernels as ``nn.linear._TallLinear`` with the operands swapped -- ``hT = W x^T`` is the NT
    product of the small matrix with the tall one --, and in the backward pass ``gx = gT^T W`` (TN) and
    ``gW = gT x`` (NN with the deterministic row-slab split) straight from the column-major gradient."""

    @staticmethod
    def forward(ctx, x, weight):
        x, weight = _f32c(x, "x"), _f32c(weight, "weight")
        n, k = x.shape
        out = weight.size(0)
        n_pad = (n + 3) // 4 * 4
        hT = torch.empty(out, n_pad, dtype=torch.float32, device=x.device)
        gemm_raw(GEMM_NT, out, n, k, weight, k, x, k, hT, n_pad, f"dense_projection[{k}x{out}]")
        ctx.save_for_backward(x, weight)
        return hT

    @staticmethod
    def backward(ctx, gT):
        x, weight = ctx.saved_tensors
        return _tall_linear_t_backward(x, weight, gT, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def _tall_linear_t_backward(x, weight, gT, want_x, want_w):
    """The two gradient products of ``hT = W x^T`` from the column-major gradient ``gT``: ``(gx, gW)``."""
    n, k = x.shape
    out = weight.size(0)
    gT = gT.contiguous()
    n_pad = gT.size(1)
    gx = gw = None
    if want_x:
        gx = torch.empty(n, k, dtype=torch.float32, device=x.device)
        gemm_raw(GEMM_TN, n, k, out, gT, n_pad, weight, k, gx, k, f"dense_projection_dgrad[{out}x{k}]")
    if want_w:
        gw = torch.empty(out, k, dtype=torch.float32, device=x.device)
        gemm_raw(GEMM_NN, out, k, n, gT, n_pad, x, k, gw, k, f"dense_projection_wgrad[{out}x{k}]")
    return gx, gw


def tall_linear_colmajor(x, weight):
    return ColMajor(_TallLinearT.apply(x, weight), x.size(0))


# The activation between two conv layers applied by the CONSUMING projection while it stages its operand
# (gda_gemm_act_cm_f32, gda_gemm_skinny_act_cm_f32) instead of by a launch of its own -- wherever the pre-activation is a
# ColMajor with one consumer (A2GNNBase.feat_bottleneck_from / feat_classifier).  Same values, bit for bit.
ACT_IN_CONSUMER = True     # tests/test_gpu_act_in_consumer.py turns it off for its reference


class _ActTallLinearT(torch.autograd.Function):
    """``relu_dropout(ColMajor)`` followed by :func:`tall_linear_colmajor` in ONE launch: the projection reads the
    column-major pre-activation ``xT [k, n_pad]`` and applies the select itself.  ``keep``: also store the row-major
    activation ``y`` -- what the backward pass needs: exactly :class:`_TallLinearT`'s on ``y``, then
    :class:`_ReluDropoutT`'s.  Without it (a pass that is not differentiated) nothing but ``hT`` is written."""

    @staticmethod
    def forward(ctx, xT, n, weight, p, keep):
        weight = _f32c(weight, "weight")
        k, n_pad = xT.shape
        out = weight.size(0)
        y = torch.empty(n, k, dtype=torch.float32, device=xT.device) if keep else None
        hT = torch.empty(out, n_pad, dtype=torch.float32, device=xT.device)
        with profiler.region(f"dense_projection[{k}x{out}]", 1, 4 * (k * n + out * k + out * n + (n * k if keep else 0)),
                             2 * out * n * k):
            _lib.call("gda_gemm_act_cm_f32", n, out, k, xT, n_pad, weight, k, y, hT, n_pad, float(p),
                      *dropout_state.generator(xT.device), _lib.stream())
        if keep:
            ctx.save_for_backward(y, weight)
        ctx.p, ctx.n_pad = float(p), n_pad
        return hT

    @staticmethod
    def backward(ctx, gT):
        y, weight = ctx.saved_tensors
        gxT, gw = act_tall_linear_t_backward(y, weight, gT, ctx.p, ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        return gxT, None, gw, None, None


# A hidden layer's data gradient and weight gradient as two block ranges of ONE launch on the target's column-major chain
# (gda_gemm_act_cm_bwd_f32): the weight gradient no longer sits on the backward chain between the data gradient and its
# consumer, and the activation's backward is the data-gradient tiles' epilogue.  Within the entry point's envelope (output
# widths up to 128) the same values, bit for bit; outside it the composition runs as before.
BWD_PAIR = True            # tests/test_gpu_bwd_pair.py turns it off for its reference


def act_tall_linear_bwd_ok(y, weight, gT):
    """The backward of :class:`_ActTallLinearT` runs as one launch: the envelope of gda_gemm_act_cm_bwd_f32 -- the
    forward's, and an output width of at most 128 (wider, the composition's data gradient is a sum of slab partials)."""
    return (BWD_PAIR and y.is_cuda and y.dtype == gT.dtype == weight.dtype == torch.float32
            and y.dim() == weight.dim() == gT.dim() == 2 and y.is_contiguous() and weight.is_contiguous()
            and gT.is_contiguous() and y.size(0) >= 1 and y.size(1) == weight.size(1) and gT.size(0) == weight.size(0)
            and gT.size(1) >= y.size(0) and weight.size(1) >= 4 and weight.size(1) % 4 == 0
            and 1 <= weight.size(0) <= 128 and weight.size(0) % 4 == 0
            and weight.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0)


def act_tall_linear_t_backward(y, weight, gT, p, want_x=True, want_w=True):
    """The backward of :class:`_ActTallLinearT` from the column-major gradient ``gT [out, n_pad]`` with the saved
    activation ``y [n, k]``: ``(gxT [k, n_pad], gW [out, k])``, either None when not wanted.  One launch (+ the slab
    sum) with the activation's backward in the data-gradient tiles' epilogue where :func:`act_tall_linear_bwd_ok`;
    elsewhere :class:`_TallLinearT`'s two products followed by :class:`_ReluDropoutT`'s backward."""
    gT = gT.contiguous()
    n, k = y.shape
    out, n_pad = weight.size(0), gT.size(1)
    if not ((want_x or want_w) and act_tall_linear_bwd_ok(y, weight, gT)):
        gy, gw = _tall_linear_t_backward(y, weight, gT, want_x, want_w)
        return (_relu_dropout_t_backward(y, gy, p, n_pad) if gy is not None else None), gw
    gxT = torch.empty(k, n_pad, dtype=torch.float32, device=y.device) if want_x else None
    gw = torch.empty(out, k, dtype=torch.float32, device=y.device) if want_w else None
    need = _lib.lib().gda_gemm_workspace_bytes(GEMM_NN, out, k, n) if want_w else 0
    ws = _lib.workspace(need, y.device, "gemm") if need else None
    # ONE region for the one launch, named after the products it runs (a --full roofline finds either name in it)
    name = "+".join(f"dense_projection_{kind}[{out}x{k}]" for kind, on in (("dgrad", want_x), ("wgrad", want_w)) if on)
    with profiler.region(name, 1, (4 * (out * n + out * k + 2 * n * k) if want_x else 0)
                         + (4 * (out * n + n * k + out * k) if want_w else 0), 2 * n * k * out * (want_x + want_w)):
        _lib.call("gda_gemm_act_cm_bwd_f32", n, out, k, gT, n_pad, weight, k, y, float(p), gxT, gw,
                  ws, ws.numel() if ws is not None else 0, _lib.stream())
    return gxT, gw


def act_tall_linear_ok(x, weight):
    """``tall_linear_colmajor(relu_dropout(x), weight)`` runs as one launch: the envelope of gda_gemm_act_cm_f32."""
    return (ACT_IN_CONSUMER and isinstance(x, ColMajor) and x.t.is_cuda and x.t.dtype == torch.float32
            and x.t.is_contiguous() and weight.dtype == torch.float32 and weight.dim() == 2 and weight.is_contiguous()
            and weight.size(1) == x.size(1) and x.n >= 1 and weight.size(1) % 4 == 0 and weight.size(1) >= 4
            and weight.size(0) % 4 == 0 and weight.data_ptr() % 16 == 0)


def act_tall_linear_colmajor(x, weight, p, training):
    """``tall_linear_colmajor(relu_dropout(x, p, training), weight)`` for a :class:`ColMajor` ``x``; the caller checks
    :func:`act_tall_linear_ok` first."""
    keep = torch.is_grad_enabled() and (x.t.requires_grad or weight.requires_grad)
    return ColMajor(_ActTallLinearT.apply(x.t, x.n, weight, float(p) if training else 0.0, keep), x.n)


def act_skinny_ok(x, weight):
    """The classifier projection of ``relu_dropout(x)`` runs as one launch (gda_gemm_skinny_act_cm_f32): a forward-only
    pass at the shapes whose composition takes the skinny kernel (:func:`_skinny_shape`, NT)."""
    return (ACT_IN_CONSUMER and isinstance(x, ColMajor) and x.t.is_cuda and x.t.dtype == torch.float32
            and x.t.is_contiguous() and not (torch.is_grad_enabled() and (x.t.requires_grad or weight.requires_grad))
            and weight.dtype == torch.float32 and weight.dim() == 2 and weight.is_contiguous()
            and weight.size(1) == x.size(1) and x.n >= SKINNY_ROWS and weight.size(0) <= 8
            and weight.size(1) in (32, 64, 128, 256))


def act_skinny_linear(x, weight, p, training):
    """``relu_dropout(x, p, training) @ weight^T`` ``[n, classes]`` for a :class:`ColMajor` ``x``, no autograd; the caller
    checks :func:`act_skinny_ok` first."""
    n, k = x.shape
    c = weight.size(0)
    out = torch.empty(n, c, dtype=torch.float32, device=x.t.device)
    with profiler.region(f"dense_projection[{k}x{c}]", 1, 4 * (k * n + c * k + n * c), 2 * n * c * k):
        _lib.call("gda_gemm_skinny_act_cm_f32", n, c, k, x.t, x.t.size(1), weight.detach(), k, out, c,
                  float(p) if training else 0.0, *dropout_state.generator(x.t.device), _lib.stream())
    return out


_colsum_hint = None      # (data_ptr, column sums, the tensor itself) left by a kernel that produced both


def colsum(x):
    """``x.sum(0)`` of a row-major ``[n, d]`` fp32 device matrix (bias gradients): deterministic two-stage sum --
    or the by-product of the kernel that just wrote ``x`` (the stacked activation's backward), when there is one."""
    global _colsum_hint
    hint, _colsum_hint = _colsum_hint, None
    if hint is not None and hint[0] == x.data_ptr() and hint[2].shape == x.shape and x.is_contiguous():
        return hint[1]
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and 0 < x.size(1) <= 1024 and x.stride(1) == 1):
        return x.sum(0)
    n, d = x.shape
    out = torch.empty(d, dtype=torch.float32, device=x.device)
    ws, nbytes = _lib.scratch("gda_colsum_workspace_bytes", x.device, "colsum", n, d)
    _lib.call("gda_colsum_f32", x, x.stride(0), n, d, out, ws, nbytes, _lib.stream())
    return out


class _PropagateT(torch.autograd.Function):
    """K-step aggregation with a COLUMN-MAJOR result (forward) and gradient (backward): the transposes on
    the activation side of the LDS kernel disappear into the fused activation kernels
    (``gda_relu_dropout_*_cm_f32``), and the bias gradient is the column sum the backward kernel takes of its
    input while loading it -- no reduction launch."""

    @staticmethod
    def forward(ctx, x, bias, graph, K, x_colmajor=False):
        """``x``: ``[n, d]`` row-major, or (``x_colmajor``) ``[d, round_up(n, 4)]`` column-major -- then the
        gradient goes back column-major as well and no transposition is left on either side."""
        x = _f32c(x, "x")
        n = graph.num_nodes
        d = x.size(0) if x_colmajor else x.size(1)
        plan, slots = graph.kstep_plan(False)
        n_pad = (n + 3) // 4 * 4
        yT = torch.empty(d, n_pad, dtype=torch.float32, device=x.device)
        b = None if bias is None else _f32c(bias, "bias")
        _launch_kstep_lds(graph, plan, slots, x, K, b, False, yT, x_colmajor=x_colmajor, y_colmajor=True)
        ctx.graph, ctx.K, ctx.has_bias, ctx.n, ctx.x_colmajor = graph, K, bias is not None, n, x_colmajor
        return yT

    @staticmethod
    def backward(ctx, gT):
        graph, n = ctx.graph, ctx.n
        gT = gT.contiguous()
        d, n_pad = gT.shape
        plan, slots = graph.kstep_plan(True)
        want_b = ctx.has_bias and ctx.needs_input_grad[1]
        gb = torch.empty(d, dtype=torch.float32, device=gT.device) if want_b else None
        if ctx.x_colmajor:
            gx = torch.empty(d, n_pad, dtype=torch.float32, device=gT.device)
            if n_pad != n:
                gx[:, n:].zero_()
        else:
            gx = torch.empty(n, d, dtype=torch.float32, device=gT.device)
        _launch_kstep_lds(graph, plan, slots, gT, ctx.K, None, True, gx, x_colmajor=True,
                          y_colmajor=ctx.x_colmajor, colsum=gb)
        return (gx if ctx.needs_input_grad[0] else None), gb, None, None, None


class _Propagate(torch.autograd.Function):
    """K-step neighbour aggregation.  Linear in x, so nothing but the graph is saved:
    backward is the same K-step kernel on the by-source CSR (A_hat^T)."""

    @staticmethod
    def forward(ctx, x, bias, graph, K):
        ctx.graph, ctx.K, ctx.has_bias = graph, K, bias is not None
        return spmm_kstep(graph, x, K, bias)

    @staticmethod
    def backward(ctx, gy):
        gx = spmm_kstep(ctx.graph, gy.contiguous(), ctx.K, None, transposed=True) \
            if ctx.needs_input_grad[0] else None
        gb = colsum(gy) if ctx.has_bias and ctx.needs_input_grad[1] else None
        return gx, gb, None, None


def propagate(x, graph: CSRGraph, K=1, bias=None, colmajor_out=False):
    """``out = A_hat^K x + bias`` with autograd (prop_gcn_conv.py:208-213).  ``colmajor_out``: hand the result
    to the fused activation as a :class:`ColMajor` when the LDS-resident kernel runs this call (static graph
    at citation size, K >= 3, width a multiple of 4) -- otherwise the ordinary tensor comes back."""
    if K < 1:
        raise ValueError("K must be >= 1")
    if isinstance(x, ColMajor):              # from tall_linear_colmajor(): eligibility was checked there
        return ColMajor(_PropagateT.apply(x.t, bias, graph, int(K), True), x.n)
    if colmajor_out and lds_colmajor_ok(x, graph, K):
        return ColMajor(_PropagateT.apply(x, bias, graph, int(K)), x.size(0))
    return _Propagate.apply(x, bias, graph, int(K))


def propagate_act_ok(x, graph, K, bias):
    """``relu_dropout(propagate(x, graph, K, bias))`` runs as the one-launch interior K-step with the activation in its
    epilogue (gda_interior_kstep_lds_act_f32): a sampled batch whose forward plan the device sampler built."""
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32
            and x.is_contiguous() and _takes_interior_path(graph, x, bias, False)
            and _interior_lds_plan(graph, x, x, int(K), False) is not None)


class _PropagateAct(torch.autograd.Function):
    """``act(A_hat^K x + bias)`` with ``act = dropout(relu(.))`` applied by the aggregation's own epilogue; with ``pair`` a
    second output carries an independent dropout draw of the same pre-activation (not differentiated: the trainer's
    loss-unused pass).  Backward: the activation's mask from the saved OUTPUT (y > 0 <=> x > 0 and kept), then the
    K-step kernel on the by-source CSR -- nothing but the output and the graph is saved."""

    @staticmethod
    def forward(ctx, x, bias, graph, K, p, pair):
        x = _f32c(x, "x")
        n, d = x.shape
        n_int = graph.n_interior
        y0 = torch.empty_like(x)
        y1 = torch.empty_like(x) if pair else None
        b = None if bias is None else _f32c(bias, "bias")
        plan = _interior_lds_plan(graph, x, y0, K, False)
        gen = dropout_state.generator(x.device, sites=2) if pair else (*dropout_state.generator(x.device), 0)
        if aggregation_log is not None:
            nnz_h, T = getattr(graph, "_nnz", None), getattr(graph, "iplan_T", None)
            executed = None
            if nnz_h is not None:
                executed = (nnz_h + (int(K) - 1) * (T + n_int) if T is not None
                            else int(K) * (nnz_h - (n - n_int)) + (n - n_int))
            aggregation_log.append((_logged(graph), int(K), executed, "interior-lds"))
        _note_path("interior-lds", int(K))
        if profiler.enabled:
            global aggregated_edges
            aggregated_edges += int(K) * graph.nnz
            nnz, n_leaf, row = graph.nnz, n - n_int, 4 * d
            alg = K * (nnz * 8 + (n + 1) * 4 + 2 * n * d * 4)
            real = nnz * 8 + min(nnz, n) * row + 6 * n_int * row + (2 + bool(pair)) * n_leaf * row
            region = profiler.region(f"interior_lds_f32[d={d}]", 3, real, K * 2 * nnz * d, alg_equiv_bytes=alg,
                                     step_loop_launches=1)
        else:
            region = profiler.region("", 0)
        ws, nbytes = _lib.scratch("gda_interior_kstep_lds_workspace_bytes", x.device, "interior_lds",
                                  _interior_lds_limits()[0], d)
        with region:
            _lib.call("gda_interior_kstep_lds_act_f32", graph.rowptr, graph.colidx, graph.val, n, n_int, d, int(K),
                      plan, x, y0, y1, b, float(p), *gen, ws, nbytes, _lib.stream())
        ctx.graph, ctx.K, ctx.has_bias, ctx.p = graph, K, bias is not None, float(p)
        ctx.save_for_backward(y0)
        ctx.sink = _offer_sink(y0, p, wanted=ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        if pair:
            ctx.mark_non_differentiable(y1)
            return y0, y1
        return y0

    @staticmethod
    def backward(ctx, g0, g1=None):
        (y0,) = ctx.saved_tensors
        if ctx.sink is not None and ctx.sink.mine(g0):       # masked by its producer already (GradSink)
            gpre = g0
        else:
            g0 = g0.contiguous()
            gpre = torch.empty_like(g0)
            _lib.call("gda_relu_dropout_bwd_f32", g0, y0, gpre, g0.numel(), ctx.p, _lib.stream())
        gx = spmm_kstep(ctx.graph, gpre, ctx.K, None, transposed=True) if ctx.needs_input_grad[0] else None
        gb = colsum(gpre) if ctx.has_bias and ctx.needs_input_grad[1] else None
        return gx, gb, None, None, None, None


def propagate_act(x, graph, K, bias, p, training, pair=False):
    """``relu_dropout(propagate(x, graph, K, bias), p, training)`` -- twice, with independent draws, when ``pair`` -- as ONE
    call when :func:`propagate_act_ok`; the caller checks that first."""
    return _PropagateAct.apply(x, bias, graph, int(K), float(p) if training else 0.0, bool(pair))


def lds_colmajor_ok(x, graph, K):
    """The K-step call on ``x [n, d]`` runs on the LDS kernel and may hand over a column-major result."""
    return (x.dim() == 2 and x.size(1) % 4 == 0 and x.is_cuda and x.dtype == torch.float32
            and lds_kstep_plan(graph, int(K), False) is not None and lds_kstep_plan(graph, int(K), True) is not None)


# ---------------------------------------------------------------------------- MMD --
# loss + unscaled row gradients in one pass over the pairs on the 16-bit matrix cores with split operands
# (csrc/gda_mmd_fused.inc); 0 = the two-pass fp32-MFMA kernels with the [times, m, m] weight matrix in between
MMD_ONE_PASS = _os.environ.get("PYGDA_AMD_MMD_ONE_PASS", "1") == "1"


# the chunked one-pass kernel (csrc/gda_mmd_chunked.inc: any width up to 1024): "auto" = the widths the register-resident
# kernel does not cover (d > 128 or not a multiple of 32: GRADE's 645), "always" = every width (experiments), "0" = never
MMD_CHUNKED = _os.environ.get("PYGDA_AMD_MMD_CHUNKED", "auto")


def mmd_chunked_plan(times, n, d, kernel_mul=2.0, kernel_num=5):
    """``(nseg, padded width)`` when the chunked one-pass MMD takes these shapes, else None."""
    if not MMD_ONE_PASS or MMD_CHUNKED == "0" or not (MMD_CHUNKED == "always" or d > 128 or d % 32):
        return None
    import ctypes
    out = (ctypes.c_int64 * 8)()
    if _lib.lib().gda_mmd_chunked_plan(int(times), int(n), int(d), float(kernel_mul), int(kernel_num), out, 8) != 0:
        return None
    return int(out[0]), int(out[1])


def mmd_one_pass_segments(times, n, d, kernel_mul=2.0, kernel_num=5):
    """Row segments of the one-pass MMD for these shapes; 0 when it does not cover them (or is switched off)."""
    if not MMD_ONE_PASS:
        return 0
    plan = mmd_chunked_plan(times, n, d, kernel_mul, kernel_num)
    if plan is not None:
        return plan[0]
    return int(_lib.lib().gda_mmd_fused_nseg(int(times), int(n), int(d), float(kernel_mul), int(kernel_num)))


_one_pass_checked = {}      # device index -> True (agrees with the two-pass kernels) | False (declined) | "running"


def mmd_one_pass_ok(dev):
    """First use of the one-pass MMD on a device: run it BESIDE the fp32-MFMA two-pass kernels on a small fixed problem
    (own generator: the global CPU stream that seeded runs depend on is not touched) and keep it only if loss and row
    gradients agree to 1e-4 -- the kernel is hand-scheduled gfx950 assembly (LDS-DMA, explicit waits) that only the GPU
    tests execute, so a library built against another driver / compiler is caught here, once, instead of training on a
    silently different loss.  ~10 launches, once per process and device; never inside a capture."""
    global MMD_ONE_PASS
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    state = _one_pass_checked.get(key)
    if state is not None:
        return state is not False
    if torch.cuda.is_current_stream_capturing():
        return True                                    # cannot compare inside a capture; checked at the next eager call
    _one_pass_checked[key] = "running"
    gen = torch.Generator().manual_seed(20240521)
    ok, why = True, ""
    try:
        for d in (128, 64, 200):                       # 200: the chunked kernel (two chunks of 128 | 96)
            times, n = 2, 80
            a = (torch.randn(times * n, d, generator=gen) * 0.7 + 0.3).to(dev).requires_grad_(True)
            b = (torch.randn(times * n, d, generator=gen) * 0.9 - 0.1).to(dev).requires_grad_(True)
            got = []
            for one in (True, False):
                MMD_ONE_PASS = one
                with torch.enable_grad():              # called from inside an autograd Function's forward
                    loss = _MMD.apply(a, b, None, None, times, n, 2.0, 5, None)
                    ga, gb = torch.autograd.grad(loss, (a, b))
                got.append((loss.detach().double(), torch.cat([ga, gb]).double()))
            MMD_ONE_PASS = True
            (l1, g1), (l2, g2) = got
            dl = float((l1 - l2).abs() / l2.abs().clamp_min(1e-30))
            dg = float((g1 - g2).norm() / g2.norm().clamp_min(1e-30))
            if not (dl <= 1e-4 and dg <= 1e-4):        # NaN fails too
                ok, why = False, f"d={d}: loss differs by {dl:.3g}, row gradients by {dg:.3g} (relative)"
                break
    except Exception as exc:                           # noqa: BLE001 -- a launch failure is a reason to decline too
        ok, why = False, f"{type(exc).__name__}: {exc}"
    finally:
        MMD_ONE_PASS = True
    _one_pass_checked[key] = ok
    if not ok:
        import warnings
        warnings.warn("one-pass MMD kernel declined by its first-use self-check (" + why +
                      "); this process uses the two-pass fp32-MFMA kernels")
    return ok


class _MMD(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, tgt, src_idx, tgt_idx, times, n, kernel_mul, kernel_num, fix_sigma, sel=None, scale=1.0,
                add=None, act_cm=None):
        """``(add +) scale * MMD``: the trainer's loss line ``loss = CE + MMD(...) * weight`` (a2gnn.py:207-209)
        without elementwise glue kernels around the loss kernels.  ``act_cm = (rows, p, seed, step, site)``: ``tgt`` is a
        column-major pre-activation (:class:`PreActCM`; the caller checked :func:`mmd_act_cm_ok`)."""
        ctx.sel, ctx.scale, ctx.has_add = sel, float(scale), add is not None
        ctx.act_cm = act_cm
        if act_cm is not None:
            return _mmd_forward_act_cm(ctx, src, tgt, src_idx, tgt_idx, times, n, kernel_mul, kernel_num, scale, add)
        ctx.sinks = (sink_of(src), sink_of(tgt))
        src, tgt = _f32c(src, "source_feat"), _f32c(tgt, "target_feat")
        d = src.size(1)
        if tgt.size(1) != d:
            raise ValueError("source and target features must have the same width")
        dev = src.device
        m = 2 * n
        ctx.feat_rows = (src.size(0), tgt.size(0))
        idx_s = idx_t = rows_s = rows_t = None
        plan = mmd_chunked_plan(times, n, d, kernel_mul, kernel_num) if not fix_sigma else None
        if plan is not None and not mmd_one_pass_ok(dev):
            plan = None
        if src_idx is not None:
            idx_s, idx_t = src_idx.contiguous(), tgt_idx.contiguous()
            if plan is None:
                # the sampled rows gathered ONCE into [times*n, d] (2 x 2.5 MB at the A2GNN shapes) -- by the
                # statistics kernel, which reads them through the index anyway; everything after reads the copy
                rows_s = torch.empty(times * n, d, dtype=torch.float32, device=dev)
                rows_t = torch.empty(times * n, d, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        bw = torch.empty(times, dtype=torch.float32, device=dev)
        addc = None if add is None else add.detach().to(torch.float32).reshape(1).contiguous()
        nseg = 0
        if plan is not None:
            nseg, dp = plan
            rows_s = torch.empty(times * n, dp, dtype=torch.float32, device=dev)     # gathered / copied, zero padded
            rows_t = torch.empty(times * n, dp, dtype=torch.float32, device=dev)
            part = torch.empty(times, nseg, m, dp, dtype=torch.float32, device=dev)
            ws, _ = _lib.scratch("gda_mmd_chunked_workspace_bytes", dev, "mmd_chunked", times, n, d)
            with profiler.region("mmd_fwd", 5, 0, times * 3 * 4 * m * m * dp):
                _lib.call("gda_mmd_chunked_fwd_f32", src, d, tgt, d, d, idx_s, idx_t, times, n, float(kernel_mul),
                          int(kernel_num), 0.0, float(scale), addc, rows_s, rows_t, dp, loss, bw, part, dp, nseg, ws,
                          ws.numel(), _lib.stream())
            ctx.one_pass, ctx.ldp = nseg, dp
            ctx.save_for_backward(src_idx, tgt_idx, part)
            ctx.cfg = (times, n, d, float(kernel_mul), int(kernel_num))
            return loss.reshape(())
        ws, _ = _lib.scratch("gda_mmd_workspace_bytes", dev, "mmd", times, n, d)
        if not fix_sigma:
            nseg = mmd_one_pass_segments(times, n, d, kernel_mul, kernel_num)
            aligned = src.data_ptr() % 16 == 0 and tgt.data_ptr() % 16 == 0
            nseg = nseg if aligned and (not nseg or mmd_one_pass_ok(dev)) else 0
        ctx.one_pass, ctx.ldp = nseg, d
        if nseg:
            part = torch.empty(times, nseg, m, d, dtype=torch.float32, device=dev)
            with profiler.region("mmd_fwd", 4, 0, times * 3 * 4 * m * m * d):
                _lib.call("gda_mmd_fused_fwd_f32", src, d, tgt, d, d, idx_s, idx_t, times, n, float(kernel_mul),
                          int(kernel_num), float(fix_sigma) if fix_sigma else 0.0, float(scale), addc, rows_s, rows_t,
                          loss, bw, part, nseg, ws, ws.numel(), _lib.stream())
            ctx.save_for_backward(src_idx, tgt_idx, part)
            ctx.cfg = (times, n, d, float(kernel_mul), int(kernel_num))
            return loss.reshape(())
        l2 = torch.empty(times, m, m, dtype=torch.float32, device=dev)
        with profiler.region("mmd_fwd", 4, 0, times * (3 * m * m * d // 2 + 12 * m * m)):
            _lib.call("gda_mmd_fwd_gather_f32", src, d, tgt, d, d, idx_s, idx_t, times, n, float(kernel_mul),
                      int(kernel_num), float(fix_sigma) if fix_sigma else 0.0, float(scale), addc, rows_s, rows_t, loss,
                      bw, l2, ws, ws.numel(), _lib.stream())
        if rows_s is not None:
            src, tgt = rows_s, rows_t
        ctx.save_for_backward(src, tgt, src_idx, tgt_idx, bw, l2)
        ctx.cfg = (times, n, float(kernel_mul), int(kernel_num))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        if ctx.act_cm is not None:
            return _mmd_backward_act_cm(ctx, gl)
        if ctx.one_pass:
            return _MMD._backward_one_pass(ctx, gl)
        src, tgt, src_idx, tgt_idx, bw, l2 = ctx.saved_tensors
        times, n, kernel_mul, kernel_num = ctx.cfg
        d, dev, m = src.size(1), src.device, 2 * n
        glc = gl.reshape(1).to(torch.float32).contiguous()
        ws, _ = _lib.scratch("gda_mmd_workspace_bytes", dev, "mmd", times, n, d)
        g_add = gl if ctx.has_add else None
        tail = (None,) * 9 + (g_add,)
        if src_idx is not None and ctx.sel is not None:
            # row gradients summed straight onto the sampled feature rows (segment reduce + scatter in one kernel)
            s_rp, s_ci, t_rp, t_ci, _ones = ctx.sel
            gs = torch.empty(ctx.feat_rows[0], d, dtype=torch.float32, device=dev)
            gt = torch.empty(ctx.feat_rows[1], d, dtype=torch.float32, device=dev)
            with profiler.region("mmd_bwd", 2, 0, times * (3 * m * m * d + 12 * m * m)):
                _lib.call("gda_mmd_bwd_ex_f32", src, d, tgt, d, d, None, None, times, n, kernel_mul, kernel_num, bw,
                          l2, glc, ctx.scale, None, s_rp, s_ci, ctx.feat_rows[0], gs, t_rp, t_ci, ctx.feat_rows[1], gt,
                          ws, ws.numel(), _lib.stream())
            return (gs if ctx.needs_input_grad[0] else None, gt if ctx.needs_input_grad[1] else None) + tail
        grad_rows = torch.empty(times, m, d, dtype=torch.float32, device=dev)
        with profiler.region("mmd_bwd", 2, 0, times * (3 * m * m * d + 12 * m * m)):
            _lib.call("gda_mmd_bwd_ex_f32", src, d, tgt, d, d, None, None, times, n, kernel_mul, kernel_num, bw, l2,
                      glc, ctx.scale, grad_rows, None, None, 0, None, None, None, 0, None, ws, ws.numel(),
                      _lib.stream())
        if src_idx is None:                       # rows as given, stacked [times, n, d]
            gs, gt = grad_rows[:, :n].reshape(times * n, d), grad_rows[:, n:].reshape(times * n, d)
        else:
            gs = _scatter_rows(grad_rows, src_idx, 0, n, ctx.feat_rows[0])
            gt = _scatter_rows(grad_rows, tgt_idx, n, n, ctx.feat_rows[1])
        return (gs if ctx.needs_input_grad[0] else None, gt if ctx.needs_input_grad[1] else None) + tail


def _mmd_backward_one_pass(ctx, gl):
    """Backward of the one-pass MMD: the forward left unscaled row-gradient partials; this folds the segments, applies
    4 * dloss * scale / (n^2 times) and scatters onto the feature rows (one launch with the selection CSRs)."""
    src_idx, tgt_idx, part = ctx.saved_tensors
    times, n, d, _, _ = ctx.cfg
    dev, m = part.device, 2 * n
    glc = gl.reshape(1).to(torch.float32).contiguous()
    g_add = gl if ctx.has_add else None
    tail = (None,) * 9 + (g_add,)
    if src_idx is not None and ctx.sel is not None:
        s_rp, s_ci, t_rp, t_ci, _ones = ctx.sel
        # a feature matrix that came straight out of dropout(relu(.)) may have handed over a GradSink: its row gradients
        # are then stored already through that activation's backward (mask in the scatter's epilogue)
        ok = lambda k, rows: (k is not None and k.buf.shape == (rows, d) and k.buf.data_ptr() % 16 == 0
                              and k.y.data_ptr() % 16 == 0)
        ks = ctx.sinks[0] if ok(ctx.sinks[0], ctx.feat_rows[0]) and ctx.needs_input_grad[0] else None
        kt = ctx.sinks[1] if ok(ctx.sinks[1], ctx.feat_rows[1]) and ctx.needs_input_grad[1] else None
        gs = ks.buf if ks is not None else torch.empty(ctx.feat_rows[0], d, dtype=torch.float32, device=dev)
        gt = kt.buf if kt is not None else torch.empty(ctx.feat_rows[1], d, dtype=torch.float32, device=dev)
        with profiler.region("mmd_bwd", 1, 0, 0):
            _lib.call("gda_mmd_fused_bwd_ld_f32", part, ctx.ldp, ctx.one_pass, times, n, d, glc, ctx.scale, None, s_rp,
                      s_ci, ctx.feat_rows[0], gs, t_rp, t_ci, ctx.feat_rows[1], gt, ks.y if ks is not None else None,
                      ks.p if ks is not None else 0.0, kt.y if kt is not None else None,
                      kt.p if kt is not None else 0.0, _lib.stream())
        for k in (ks, kt):
            if k is not None:
                k.written = True
        return (gs if ctx.needs_input_grad[0] else None, gt if ctx.needs_input_grad[1] else None) + tail
    grad_rows = torch.empty(times, m, d, dtype=torch.float32, device=dev)
    with profiler.region("mmd_bwd", 1, 0, 0):
        _lib.call("gda_mmd_fused_bwd_ld_f32", part, ctx.ldp, ctx.one_pass, times, n, d, glc, ctx.scale, grad_rows, None,
                  None, 0, None, None, None, 0, None, None, 0.0, None, 0.0, _lib.stream())
    if src_idx is None:                       # rows as given, stacked [times, n, d]
        gs, gt = grad_rows[:, :n].reshape(times * n, d), grad_rows[:, n:].reshape(times * n, d)
    else:
        gs = _scatter_rows(grad_rows, src_idx, 0, n, ctx.feat_rows[0])
        gt = _scatter_rows(grad_rows, tgt_idx, n, n, ctx.feat_rows[1])
    return (gs if ctx.needs_input_grad[0] else None, gt if ctx.needs_input_grad[1] else None) + tail


_MMD._backward_one_pass = staticmethod(_mmd_backward_one_pass)


# The full-batch A2GNN step's target features reach the MMD as the K-step kernel's column-major PRE-activation: the one-pass
# kernels apply dropout(relu(.)) while they gather the sampled rows (gda_mmd_fused_fwd_act_cm_f32) and write the gradient of
# the pre-activation, column-major, from their scatter (gda_mmd_fused_bwd_act_cm_f32) -- the activation's two launches and
# the row-major [nt, d] matrix between them are gone.  Same values, bit for bit; outside the envelope the composition runs.
MMD_ACT_CM = True          # tests/test_gpu_mmd_act_cm.py turns it off for its reference


class PreActCM:
    """Target features NOT yet activated: the :class:`ColMajor` pre-activation, the dropout probability and the generator
    triple ``(seed, step counter, site)`` drawn where the activation would have been issued (so every other mask of the
    step keeps its site).  :func:`mmd_loss` hands it to the one-pass kernels or, outside their envelope, composes."""
    __slots__ = ("pre", "p", "gen")

    def __init__(self, pre, p, gen):
        self.pre, self.p, self.gen = pre, float(p), tuple(gen)

    shape = property(lambda self: self.pre.shape)
    device = property(lambda self: self.pre.t.device)
    is_cuda = property(lambda self: self.pre.t.is_cuda)
    dtype = property(lambda self: self.pre.t.dtype)

    def size(self, k=None):
        return self.pre.size(k)

    def compose(self):
        """The activation as its own launch, with the triple drawn already: the ordinary row-major features."""
        return _ReluDropoutT.apply(self.pre.t, self.pre.n, self.p, self.gen)


def mmd_act_cm_ok(times, n, d, sel, ptrs=(), lds=(), fix_sigma=None, kernel_mul=2.0, kernel_num=5):
    """The envelope of gda_mmd_fused_{fwd,bwd}_act_cm_f32: the one-pass register kernel's widths and segment counts, the
    selection CSRs of the gradient scatter, 16-byte aligned operands (``ptrs``: their addresses, ``lds``: their leading
    dimensions in floats), a data-dependent bandwidth.  Host arithmetic only."""
    if not MMD_ACT_CM or fix_sigma or sel is None or len(sel) < 4 or any(s is None for s in sel[:4]):
        return False
    if d not in (32, 64, 96, 128) or any(int(a) % 16 for a in ptrs) or any(int(l) % 4 for l in lds):
        return False
    if mmd_chunked_plan(times, n, d, kernel_mul, kernel_num) is not None:
        return False
    return 1 <= mmd_one_pass_segments(times, n, d, kernel_mul, kernel_num) <= 8


def _mmd_forward_act_cm(ctx, src, xT, src_idx, tgt_idx, times, n, kernel_mul, kernel_num, scale, add):
    rows_t_total, p, seed, step, site = ctx.act_cm
    ctx.sinks = (sink_of(src), None)
    src = _f32c(src, "source_feat")
    d, dev, m = src.size(1), src.device, 2 * n
    ctx.feat_rows = (src.size(0), int(rows_t_total))
    idx_s, idx_t = src_idx.contiguous(), tgt_idx.contiguous()
    nseg = mmd_one_pass_segments(times, n, d, kernel_mul, kernel_num)
    rows_s = torch.empty(times * n, d, dtype=torch.float32, device=dev)
    rows_t = torch.empty(times * n, d, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    bw = torch.empty(times, dtype=torch.float32, device=dev)
    addc = None if add is None else add.detach().to(torch.float32).reshape(1).contiguous()
    part = torch.empty(times, nseg, m, d, dtype=torch.float32, device=dev)
    ws, _ = _lib.scratch("gda_mmd_workspace_bytes", dev, "mmd", times, n, d)
    with profiler.region("mmd_fwd", 4, 0, times * 3 * 4 * m * m * d):
        _lib.call("gda_mmd_fused_fwd_act_cm_f32", src, d, xT, xT.size(1), int(rows_t_total), d, idx_s, idx_t, times, n,
                  float(kernel_mul), int(kernel_num), 0.0, float(scale), addc, rows_s, rows_t, loss, bw, part, nseg,
                  float(p), seed, step, site, ws, ws.numel(), _lib.stream())
    ctx.one_pass, ctx.ldp = nseg, d
    ctx.save_for_backward(part, xT)
    ctx.cfg = (times, n, d, float(kernel_mul), int(kernel_num))
    return loss.reshape(())


def _mmd_backward_act_cm(ctx, gl):
    """One scatter launch: the source's row gradients as ever, the target's as the column-major gradient of ``xT``."""
    part, xT = ctx.saved_tensors
    times, n, d, _, _ = ctx.cfg
    _, p, seed, step, site = ctx.act_cm
    dev = part.device
    glc = gl.reshape(1).to(torch.float32).contiguous()
    s_rp, s_ci, t_rp, t_ci = ctx.sel[:4]
    ks = ctx.sinks[0]
    if not (ks is not None and ctx.needs_input_grad[0] and ks.buf.shape == (ctx.feat_rows[0], d)
            and ks.buf.data_ptr() % 16 == 0 and ks.y.data_ptr() % 16 == 0):
        ks = None
    gs = ks.buf if ks is not None else torch.empty(ctx.feat_rows[0], d, dtype=torch.float32, device=dev)
    gxT = torch.empty_like(xT)
    with profiler.region("mmd_bwd", 1, 0, 0):
        _lib.call("gda_mmd_fused_bwd_act_cm_f32", part, ctx.one_pass, times, n, d, glc, ctx.scale, s_rp, s_ci,
                  ctx.feat_rows[0], gs, t_rp, t_ci, ctx.feat_rows[1], xT, gxT, xT.size(1), float(p), seed, step, site,
                  ks.y if ks is not None else None, ks.p if ks is not None else 0.0, _lib.stream())
    if ks is not None:
        ks.written = True
    return (gs if ctx.needs_input_grad[0] else None, gxT if ctx.needs_input_grad[1] else None) + (None,) * 9 + \
        (gl if ctx.has_add else None, None)


class _PinnedRing:
    """A few pinned host blocks handed out in turn, each guarded by the event of the copy that last left it: what a
    step ships to the device (MMD row samples + their selection CSRs, ~1.4 MB at cfg-S) goes as ONE asynchronous
    copy.  ``tensor.to(device)`` from pageable memory is synchronous -- the host waits for the stream to drain
    first -- which serialised the eager sampled-training loop against the GPU (six such copies per step: 1.2 ms)."""

    def __init__(self, slots=4):
        self.slots, self.turn = [None] * slots, 0

    def take(self, nbytes):
        i = self.turn
        self.turn = (i + 1) % len(self.slots)
        hit = self.slots[i]
        if hit is not None and hit[1] is not None:
            hit[1].synchronize()                       # the copy out of this block (several steps ago) has finished
        if hit is None or hit[0].numel() < nbytes:
            cap = 1 << 16
            while cap < nbytes + nbytes // 2:          # headroom: batches differ in size, pinning is expensive (~50 ms)
                cap <<= 1
            hit = [torch.empty(cap, dtype=torch.uint8).pin_memory(), None]
            self.slots[i] = hit
        return i, hit[0]

    def sent(self, i, stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        self.slots[i][1] = ev


_pinned_ring = _PinnedRing()


def mmd_samples_to_device(source_sample, target_sample, ns, nt, dev, stacked=True):
    """The two ``[times, n]`` CPU row-sample tensors of an MMD call and the selection CSRs of their gradient scatter
    -> ``(idx_s, idx_t, sel)`` on the device through one pinned block and one non-blocking copy.  ``stacked``: the
    gradient buffer holds source and target rows side by side (``[times, 2n, d]``, the single-process loss);
    otherwise each domain scatters out of its own ``[times, n, d]`` buffer (the data-parallel row exchange)."""
    times, n = source_sample.shape
    m = 2 * n if stacked else n
    a16 = lambda v: (v + 15) // 16 * 16
    sizes = [8 * times * n, 8 * times * n, 4 * (ns + 1), 4 * times * n, 4 * (nt + 1), 4 * times * n]
    offs = [0]
    for sz in sizes:
        offs.append(offs[-1] + a16(sz))
    slot, host = _pinned_ring.take(offs[-1])
    view = lambda k, dt, cnt: host[offs[k]:offs[k] + sizes[k]].view(dt)[:cnt]
    view(0, torch.int64, times * n).copy_(source_sample.reshape(-1))
    view(1, torch.int64, times * n).copy_(target_sample.reshape(-1))
    selection_csr_host(source_sample, ns, 0, m, out=(view(2, torch.int32, ns + 1), view(3, torch.int32, times * n)))
    selection_csr_host(target_sample, nt, n if stacked else 0, m,
                       out=(view(4, torch.int32, nt + 1), view(5, torch.int32, times * n)))
    block = torch.empty(offs[-1], dtype=torch.uint8, device=dev)
    from .hipgraph import _ship
    _ship(block, host[:offs[-1]])              # a kernel of this stream that reads the pinned block (no DMA-engine hand-over)
    _pinned_ring.sent(slot, torch.cuda.current_stream())
    dview = lambda k, dt, cnt: block[offs[k]:offs[k] + sizes[k]].view(dt)[:cnt]
    sel = (dview(2, torch.int32, ns + 1), dview(3, torch.int32, times * n),
           dview(4, torch.int32, nt + 1), dview(5, torch.int32, times * n),
           torch.ones(times * n, dtype=torch.float32, device=dev))
    return dview(0, torch.int64, times * n).view(times, n), dview(1, torch.int64, times * n).view(times, n), sel


def selection_csr_host(idx, num_feat_rows, offset, m, out=None):
    """Host side of the sample-gradient scatter (native counting sort, csrc/gda_sampler.cpp):
    for ``idx [times, n]`` (CPU int64 row samples) the CSR of the 0/1 selection matrix -- rows =
    feature rows, columns = positions ``t*m + offset + r`` of the ``[times, m, d]`` gradient
    buffer.  ``out = (rowptr, colidx)`` may name preallocated (pinned) CPU int32 tensors."""
    idx = idx.contiguous()
    times, n = idx.shape
    if out is None:
        out = (torch.empty(num_feat_rows + 1, dtype=torch.int32), torch.empty(times * n, dtype=torch.int32))
    _lib.call("gda_selection_csr_host", idx.data_ptr(), int(times), int(n), int(num_feat_rows), int(offset), int(m),
              out[0].data_ptr(), out[1].data_ptr())
    return out


def _selection_spmm(rowptr, colidx, ones, flat, num_feat_rows):
    d = flat.size(1)
    out = torch.empty(num_feat_rows, d, dtype=torch.float32, device=flat.device)
    _lib.call("gda_spmm_csr_f32", rowptr, colidx, ones, num_feat_rows, d, flat, d, out, d, None, _lib.stream())
    return out


def _scatter_rows(grad_rows, idx, offset, n, num_feat_rows):
    """Sum the per-sample row gradients back onto the sampled feature rows (duplicates
    included) deterministically: a CSR SpMM with the 0/1 selection matrix, built on device
    by the same ingestion kernel (no self loops, no normalisation)."""
    times, m, d = grad_rows.shape
    dev = grad_rows.device
    pos = (torch.arange(times, device=dev).view(-1, 1) * m + offset +
           torch.arange(n, device=dev).view(1, -1)).reshape(-1)
    n_nodes = max(num_feat_rows, times * m)
    g = build_csr(torch.stack([pos, idx.reshape(-1)]), n_nodes, None, add_self_loops=False,
                  normalize=False, validate=False)
    flat = grad_rows.view(times * m, d)
    if n_nodes > times * m:                       # SpMM gathers rows < n_nodes only via colidx: fine
        pass
    out = torch.empty(num_feat_rows, d, dtype=torch.float32, device=dev)
    _lib.call("gda_spmm_csr_f32", g.rowptr, g.colidx, g.val, num_feat_rows, d, flat, d, out, d, None, _lib.stream())
    return out


class _SampleRows(torch.autograd.Function):
    """``feat[idx]`` for ``idx [times, n]`` -> ``[times, n, d]``: gather kernel forward,
    deterministic selection-matrix SpMM backward (duplicates summed in a fixed order)."""

    @staticmethod
    def forward(ctx, feat, idx, sel=None):
        ctx.save_for_backward(idx)
        ctx.rows, ctx.sel = feat.size(0), sel
        return gather_rows(feat, idx.reshape(-1)).view(idx.size(0), idx.size(1), feat.size(1))

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        times, n, d = g.shape
        g = g.contiguous()
        if ctx.sel is not None:               # selection CSR prepared on the host with the draws
            rowptr, colidx, ones = ctx.sel
            return _selection_spmm(rowptr, colidx, ones, g.view(times * n, d), ctx.rows), None, None
        return _scatter_rows(g.view(times, n, d), idx, 0, n, ctx.rows), None, None


def sample_rows(feat, idx, sel=None):
    """``sel = (rowptr, colidx, ones)``: device CSR of the 0/1 selection matrix of ``idx`` (columns
    ``t * n + r``; :func:`selection_csr_host` with ``offset=0, m=n``) -- without it the backward
    pass builds that CSR on the device (a sort per call)."""
    return _SampleRows.apply(_f32c(feat, "feat"), idx, sel)


def mmd_loss_rows(source_rows, target_rows, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """MMD over explicit row sets ``[times, n, d]`` per domain (the data-parallel path, where
    the rows are an all-gather of every rank's samples)."""
    if source_rows.shape != target_rows.shape or source_rows.dim() != 3:
        raise RuntimeError("row sets must both be [times, n, d]")
    times, n, d = source_rows.shape
    return _MMD.apply(source_rows.reshape(times * n, d), target_rows.reshape(times * n, d), None, None,
                      int(times), int(n), kernel_mul, kernel_num, fix_sigma)


def mmd_loss(source_feat, target_feat, src_idx=None, tgt_idx=None, kernel_mul=2.0, kernel_num=5,
             fix_sigma=None, sel=None, scale=1.0, add=None):
    """Sampled multi-kernel MMD (mmd.py:57-159).  ``src_idx/tgt_idx``: ``[times, n]`` int64
    device tensors of row samples, or both ``None`` for get_MMD on the rows as given."""
    if (src_idx is None) != (tgt_idx is None):
        raise ValueError("give both index tensors or neither")
    if src_idx is None:
        if source_feat.size(0) != target_feat.size(0):
            # the reference's XX + YY - XY - YX broadcast fails the same way (mmd.py:100-106)
            raise RuntimeError("get_MMD needs equally many source and target rows, got "
                               f"{source_feat.size(0)} and {target_feat.size(0)}")
        times, n = 1, source_feat.size(0)
    else:
        _lib.require_gpu_tensor(src_idx, "src_idx", torch.int64)
        _lib.require_gpu_tensor(tgt_idx, "tgt_idx", torch.int64)
        if src_idx.shape != tgt_idx.shape or src_idx.dim() != 2:
            raise RuntimeError("source and target samples must both be [times, sampling_num]")
        times, n = src_idx.shape
        src_idx, tgt_idx = src_idx.contiguous(), tgt_idx.contiguous()
    if isinstance(target_feat, PreActCM):
        pre, xT = target_feat, target_feat.pre.t
        if src_idx is not None and source_feat.is_cuda and xT.dtype == torch.float32 and xT.is_contiguous():
            source_feat = _f32c(source_feat, "source_feat")
            if (xT.size(0) == source_feat.size(1)
                    and mmd_act_cm_ok(times, n, source_feat.size(1), sel, (source_feat.data_ptr(), xT.data_ptr()),
                                      (xT.size(1),), fix_sigma, kernel_mul, kernel_num)
                    and mmd_one_pass_ok(source_feat.device)):
                return _MMD.apply(source_feat, xT, src_idx, tgt_idx, int(times), int(n), kernel_mul, kernel_num,
                                  fix_sigma, sel, scale, add, (pre.pre.n, pre.p, *pre.gen))
        target_feat = pre.compose()
    return _MMD.apply(source_feat, target_feat, src_idx, tgt_idx, int(times), int(n), kernel_mul,
                      kernel_num, fix_sigma, sel, scale, add)


# ------------------------------------------------- GRL + discriminator + CE (fused) --
class _GrlDiscCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fs, ft, W, b, alpha, labels):
        fs, ft, W, b = _f32c(fs, "source_feat"), _f32c(ft, "target_feat"), _f32c(W, "weight"), _f32c(b, "bias")
        ns, nt, h, C = fs.size(0), ft.size(0), fs.size(1), W.size(0)
        dev = fs.device
        probs = torch.empty(ns + nt, C, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws, _ = _lib.scratch("gda_grl_disc_workspace_bytes", dev, "disc", ns + nt, h, C)
        _lib.call("gda_grl_disc_ce_fwd_f32", fs, h, ns, ft, h, nt, h, C, W, b, labels, probs, loss, ws, ws.numel(),
                  _lib.stream())
        ctx.save_for_backward(fs, ft, W, probs, labels)
        ctx.alpha = float(alpha)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        fs, ft, W, probs, labels = ctx.saved_tensors
        ns, nt, h, C = fs.size(0), ft.size(0), fs.size(1), W.size(0)
        dev = fs.device
        gfs = torch.empty_like(fs) if ctx.needs_input_grad[0] else None
        gft = torch.empty_like(ft) if ctx.needs_input_grad[1] else None
        gW, gb = torch.empty_like(W), torch.empty(C, dtype=torch.float32, device=dev)
        gl = gl.reshape(1).to(torch.float32).contiguous()
        ws, _ = _lib.scratch("gda_grl_disc_workspace_bytes", dev, "disc", ns + nt, h, C)
        _lib.call("gda_grl_disc_ce_bwd_f32", fs, h, ns, ft, h, nt, h, C, W, labels, probs, gl, ctx.alpha, gfs, gft, gW,
                  gb, ws, ws.numel(), _lib.stream())
        return gfs, gft, gW, gb, None, None


def grl_disc_ce(source_feat, target_feat, weight, bias, alpha, labels=None):
    """``F.cross_entropy(Linear(GradReverse(cat(source, target))), domain_labels)`` fused
    (a2gnn.py:197-205 / grade.py:170-176).  Default labels: 0 for source rows, 1 for target.
    ``alpha`` may be a 0-dim DEVICE tensor (the captured step updates it per epoch without touching
    the graph): the fused kernel then runs with the reversal folded out (alpha = -1) behind a
    tensor-valued GradReverse."""
    if torch.is_tensor(alpha):
        from .nn.reverse_layer import GradReverse
        return _GrlDiscCE.apply(GradReverse.apply(source_feat, alpha), GradReverse.apply(target_feat, alpha),
                                weight, bias, -1.0, labels)
    return _GrlDiscCE.apply(source_feat, target_feat, weight, bias, alpha, labels)


# ------------------------------ GRL + two-layer discriminator + per-domain CE (fused) --
def _grl_mlp_fwd(ctx, es, et, W1, b1, W2, b2, alpha, p, head=0):
    ctx.head = head
    es, et = _f32c(es, "source_feat"), _f32c(et, "target_feat")
    W1, b1, W2, b2 = _f32c(W1, "W1"), _f32c(b1, "b1"), _f32c(W2, "W2"), _f32c(b2, "b2")
    ns, nt, h, a = es.size(0), et.size(0), es.size(1), W1.size(0)
    dev = es.device
    seed, step, site, _ = dropout_state.generator(dev, sites=2)      # two call sites: source rows, target rows
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    ws, _ = _lib.scratch("gda_grl_mlp_ce_workspace_bytes", dev, "disc_mlp", h, a)
    with profiler.region(f"disc_mlp_fwd[{h}x{a}]", 2, 4 * (ns + nt) * h, 2 * (ns + nt) * a * (h + W2.size(0))):
        _lib.call("gda_mlp_head_fwd_f32", head, es, h, ns, et, h, nt, h, a, W1, b1, W2, b2, float(p), seed, step, site,
                  losses, ws, ws.numel(), _lib.stream())
    ctx.save_for_backward(es, et, W1, b1, W2, b2, alpha if torch.is_tensor(alpha) else None)
    ctx.alpha = None if torch.is_tensor(alpha) else float(alpha)
    ctx.p, ctx.seed, ctx.site = float(p), seed, site
    return losses


def _grl_mlp_bwd(ctx, g, stride):
    es, et, W1, b1, W2, b2, alpha_dev = ctx.saved_tensors
    ns, nt, h, a = es.size(0), et.size(0), es.size(1), W1.size(0)
    dev = es.device
    ges = torch.empty_like(es) if ctx.needs_input_grad[0] else None
    get = torch.empty_like(et) if ctx.needs_input_grad[1] else None
    gW1, gb1, gW2, gb2 = torch.empty_like(W1), torch.empty_like(b1), torch.empty_like(W2), torch.empty_like(b2)
    if alpha_dev is not None:
        alpha_dev = alpha_dev.detach().reshape(1).to(torch.float32)
    ws, _ = _lib.scratch("gda_grl_mlp_ce_workspace_bytes", dev, "disc_mlp", h, a)
    # recomputed first layer, d hidden . W1 (input gradients), d hidden^T x (weight gradient): 3 products of rows x a x h
    with profiler.region(f"disc_mlp_bwd[{h}x{a}]", 2, 4 * (ns + nt) * h * (2 if ges is not None else 1), 6 * (ns + nt) * a * h):
        _lib.call("gda_mlp_head_bwd_f32", ctx.head, es, h, ns, et, h, nt, h, a, W1, b1, W2, b2, ctx.p, ctx.seed,
                  dropout_state.counter(dev), ctx.site, g, stride, 0.0 if ctx.alpha is None else ctx.alpha, alpha_dev,
                  ges, get, gW1, gb1, gW2, gb2, ws, ws.numel(), _lib.stream())
    return ges, get, gW1, gb1, gW2, gb2, None, None


class _GrlMlpCESum(torch.autograd.Function):
    """The two domain means added, as the reference adds them: one scalar out, one scalar gradient in."""

    @staticmethod
    def forward(ctx, es, et, W1, b1, W2, b2, alpha, p):
        return _grl_mlp_fwd(ctx, es, et, W1, b1, W2, b2, alpha, p)[2]

    @staticmethod
    def backward(ctx, g):
        return _grl_mlp_bwd(ctx, g.reshape(1).to(torch.float32).contiguous(), 0)


class _GrlMlpCEPair(torch.autograd.Function):
    """The two domain means separately (data-parallel callers weight them by node counts)."""

    @staticmethod
    def forward(ctx, es, et, W1, b1, W2, b2, alpha, p):
        losses = _grl_mlp_fwd(ctx, es, et, W1, b1, W2, b2, alpha, p)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_s, g_t):
        return _grl_mlp_bwd(ctx, torch.stack([g_s.reshape(()).to(torch.float32), g_t.reshape(()).to(torch.float32)]), 1)


class _CriticMeans(torch.autograd.Function):
    """``(mean D(source rows), mean D(target rows))`` for ``D = Linear(h, a) - ReLU - Dropout(p) - Linear(a, 1) - Sigmoid``
    (AdaGCN's critic inside the ENCODER's loss, adagcn.py:190-193): the row kernels of the two-layer discriminator with
    the sigmoid-mean head (gda_mlp_head_*_f32, head = 1), no gradient reversal."""

    @staticmethod
    def forward(ctx, es, et, W1, b1, W2, b2, p):
        losses = _grl_mlp_fwd(ctx, es, et, W1, b1, W2, b2, -1.0, p, head=1)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_s, g_t):
        return _grl_mlp_bwd(ctx, torch.stack([g_s.reshape(()).to(torch.float32), g_t.reshape(()).to(torch.float32)]), 1)[:7]


class _CriticMeansVec(torch.autograd.Function):
    """:class:`_CriticMeans` with the kernel's result block ``[mean D(source), mean D(target), unused]`` handed on as ONE
    tensor: its gradient arrives as one tensor too (no stack in front of the backward kernels)."""

    @staticmethod
    def forward(ctx, es, et, W1, b1, W2, b2, p):
        return _grl_mlp_fwd(ctx, es, et, W1, b1, W2, b2, -1.0, p, head=1)

    @staticmethod
    def backward(ctx, g):
        return _grl_mlp_bwd(ctx, g.to(torch.float32).contiguous(), 1)[:7]


class _AddAbsGap(torch.autograd.Function):
    """``base + weight * |v[0] - v[1]|`` for a scalar ``base`` and a device vector ``v`` in four small launches forward and
    one backward (the composed expression and its autograd graph: seventeen)."""
    _wvec = {}

    @staticmethod
    def forward(ctx, base, v, weight):
        key = (float(weight), v.device, v.numel())
        wv = _AddAbsGap._wvec.get(key)
        if wv is None:
            wv = _AddAbsGap._wvec[key] = torch.tensor([weight, -weight] + [0.0] * (v.numel() - 2), dtype=torch.float32, device=v.device)
        d = v[0] - v[1]
        svec = torch.sign(d) * wv                         # d |gap| / d v, times the weight
        ctx.save_for_backward(svec)
        return torch.addcmul(base, d, svec[0])            # d * sign(d) * weight = weight * |d|

    @staticmethod
    def backward(ctx, g):
        (svec,) = ctx.saved_tensors
        return g, g * svec, None


def critic_abs_gap_loss(base, source_feat, target_feat, W1, b1, W2, b2, dropout_p, weight):
    """``base + weight * |mean D(source) - mean D(target)|`` (AdaGCN's encoder loss, adagcn.py:186-193) for the
    sigmoid-headed two-layer critic: the fused means (:func:`critic_means`) and the scalar tail in a handful of launches."""
    v = _CriticMeansVec.apply(source_feat, target_feat, W1, b1, W2, b2, dropout_p)
    return _AddAbsGap.apply(base, v, float(weight))


def critic_means_ok(es, W1, W2):
    return (es.is_cuda and es.dtype == torch.float32 and es.dim() == 2 and es.size(1) <= 128
            and W1.size(0) <= 64 and W2.dim() == 2 and W2.size(0) == 1)


def critic_means(source_feat, target_feat, W1, b1, W2, b2, dropout_p=0.0):
    """The two means ``torch.mean(D(source)), torch.mean(D(target))`` of a sigmoid-headed two-layer critic, fused."""
    return _CriticMeans.apply(source_feat, target_feat, W1, b1, W2, b2, dropout_p)


def grl_mlp_ce_ok(es, W1, W2):
    """Shapes the fused two-layer discriminator covers (csrc/gda_disc_mlp.hip)."""
    return (es.is_cuda and es.dtype == torch.float32 and es.dim() == 2 and es.size(1) <= 128
            and W1.size(0) <= 64 and W2.size(0) == 2)


def grl_mlp_ce(source_feat, target_feat, W1, b1, W2, b2, alpha, dropout_p=0.0, pair=False):
    """``CE(D(GradReverse(source)), 0).mean() + CE(D(GradReverse(target)), 1).mean()`` (``pair``: the two means as a
    tuple) for the two-layer discriminator ``D = Linear(h, a) - ReLU - Dropout(p) - Linear(a, 2)`` of UDAGCN
    (udagcn.py:176-190, udagcn_base.py:157-162), fused: one row kernel and one fold each way (include/gda_hip.h:
    gda_grl_mlp_ce_fwd_f32 / _bwd_f32).  ``alpha`` may be a 0-dim device tensor (captured steps)."""
    fn = _GrlMlpCEPair if pair else _GrlMlpCESum
    return fn.apply(source_feat, target_feat, W1, b1, W2, b2, alpha, dropout_p)


# ------------------------------------------------------ LSGAN discriminator head (DANE) --
class _LsganHead(torch.autograd.Function):
    """``mean((Linear(h, 1)(relu(x W1^T + b1)) - target) ** 2)``: first layer on the matrix-core kernels (bias in the
    epilogue), everything after it in one pass each way over Z (gda_lsgan_head_fwd/bwd_f32); gW1 / gb1 / gx from gZ
    by the TN (column sums as a by-product) and NN kernels."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, target):
        x, W1, b1 = _f32c(x, "rows"), _f32c(W1, "W1"), _f32c(b1, "b1")
        w2, b2 = _f32c(W2, "W2").reshape(-1), _f32c(b2, "b2").reshape(-1)
        rows, a = x.size(0), W1.size(0)
        Z = gemm(GEMM_NT, x, W1, bias=b1)
        pre = torch.empty(rows, dtype=torch.float32, device=x.device)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        ws, _ = _lib.scratch("gda_lsgan_head_workspace_bytes", x.device, "lsgan", a)
        _lib.call("gda_lsgan_head_fwd_f32", Z, a, rows, a, w2, b2, float(target), pre, loss, ws, ws.numel(),
                  _lib.stream())
        ctx.save_for_backward(x, W1, Z, w2, pre)
        ctx.target, ctx.w2_shape, ctx.b2_shape = float(target), W2.shape, b2.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        x, W1, Z, w2, pre = ctx.saved_tensors
        rows, a = Z.shape
        gZ = torch.empty_like(Z)
        gw2 = torch.empty(a, dtype=torch.float32, device=Z.device)
        gb2 = torch.empty(1, dtype=torch.float32, device=Z.device)
        g = g.reshape(1).to(torch.float32).contiguous()
        ws, _ = _lib.scratch("gda_lsgan_head_workspace_bytes", Z.device, "lsgan", a)
        _lib.call("gda_lsgan_head_bwd_f32", Z, a, rows, a, w2, pre, ctx.target, g, gZ, a, gw2, gb2, ws, ws.numel(),
                  _lib.stream())
        gx = gemm(GEMM_NN, gZ, W1) if ctx.needs_input_grad[0] else None
        gb1 = torch.empty(a, dtype=torch.float32, device=Z.device)
        gW1 = gemm(GEMM_TN, gZ, x, colsum=gb1)
        return gx, gW1, gb1, gw2.reshape(ctx.w2_shape), gb2.reshape(ctx.b2_shape), None


def lsgan_head_ok(x, W1, W2):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and 1 <= x.size(0) <= 200_000
            and W1.size(0) <= 256 and W1.size(1) <= 256 and W2.size(0) == 1)


def lsgan_head(x, W1, b1, W2, b2, target):
    """``((D(x) - target) ** 2).mean()`` for DANE's ``D = Linear(h, a) - ReLU - Linear(a, 1)`` (dane.py:241-247,
    339-350, 468-470): one GEMM, one row pass and one fold forward; one row pass, one fold and the GEMMs of the first
    layer backward."""
    return _LsganHead.apply(x, W1, b1, W2, b2, target)


# ------------------------------------------- Wasserstein critic update (WGAN-GP), fused --
def wgan_critic_grads(es, et, idx_s, idx_t, alpha, W1, b1, W2, b2, dropout_p, gp_weight, out):
    """Loss and parameter gradients of one critic update of AdaGCN (pygda/models/adagcn.py:169-183,387-454)
    in closed form (include/gda_hip.h: gda_wgan_critic_f32): ``out = (loss [1], gW1, gb1, gW2, gb2)``
    preallocated like the parameters -- the gradients land where the critic's optimiser reads them."""
    es, et = _f32c(es, "encoded_source"), _f32c(et, "encoded_target")
    n_s, h = es.shape
    n_t = et.size(0)
    a = W1.size(0)
    n_i = 0 if idx_s is None else idx_s.numel()
    ws, _ = _lib.scratch("gda_wgan_critic_workspace_bytes", es.device, "critic", n_s, n_t, n_i, h, a)
    seed, step, site, _, _ = dropout_state.generator(es.device, sites=3)   # three mask sets: D(es), D(et), penalty rows
    loss, gW1, gb1, gW2, gb2 = out
    # algorithmic work of one update: per penalty row the products W1 x, W1^T u, W1 y and the row's u y^T (2 a h flops
    # each), per gap row its u x^T; the encodings read once, two rows gathered per interpolate
    rows_gp = n_s + n_t + n_i
    with profiler.region(f"wgan_critic[{h}x{a}]", 2 if h in (64, 96, 128) and a % 4 == 0 else 7,
                         4 * h * (n_s + n_t + 2 * n_i), 2 * a * h * (4 * rows_gp + n_s + n_t)):
        _lib.call("gda_wgan_critic_f32", es, n_s, et, n_t, h, idx_s, idx_t,
                  None if alpha is None else _f32c(alpha, "alpha"), n_i, _f32c(W1, "W1"), _f32c(b1, "b1"),
                  _f32c(W2, "W2"), _f32c(b2, "b2"), a, float(dropout_p), seed, step, site, float(gp_weight), loss, gW1, gb1, gW2, gb2, ws, ws.numel(), _lib.stream())
    return loss


def wgan_critic_adam(es, et, idx_s, idx_t, alpha, params, optimizer, dropout_p, gp_weight, loss):
    """One iteration of AdaGCN's critic loop INCLUDING ``c_optimizer.step()`` (pygda/models/adagcn.py:169-183) in the two
    launches of :func:`wgan_critic_grads` (include/gda_hip.h: gda_wgan_critic_adam_f32): ``params = (W1, b1, W2, b2)`` with
    preallocated ``.grad``, ``optimizer`` the :class:`pygda_amd.optim.Adam` that holds exactly them in one group.  Returns
    False -- nothing launched, nothing changed -- when the shapes are not the matrix-core path's or the optimiser is not
    of that form; the caller then runs :func:`wgan_critic_grads` + ``optimizer.step()``: the same bits."""
    from .optim import Adam
    if not isinstance(optimizer, Adam) or len(optimizer.param_groups) != 1 or optimizer.grad_aliases:
        return False
    group = optimizer.param_groups[0]
    if len(group["params"]) != 4 or any(a is not b for a, b in zip(group["params"], params)):
        return False
    es, et = _f32c(es, "encoded_source"), _f32c(et, "encoded_target")
    n_s, h = es.shape
    n_t, a = et.size(0), params[0].size(0)
    W1 = params[0]
    if not (h in (64, 96, 128) and a % 4 == 0 and all(p.is_contiguous() and p.dtype == torch.float32 for p in params)
            and (es.data_ptr() | et.data_ptr() | W1.data_ptr()) % 16 == 0):
        return False
    n_i = 0 if idx_s is None else idx_s.numel()
    ws, _ = _lib.scratch("gda_wgan_critic_workspace_bytes", es.device, "critic", n_s, n_t, n_i, h, a)
    table = (_lib.AdamTensorStruct * 4)()
    for k, p in enumerate(params):
        stt = optimizer._state(p)
        if p.grad is None or not p.grad.is_contiguous() or any(stt[n].stride() != p.stride() for n in ("exp_avg", "exp_avg_sq")):
            return False
        table[k] = _lib.AdamTensorStruct(p.data_ptr(), p.grad.data_ptr(), stt["exp_avg"].data_ptr(),
                                         stt["exp_avg_sq"].data_ptr(), stt["step"].data_ptr(), p.numel())
    seed, step, site, _, _ = dropout_state.generator(es.device, sites=3)   # three mask sets: D(es), D(et), penalty rows
    b1_, b2_ = group["betas"]
    rows_gp = n_s + n_t + n_i
    with profiler.region(f"wgan_critic[{h}x{a}]", 2, 4 * h * (n_s + n_t + 2 * n_i), 2 * a * h * (4 * rows_gp + n_s + n_t)):
        _lib.call("gda_wgan_critic_adam_f32", es, n_s, et, n_t, h, idx_s, idx_t,
                  None if alpha is None else _f32c(alpha, "alpha"), n_i, a, float(dropout_p), seed, step, site,
                  float(gp_weight), loss, table, float(group["lr"]), float(b1_), float(b2_), float(group["eps"]),
                  float(group["weight_decay"]), ws, ws.numel(), _lib.stream())
    return True


# ------------------------------- SpecReg: three-layer critic update, gap and spectral hinges (csrc/gda_critic3.hip) --
CRITIC3_MIN_WIDTH, CRITIC3_MAX_WIDTH = 4, 128
# the row kernel's grid cap (256 workgroups) times a workgroup's 4 x 32 rows: gda_critic3_rows_per_trip() of the library
# (tests/test_specreg_host.py holds the two to each other)
CRITIC3_ROWS_PER_TRIP = 256 * 128


def critic3_params(critic):
    """``(W1, b1, W2, b2, W3, b3)`` of a Linear-ReLU-Linear-ReLU-Linear ``Sequential``."""
    return (critic[0].weight, critic[0].bias, critic[2].weight, critic[2].bias, critic[4].weight, critic[4].bias)


def critic3_refusal(es, critic):
    """Why the gda_critic3_* entry points do not take ``(es, critic)`` -- one of "input", "module", "width", "bias",
    "shapes", "device" -- or None when they do.  The envelope: CUDA fp32 2-D encodings against SpecReg's critic
    (specreg.py:281-287), an ``nn.Sequential`` of exactly Linear(h, h) - ReLU - Linear(h, h) - ReLU - Linear(h, 1) with
    biases, h % 4 == 0 and 4 <= h <= 128.  The device is asked last, so that each answer names its own property."""
    nn = torch.nn
    if not (isinstance(es, torch.Tensor) and es.dtype == torch.float32 and es.dim() == 2 and es.size(0) >= 1):
        return "input"
    if not (isinstance(critic, nn.Sequential) and len(critic) == 5
            and all(isinstance(critic[k], nn.Linear) for k in (0, 2, 4))
            and all(isinstance(critic[k], nn.ReLU) for k in (1, 3))):
        return "module"
    h = es.size(1)
    if h % 4 != 0 or not CRITIC3_MIN_WIDTH <= h <= CRITIC3_MAX_WIDTH:
        return "width"
    if any(critic[k].bias is None for k in (0, 2, 4)):
        return "bias"
    params = critic3_params(critic)
    if ([tuple(p.shape) for p in params] != [(h, h), (h,), (h, h), (h,), (1, h), (1,)]
            or not all(p.dtype == torch.float32 and p.is_contiguous() for p in params)):
        return "shapes"
    if not (es.is_cuda and all(p.is_cuda for p in params)):
        return "device"
    return None


def critic3_ok(es, critic):
    """True when :func:`critic3_refusal` has no objection; anything else keeps the torch composition."""
    return critic3_refusal(es, critic) is None


def _critic3_work(n_s, n_t, h):
    """Algorithmic bytes and flops of one update: the encodings read once; per row six [h, h] matrix-vector products and
    two outer products, 16 h^2 flops."""
    return 4 * h * (n_s + n_t), 16 * h * h * (n_s + n_t)


def critic3_grads(es, et, params, out):
    """Loss and parameter gradients of one critic update of SpecReg (pygda/models/specreg.py:194-200,380-419) in closed
    form (include/gda_hip.h: gda_critic3_update_f32): ``params = (W1, b1, W2, b2, W3, b3)``, ``out = (loss [1], gW1, gb1,
    gW2, gb2, gW3, gb3)`` preallocated like the parameters -- the gradients land where the critic's optimiser reads them."""
    es, et = _f32c(es, "encoded_source"), _f32c(et, "encoded_target")
    n_s, h = es.shape
    n_t = et.size(0)
    params = tuple(_f32c(p, "critic parameter") for p in params)
    # the entry point writes through raw pointers: every extent is checked here
    if es.dim() != 2 or et.dim() != 2 or et.size(1) != h:
        raise ValueError(f"encodings of shapes {tuple(es.shape)} and {tuple(et.shape)}")
    if [tuple(p.shape) for p in params] != [(h, h), (h,), (h, h), (h,), (1, h), (1,)]:
        raise ValueError(f"critic parameters {[tuple(p.shape) for p in params]} for width {h}")
    if len(out) != 7 or out[0].numel() != 1 or any(o.shape != p.shape for o, p in zip(out[1:], params)):
        raise ValueError("out must be (loss [1], gW1, gb1, gW2, gb2, gW3, gb3) shaped like the parameters")
    if not all(o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() for o in out):
        raise ValueError("out tensors must be contiguous fp32 tensors on the device")
    ws, _ = _lib.scratch("gda_critic3_workspace_bytes", es.device, "critic3", n_s, n_t, h)
    nbytes, flops = _critic3_work(n_s, n_t, h)
    with profiler.region(f"critic3[{h}]", 6, nbytes, flops):
        _lib.call("gda_critic3_update_f32", es, n_s, et, n_t, h, *params, *out,
                  ws, ws.numel(), _lib.stream())
    return out[0]


def critic3_adam(es, et, params, optimizer, loss):
    """One iteration of SpecReg's critic loop INCLUDING ``optimizer_critic.step()`` (specreg.py:194-200) in the launches of
    :func:`critic3_grads` (include/gda_hip.h: gda_critic3_update_adam_f32): ``params = (W1, b1, W2, b2, W3, b3)`` with
    preallocated ``.grad``, ``optimizer`` the :class:`pygda_amd.optim.Adam` that holds exactly them in one group with no
    gradient aliases.  Returns False -- nothing launched, nothing changed -- otherwise; the caller then runs
    :func:`critic3_grads` + ``optimizer.step()``: the same bits."""
    from .optim import Adam
    if not isinstance(optimizer, Adam) or len(optimizer.param_groups) != 1 or optimizer.grad_aliases:
        return False
    group = optimizer.param_groups[0]
    if len(group["params"]) != 6 or len(params) != 6 or any(a is not b for a, b in zip(group["params"], params)):
        return False
    es, et = _f32c(es, "encoded_source"), _f32c(et, "encoded_target")
    n_s, h = es.shape
    n_t = et.size(0)
    if not (h % 4 == 0 and CRITIC3_MIN_WIDTH <= h <= CRITIC3_MAX_WIDTH and et.size(1) == h
            and all(p.is_cuda and p.is_contiguous() and p.dtype == torch.float32 for p in params)):
        return False
    table = (_lib.AdamTensorStruct * 6)()
    for k, p in enumerate(params):
        stt = optimizer._state(p)
        if p.grad is None or not p.grad.is_contiguous() or any(stt[n].stride() != p.stride() for n in ("exp_avg", "exp_avg_sq")):
            return False
        table[k] = _lib.AdamTensorStruct(p.data_ptr(), p.grad.data_ptr(), stt["exp_avg"].data_ptr(),
                                         stt["exp_avg_sq"].data_ptr(), stt["step"].data_ptr(), p.numel())
    ws, _ = _lib.scratch("gda_critic3_workspace_bytes", es.device, "critic3", n_s, n_t, h)
    b1_, b2_ = group["betas"]
    nbytes, flops = _critic3_work(n_s, n_t, h)
    with profiler.region(f"critic3[{h}]", 6, nbytes, flops):
        _lib.call("gda_critic3_update_adam_f32", es, n_s, et, n_t, h, loss, table, float(group["lr"]), float(b1_),
                  float(b2_), float(group["eps"]), float(group["weight_decay"]), ws, ws.numel(), _lib.stream())
    return True


class _Critic3Gap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, es, et, W1, b1, W2, b2, W3, b3):
        es, et = _f32c(es, "encoded_source"), _f32c(et, "encoded_target")
        n_s, h = es.shape
        n_t = et.size(0)
        want = any(ctx.needs_input_grad[:2])
        means = torch.empty(2, dtype=torch.float32, device=es.device)
        ges = torch.empty_like(es) if want else None
        get = torch.empty_like(et) if want else None
        ws, _ = _lib.scratch("gda_critic3_workspace_bytes", es.device, "critic3", n_s, n_t, h)
        with profiler.region(f"critic3_gap[{h}]", 2, 4 * h * (n_s + n_t) * (2 if want else 1), 8 * h * h * (n_s + n_t)):
            _lib.call("gda_critic3_gap_f32", es, n_s, et, n_t, h, *(_f32c(p.detach(), "critic parameter") for p in (W1, b1, W2, b2, W3, b3)),
                      means, ges, get, ws, ws.numel(), _lib.stream())
        ctx.grads = (ges, get)
        return means[0] - means[1]

    @staticmethod
    def backward(ctx, g):
        ges, get = ctx.grads
        return (ges * g if ctx.needs_input_grad[0] else None, get * g if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None)


def critic3_gap(es, et, W1, b1, W2, b2, W3, b3):
    """``mean D(es) - mean D(et)`` for SpecReg's critic (pygda/models/specreg.py:202, ``loss_grl``) with its input
    gradients in ONE row launch (include/gda_hip.h: gda_critic3_gap_f32): D is piecewise linear, so the gradient
    ``+grad_x D / n_s`` | ``-grad_x D / n_t`` is formed in the forward when a gradient is wanted and the backward only scales
    it by the incoming scalar.  The critic's parameters receive NO gradient: the trainer zeroes the critic's ``.grad``
    before every use (``optimizer_critic.zero_grad()`` opens each critic iteration), so what the reference accumulates
    there from this term is never observed."""
    return _Critic3Gap.apply(es, et, W1, b1, W2, b2, W3, b3)


_HINGE_ROWS = 512     # the NN product's deterministic split over the reduction wants M <= 512 (csrc/gda_gemm.hip)


class _SpectralHinge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eivec, encoded, thr_smooth, gamma_smooth, thr_mfr, gamma_mfr):
        eivec, encoded = _f32c(eivec, "eivec"), _f32c(encoded, "encoded")
        k, h = eivec.size(0), encoded.size(1)
        X = torch.empty(k, h, dtype=torch.float32, device=encoded.device)
        for r0 in range(0, k, _HINGE_ROWS):     # at most 512 rows a call: gda_gemm_f32 then splits the N-long reduction
            rows = min(_HINGE_ROWS, k - r0)
            gemm_raw(GEMM_NN, rows, h, eivec.size(1), eivec[r0:r0 + rows], eivec.size(1), encoded, h, X[r0:r0 + rows], h,
                     f"spectral_projection[{rows}x{h}]")
        value = torch.empty(1, dtype=torch.float32, device=encoded.device)
        G = torch.empty_like(X)
        ws, nbytes = _lib.scratch("gda_spectral_hinge_workspace_bytes", encoded.device, "spectral_hinge", k, h)
        with profiler.region(f"spectral_hinge[{k}x{h}]", 1, 8 * k * h, 10 * k * h):
            _lib.call("gda_spectral_hinge_f32", X, k, h, float(thr_smooth), float(gamma_smooth), float(thr_mfr),
                      float(gamma_mfr), value, G, ws, nbytes, _lib.stream())
        ctx.save_for_backward(eivec, G)
        return value[0]

    @staticmethod
    def backward(ctx, g):
        eivec, G = ctx.saved_tensors
        ge = gemm(GEMM_TN, eivec, G) * g if ctx.needs_input_grad[1] else None
        return None, ge, None, None, None, None


def spectral_hinge(eivec, encoded, thr_smooth, gamma_smooth, thr_mfr, gamma_mfr):
    """SpecReg's regulariser of one domain (pygda/models/specreg.py:209-215) on ``X = eivec @ encoded``:
    ``gamma_smooth * relu(|X[:-1] - X[1:]| - thr_smooth).mean() + gamma_mfr * relu(|X| - thr_mfr).mean()``, a term present only
    if its threshold is > 0.  The projection is the project's GEMM, the hinges and their gradient one launch
    (include/gda_hip.h: gda_spectral_hinge_f32); the backward is ``eivec^T G`` scaled by the incoming scalar, no gradient
    for ``eivec``.  With both thresholds off nothing is launched and the value is 0 (the reference forms the projection
    even then; the value does not depend on it)."""
    if thr_smooth <= 0 and thr_mfr <= 0:
        return encoded.new_zeros(())
    return _SpectralHinge.apply(eivec, encoded, thr_smooth, gamma_smooth, thr_mfr, gamma_mfr)


# -------------------------------------------------------------------------- gather --
def gather_rows(x, idx):
    """``x[idx]`` for a ``[N, d]`` fp32 feature matrix (mini-batch assembly)."""
    x = _f32c(x, "x")
    _lib.require_gpu_tensor(idx, "idx", torch.int64)
    idx = idx.contiguous()
    out = torch.empty(idx.numel(), x.size(1), dtype=torch.float32, device=x.device)
    _lib.call("gda_gather_rows_f32", x, x.size(1), x.size(1), idx, idx.numel(), out, x.size(1), _lib.stream())
    return out


# ---------------------------------------------------------- graph-level readout --
class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg_ptr, batch):
        x = _f32c(x, "x")
        G, d = seg_ptr.numel() - 1, x.size(1)
        out = torch.empty(G, d, dtype=torch.float32, device=x.device)
        _lib.call("gda_segment_mean_fwd_f32", x, d, seg_ptr, G, d, out, d, _lib.stream())
        ctx.save_for_backward(seg_ptr, batch)
        ctx.n = x.size(0)
        return out

    @staticmethod
    def backward(ctx, gout):
        seg_ptr, batch = ctx.saved_tensors
        gout = gout.contiguous()
        d = gout.size(1)
        gx = torch.empty(ctx.n, d, dtype=torch.float32, device=gout.device)
        _lib.call("gda_segment_mean_bwd_f32", gout, d, seg_ptr, batch, ctx.n, d, gx, d, _lib.stream())
        return gx, None, None


def segment_ptr(batch, size=None):
    """``seg_ptr [G+1]`` of a SORTED graph-index vector (what a DataLoader's collation produces), cached on the
    tensor; an unsorted vector is rejected (one device check per vector): the readout kernel walks contiguous rows."""
    hit = getattr(batch, "_gda_seg_ptr", None)
    if hit is not None and (size is None or hit.numel() - 1 == size):
        return hit
    _lib.require_gpu_tensor(batch, "batch", torch.int64)
    if batch.numel() > 1 and not getattr(batch, "_gda_sorted", False) and bool((batch[1:] < batch[:-1]).any()):
        raise ValueError("global_mean_pool: `batch` must be sorted (nodes of a graph contiguous), as PyG's DataLoader "
                         "collates it")
    G = (int(batch[-1]) + 1 if batch.numel() else 0) if size is None else int(size)
    seg = torch.zeros(G + 1, dtype=torch.int64, device=batch.device)
    if batch.numel():
        seg[1:] = torch.cumsum(torch.bincount(batch, minlength=G), 0)
    batch._gda_seg_ptr = seg
    return seg


def segment_mean(x, batch, size=None):
    """``global_mean_pool(x, batch)`` (pygda/nn/a2gnn_base.py:141) for a sorted ``batch``."""
    return _SegmentMean.apply(x, segment_ptr(batch, size), batch.contiguous())


# ------------------------------------------------------------ ReLU + dropout (fused) --
class _DropoutState:
    """Device step counter + per-step call-site numbering for the fused activation's generator."""

    def __init__(self):
        self.step = {}           # device -> int64[1]
        self.site = 0
        self.seed = None

    def counter(self, dev):
        t = self.step.get(dev)
        if t is None:
            t = self.step[dev] = torch.zeros(1, dtype=torch.int64, device=dev)
        return t

    def next_step(self, dev):
        """Called by the trainers once per training step (inside the captured graph as well)."""
        self.counter(dev).add_(1)
        self.site = 0

    def next_site(self):
        self.site += 1
        return self.site

    def generator(self, dev, sites=1):
        """``(seed, step counter, site)`` -- with ``sites=2`` ``(seed, step counter, site, site)`` -- : the generator
        arguments of a masking kernel, in the ABI's order.  The seed is drawn on first use."""
        if self.seed is None:
            self.seed = int(torch.initial_seed()) & (2 ** 63 - 1)
        return (self.seed, self.counter(dev), *[self.next_site() for _ in range(sites)])


dropout_state = _DropoutState()


class _ReluDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        x = _f32c(x, "x")
        y = torch.empty_like(x)
        _lib.call("gda_relu_dropout_fwd_f32", x, y, x.numel(), float(p), *dropout_state.generator(x.device),
                  _lib.stream())
        ctx.save_for_backward(y)
        ctx.p = float(p)
        ctx.sink = _offer_sink(y, p, wanted=ctx.needs_input_grad[0])
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        if ctx.sink is not None and ctx.sink.mine(gy):       # the producer stored it masked already (GradSink)
            return gy, None
        gy = gy.contiguous()
        gx = torch.empty_like(gy)
        _lib.call("gda_relu_dropout_bwd_f32", gy, y, gx, gy.numel(), ctx.p, _lib.stream())
        return gx, None


class _ReluDropoutT(torch.autograd.Function):
    """The activation across the layout change: column-major input ``[d, n_pad]`` -> row-major ``[n, d]``
    output, and back in the backward pass (gda_relu_dropout_{fwd,bwd}_cm_f32)."""

    @staticmethod
    def forward(ctx, xT, n, p, gen=None):
        """``gen``: a ``(seed, step counter, site)`` triple drawn earlier (:class:`PreActCM`), else drawn here."""
        d, n_pad = xT.shape
        y = torch.empty(n, d, dtype=torch.float32, device=xT.device)
        _lib.call("gda_relu_dropout_fwd_cm_f32", xT, n_pad, y, n, d, float(p),
                  *(dropout_state.generator(xT.device) if gen is None else gen), _lib.stream())
        ctx.save_for_backward(y)
        ctx.p, ctx.n_pad = float(p), n_pad
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return _relu_dropout_t_backward(y, gy, ctx.p, ctx.n_pad), None, None, None


def _relu_dropout_t_backward(y, gy, p, n_pad):
    """Row-major ``gy``, ``y [n, d]`` -> the column-major gradient ``gxT [d, n_pad]`` of the pre-activation."""
    n, d = y.shape
    gy = gy.contiguous()
    gxT = torch.empty(d, n_pad, dtype=torch.float32, device=gy.device)
    if n_pad != n:
        gxT[:, n:].zero_()                       # the padding rows of a column are never read as values,
                                                 # but they may be summed with another consumer's gradient
    _lib.call("gda_relu_dropout_bwd_cm_f32", gy, y, gxT, n_pad, n, d, p, _lib.stream())
    return gxT


class _ReluDropoutPair(torch.autograd.Function):
    """gda_relu_dropout_pair_{fwd,bwd}_f32: ``[drop_a(relu(x)) ; drop_b(relu(x))]`` ``[2n, d]``."""

    @staticmethod
    def forward(ctx, x, p):
        x = _f32c(x, "x")
        n, d = x.shape
        y = torch.empty(2 * n, d, dtype=torch.float32, device=x.device)
        _lib.call("gda_relu_dropout_pair_fwd_f32", x, y, n, d, float(p), *dropout_state.generator(x.device, sites=2),
                  _lib.stream())
        ctx.save_for_backward(y)
        ctx.p = float(p)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        n, d = y.size(0) // 2, y.size(1)
        gy = gy.contiguous()
        gx = torch.empty(n, d, dtype=torch.float32, device=gy.device)
        cs = ws = None
        nbytes = 0
        if d <= 1024:                     # column sums of gx ride along: the bias gradient of the layer below
            cs = torch.empty(d, dtype=torch.float32, device=gy.device)
            ws, nbytes = _lib.scratch("gda_relu_dropout_pair_workspace_bytes", gy.device, "pair_colsum", d)
        _lib.call("gda_relu_dropout_pair_bwd_f32", gy, y, gx, n, d, ctx.p, cs, ws, nbytes, _lib.stream())
        global _colsum_hint
        _colsum_hint = (gx.data_ptr(), cs, gx) if cs is not None else None
        return gx, None


def relu_dropout_pair_ok(x):
    return torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.size(1) % 4 == 0


def relu_dropout_pair(x, p, training=True):
    """Two independent ``F.dropout(F.relu(x), p)`` draws of the same ``x [n, d]`` as one stacked ``[2n, d]``."""
    return _ReluDropoutPair.apply(x, float(p) if training else 0.0)


class _SplitHalves(torch.autograd.Function):
    """``x [2n, d] -> (x[:n], x[n:])``; backward stacks the two gradients in one launch (a missing one reads as
    zeros) instead of autograd's fill + copy + add per slice."""

    @staticmethod
    def forward(ctx, x):
        n = x.size(0) // 2
        ctx.shape = (n, x.size(1))
        ctx.set_materialize_grads(False)
        return x.narrow(0, 0, n), x.narrow(0, n, n)

    @staticmethod
    def backward(ctx, ga, gb):
        n, d = ctx.shape
        ref = ga if ga is not None else gb
        if ref is None:
            return None
        out = torch.empty(2 * n, d, dtype=torch.float32, device=ref.device)
        ga = None if ga is None else ga.contiguous()
        gb = None if gb is None else gb.contiguous()
        _lib.call("gda_stack2_f32", ga, gb, out, n * d, _lib.stream())
        return out


def split_halves(x):
    return _SplitHalves.apply(x)


class _SplitRows(torch.autograd.Function):
    """``x [n, d] -> (x[:k], x[k:])`` (views); backward writes the two gradients into ONE buffer (a missing one as
    zeros): two copies instead of autograd's fill + copy per slice and the add that joins them."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.k, ctx.shape = int(k), tuple(x.shape)
        ctx.set_materialize_grads(False)
        return x.narrow(0, 0, ctx.k), x.narrow(0, ctx.k, x.size(0) - ctx.k)

    @staticmethod
    def backward(ctx, ga, gb):
        ref = ga if ga is not None else gb
        if ref is None:
            return None, None
        out = torch.empty(ctx.shape, dtype=ref.dtype, device=ref.device)
        for part, g in ((out[:ctx.k], ga), (out[ctx.k:], gb)):
            if g is None:
                part.zero_()
            else:
                part.copy_(g)
        return out, None


def split_rows(x, k):
    """The first ``k`` rows and the rest of a stacked matrix (a block-diagonal pair of graphs: BaseGDA._stacked_pair)."""
    return _SplitRows.apply(x, k)


class _ReluDropoutSplit(torch.autograd.Function):
    """``split_halves(relu_dropout(x, p))`` for a stacked ``x [2n, d]``: the forward is the ordinary activation kernel,
    the backward masks the two halves' gradients while it stacks them (gda_relu_dropout_bwd2_f32) -- the unmasked
    ``[2n, d]`` stack that `_SplitHalves` + `_ReluDropout` write and read back is never formed."""

    @staticmethod
    def forward(ctx, x, p):
        x = _f32c(x, "x")
        y = torch.empty_like(x)
        _lib.call("gda_relu_dropout_fwd_f32", x, y, x.numel(), float(p), *dropout_state.generator(x.device),
                  _lib.stream())
        ctx.save_for_backward(y)
        ctx.p = float(p)
        ctx.set_materialize_grads(False)
        n = x.size(0) // 2
        a, b = y.narrow(0, 0, n), y.narrow(0, n, n)
        ctx.sinks, ctx.G = (None, None), None
        if _sinks_on and ctx.needs_input_grad[0]:
            # both halves' masked gradients land in ONE [2n, d] buffer: when both producers wrote, it IS the result
            ctx.G = torch.empty_like(y)
            ctx.sinks = (_offer_sink(a, p, ctx.G.narrow(0, 0, n)), _offer_sink(b, p, ctx.G.narrow(0, n, n)))
        return a, b

    @staticmethod
    def backward(ctx, ga, gb):
        (y,) = ctx.saved_tensors
        if ga is None and gb is None:
            return None, None
        n = y.size(0) // 2
        done = [k is not None and k.mine(g) for k, g in zip(ctx.sinks, (ga, gb))]
        if any(done):
            # a half that arrived masked sits in G already; the other one (an ordinary gradient, or none) is masked into its
            # half of G by the ordinary kernel
            for k, (g, ok) in enumerate(zip((ga, gb), done)):
                if ok:
                    continue
                dst, yh = ctx.G.narrow(0, k * n, n), y.narrow(0, k * n, n)
                if g is None:
                    dst.zero_()
                else:
                    g = g.contiguous()
                    _lib.call("gda_relu_dropout_bwd_f32", g, yh, dst, g.numel(), ctx.p, _lib.stream())
            return ctx.G, None
        ga = None if ga is None else ga.contiguous()
        gb = None if gb is None else gb.contiguous()
        gx = torch.empty_like(y)
        _lib.call("gda_relu_dropout_bwd2_f32", ga, gb, y, gx, y.numel() // 2, ctx.p, _lib.stream())
        return gx, None


# ------------------------------- projections of a sampled batch: gather in the operand fetch, activation in the epilogue --
TALL_FUSED = True         # tests/test_gpu_sampler.py turns it off for its reference


class GatheredRows:
    """``base[idx]`` NOT materialised: the feature rows of a sampled batch as (resident feature matrix, node ids).  The
    batch's first projection reads them through the ids in its operand fetch (gda_gemm_tall_fwd_ex_f32) and so does its
    weight gradient (gda_gemm_tall_wgrad_gather_f32): the gather pass that wrote and re-read ``[n, F]`` per domain and step
    is gone.  Quacks like the tensor where the trainers only ask for its shape / device; ``dense()`` materialises."""
    __slots__ = ("base", "idx", "_dense")
    requires_grad = False
    _version = 0

    def __init__(self, base, idx):
        self.base, self.idx, self._dense = base, idx, None

    shape = property(lambda self: torch.Size((self.idx.numel(), self.base.size(1))))
    device = property(lambda self: self.base.device)
    dtype = property(lambda self: self.base.dtype)
    is_cuda = property(lambda self: self.base.is_cuda)

    def size(self, k=None):
        return self.shape if k is None else self.shape[k]

    def dim(self):
        return 2

    def data_ptr(self):
        return 0

    def dense(self):
        if self._dense is None:
            self._dense = gather_rows(self.base, self.idx)
        return self._dense


def tall_fused_ok(x, weight, need_rows=None):
    """The envelope of gda_gemm_tall_fwd_ex_f32 for ``x W^T``: a sampled batch's row count, extents 128 / 256."""
    rows = x.size(0)
    return (TALL_FUSED and x.is_cuda and x.dtype == torch.float32 and rows >= TALL_ROWS
            and weight.size(0) in (128, 256) and weight.size(1) in (128, 256) and x.size(1) == weight.size(1)
            and _os.environ.get("PYGDA_AMD_GEMM_SPLIT_F16", "1") != "0")


class _TallLinearAct(torch.autograd.Function):
    """``act(x W^T + b)`` of a sampled batch in ONE launch: the tall split-fp16 product with (optionally) the feature
    gather in its operand fetch and ``dropout(relu(.))`` in its epilogue.  ``mode``: 0 no activation; 1 activation; 2 two
    independent draws stacked ``[2M, N]`` (A2GNN's two source passes over one layer-0 output); 3 activation, result handed
    out as its two halves (the stacked rows' last layer), both halves offering GradSinks into one ``[M, N]`` buffer.
    Backward: the activation's mask from the saved OUTPUT, the weight gradient through the same node ids, the bias
    gradient as the weight-gradient kernel's column sums (mode 2: of the pair kernel's)."""

    @staticmethod
    def forward(ctx, base, idx, weight, bias, p, mode):
        base, weight = _f32c(base, "x"), _f32c(weight, "weight")
        M = base.size(0) if idx is None else idx.numel()
        K, N = base.size(1), weight.size(0)
        y = torch.empty((2 * M if mode == 2 else M), N, dtype=torch.float32, device=base.device)
        draws = 2 if mode == 2 else (1 if mode else 0)                   # the mask sets the epilogue draws
        gen = dropout_state.generator(base.device, sites=draws) + (0,) * (2 - draws)
        b = None if bias is None else _f32c(bias, "bias")
        with profiler.region(f"dense_projection[{K}x{N}]", 1, 4 * (M * K + N * K + y.numel()), 2 * M * N * K):
            _lib.call("gda_gemm_tall_fwd_ex_f32", M, N, K, base, K, idx, weight, K, y, N, b, draws, float(p), *gen,
                      _lib.stream())
        ctx.mode, ctx.p, ctx.has_bias, ctx.M = mode, float(p), bias is not None, M
        ctx.sink_in = sink_of(base) if idx is None else None
        ctx.save_for_backward(base, idx, weight, y if mode else None)
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        ctx.sink = ctx.sinks = ctx.G = None
        if mode == 1:
            ctx.sink = _offer_sink(y, p, wanted=want)
        if mode == 3:
            h = M // 2
            a, c = y.narrow(0, 0, h), y.narrow(0, h, h)
            if _sinks_on and want:
                ctx.G = torch.empty_like(y)
                ctx.sinks = (_offer_sink(a, p, ctx.G.narrow(0, 0, h)), _offer_sink(c, p, ctx.G.narrow(0, h, h)))
            ctx.set_materialize_grads(False)
            return a, c
        return y

    @staticmethod
    def backward(ctx, g, g2=None):
        base, idx, weight, y = ctx.saved_tensors
        L = _lib.lib()
        M, mode, dev = ctx.M, ctx.mode, weight.device
        N, K = weight.shape
        gb = None
        if mode == 0:
            gpre = g.contiguous()
        elif mode == 1:
            if ctx.sink is not None and ctx.sink.mine(g):
                gpre = g
            else:
                g = g.contiguous()
                gpre = torch.empty_like(g)
                _lib.call("gda_relu_dropout_bwd_f32", g, y, gpre, g.numel(), ctx.p, _lib.stream())
        elif mode == 2:
            # (the bias gradient comes from the weight-gradient kernel's column sums below, as in tall_linear_bias: the same
            # summation order as the unfused composition)
            g = g.contiguous()
            gpre = torch.empty(M, N, dtype=torch.float32, device=dev)
            _lib.call("gda_relu_dropout_pair_bwd_f32", g, y, gpre, M, N, ctx.p, None, None, 0, _lib.stream())
        else:
            ga, gc = g, g2
            if ga is None and gc is None:
                return None, None, None, None, None, None
            h = M // 2
            done = [k is not None and k.mine(t) for k, t in zip(ctx.sinks or (None, None), (ga, gc))]
            if any(done):
                for k, (t, ok) in enumerate(zip((ga, gc), done)):
                    if ok:
                        continue
                    dst, yh = ctx.G.narrow(0, k * h, h), y.narrow(0, k * h, h)
                    if t is None:
                        dst.zero_()
                    else:
                        t = t.contiguous()
                        _lib.call("gda_relu_dropout_bwd_f32", t, yh, dst, t.numel(), ctx.p, _lib.stream())
                gpre = ctx.G
            else:
                ga = None if ga is None else ga.contiguous()
                gc = None if gc is None else gc.contiguous()
                gpre = torch.empty_like(y)
                _lib.call("gda_relu_dropout_bwd2_f32", ga, gc, y, gpre, y.numel() // 2, ctx.p, _lib.stream())
        gw = None
        if ctx.needs_input_grad[2]:
            want_cs = ctx.has_bias and gb is None and ctx.needs_input_grad[3]
            if want_cs:
                gb = torch.empty(N, dtype=torch.float32, device=dev)
            if idx is None:
                gw = gemm(GEMM_TN, gpre, base, colsum=gb if want_cs else None)
            else:
                gw = torch.empty(N, K, dtype=torch.float32, device=dev)
                need = L.gda_gemm_tall_workspace_bytes(GEMM_TN, 128, K, M)
                ok = N == 128 and need > 0 and M >= TALL_WGRAD_ROWS
                if ok:
                    ws = _lib.workspace(need, dev, "gemm")
                    with profiler.region(f"dense_projection_wgrad[{N}x{K}]", 2, 4 * (M * N + M * K + N * K), 2 * M * N * K):
                        _lib.call("gda_gemm_tall_wgrad_gather_f32", K, M, gpre, N, base, K, idx, gw, K,
                                  gb if want_cs else None, ws, ws.numel(), _lib.stream())
                else:
                    gw = gemm(GEMM_TN, gpre, gather_rows(base, idx), colsum=gb if want_cs else None)
        elif ctx.has_bias and gb is None and ctx.needs_input_grad[3]:
            gb = colsum(gpre)
        gx = None
        if idx is None and ctx.needs_input_grad[0]:
            gx = masked_dgrad(gpre, weight, ctx.sink_in) if ctx.sink_in is not None else gemm(GEMM_NN, gpre, weight)
        return gx, None, gw, (gb if ctx.has_bias else None), None, None


def tall_linear_act(x, weight, bias, p, training, mode):
    """See :class:`_TallLinearAct`; ``x`` a tensor or :class:`GatheredRows`; the caller checked :func:`tall_fused_ok`."""
    base, idx = (x.base, x.idx) if isinstance(x, GatheredRows) else (x, None)
    return _TallLinearAct.apply(base, idx, weight, bias, float(p) if training else 0.0, int(mode))


def relu_dropout_split(x, p, training=True):
    """``split_halves(relu_dropout(x, p, training))`` with a fused backward; ``x [2n, d]`` on the device, d % 4 == 0,
    training with p > 0 -- otherwise the composition."""
    if (training and p > 0.0 and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
            and x.size(0) % 2 == 0 and (x.size(0) // 2 * x.size(1)) % 4 == 0):
        return _ReluDropoutSplit.apply(x, float(p))
    return split_halves(relu_dropout(x, p, training))


def relu_dropout_copies(x, copies, p, training=True):
    """``F.dropout(F.relu(x.repeat(copies, 1)), p, training)`` for ``x [n, d]`` without materialising the copies
    (include/gda_hip.h: gda_relu_dropout_tiled_fwd_f32); forward only."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise _lib.GdaError("relu_dropout_copies is forward-only: call it under torch.no_grad()")
    if (not training or p <= 0.0 or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.numel() % 4 != 0
            or not x.is_contiguous() or x.data_ptr() % 16 != 0):
        return relu_dropout(x.repeat(copies, 1), p, training)
    y = torch.empty(copies * x.size(0), x.size(1), dtype=torch.float32, device=x.device)
    _lib.call("gda_relu_dropout_tiled_fwd_f32", x, x.numel(), int(copies), y, float(p),
              *dropout_state.generator(x.device), _lib.stream())
    return y


def relu_dropout(x, p, training=True):
    """``F.dropout(F.relu(x), p, training)`` in one kernel each way (no mask tensor).  A :class:`ColMajor`
    input (the K-step kernel's layout) is consumed as it is and comes out as the ordinary row-major tensor."""
    if isinstance(x, ColMajor):
        return _ReluDropoutT.apply(x.t, x.n, float(p) if training else 0.0)
    if not training or p <= 0.0 or not x.is_cuda or x.dtype != torch.float32:
        return torch.relu(x)
    return _ReluDropout.apply(x, p)


# ------------------------------------------ mixup layer epilogue (StruRW mode='mixup') --
class _MixupCombine(torch.autograd.Function):
    """gda_mixup_combine_{fwd,bwd}_f32: ``XX' = [drop(relu(P + C + b)) ; drop(lam relu(P + Cm + b) +
    (1-lam) relu(Pb + Cm + b))]`` with ``Pb = P[perm]`` unless given (pygda/nn/mixup_base.py:146-196)."""

    @staticmethod
    def forward(ctx, P, Pb, CC, bias, perm, inv, lam, p, first):
        P, CC, bias = _f32c(P, "P"), _f32c(CC, "CC"), _f32c(bias, "bias")
        if Pb is not None:
            Pb = _f32c(Pb, "Pb")
        n, h = P.shape
        if CC.shape != ((n, h) if first else (2 * n, h)):
            raise ValueError(f"centre projections must be {'[n, h]' if first else '[2n, h]'}, got {tuple(CC.shape)}")
        XX = torch.empty(2 * n, h, dtype=torch.float32, device=P.device)
        mask = torch.empty(n, h, dtype=torch.uint8, device=P.device)
        _lib.call("gda_mixup_combine_fwd_f32", P, Pb, CC, int(first), bias, perm, n, h, float(lam), float(p),
                  *dropout_state.generator(P.device, sites=2), XX, mask, _lib.stream())
        ctx.save_for_backward(XX, mask, inv)
        ctx.cfg = (float(lam), float(p), bool(first), Pb is not None)
        return XX

    @staticmethod
    def backward(ctx, gXX):
        XX, mask, inv = ctx.saved_tensors
        lam, p, first, sep = ctx.cfg
        n, h = mask.shape
        gXX = gXX.contiguous()
        f32 = dict(dtype=torch.float32, device=gXX.device)
        gP = torch.empty(n, h, **f32)
        gPb = torch.empty(n, h, **f32) if sep else None
        gCC = torch.empty(n if first else 2 * n, h, **f32)
        gb = torch.empty(h, **f32)
        ws, nbytes = _lib.scratch("gda_mixup_combine_workspace_bytes", gXX.device, "mixup", n, h)
        _lib.call("gda_mixup_combine_bwd_f32", gXX, XX, mask, inv, int(first), n, h, lam, p, gP, gPb, gCC, gb, ws,
                  nbytes, _lib.stream())
        return gP, gPb, gCC, gb, None, None, None, None, None


def mixup_combine_ok(P, h):
    return P.is_cuda and P.dtype == torch.float32 and h % 4 == 0 and h <= 1024


def mixup_combine(P, Pb, CC, bias, perm, inv, lam, p, training, first):
    """One mixup layer's epilogue -> the stacked pair ``[x' ; x_mix']`` ``[2n, h]``.  ``perm`` / ``inv`` are
    int64 device vectors (new position -> old node and its inverse)."""
    return _MixupCombine.apply(P, Pb, CC, bias, perm, inv, float(lam), float(p) if training else 0.0, bool(first))


# ------------------------------------------------- Laplacian smoothness (TDSS) --
class _Laplacian(torch.autograd.Function):
    """``1/2 sum_e ||f[row] dinv[row] - f[col] dinv[col]||^2`` over the edges of ``graph`` (built
    with ``add_self_loops=False, normalize=False``: by-source CSR = rows of ``row`` nodes)."""

    @staticmethod
    def forward(ctx, feats, graph):
        f = _f32c(feats, "features")
        n, d = f.shape
        if n != graph.num_nodes:
            raise ValueError(f"features must have num_nodes={graph.num_nodes} rows, got {n}")
        dev = f.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dinv = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        ws, _ = _lib.scratch("gda_laplacian_workspace_bytes", dev, "laplacian", n)
        nnz = graph.nnz if profiler.enabled else 0
        with profiler.region(f"laplacian_fwd[d={d}]", 1, nnz * 4 + n * (d * 4 + 12), 3 * nnz * d):
            _lib.call("gda_laplacian_fwd_f32", graph.t_rowptr, graph.t_colidx, n, d, f, d, loss, dinv, ws, ws.numel(),
                      _lib.stream())
        ctx.graph = graph
        ctx.save_for_backward(f, dinv)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        f, dinv = ctx.saved_tensors
        g = ctx.graph
        n, d = f.shape
        gf = torch.empty_like(f)
        gl = gl.reshape(1).to(torch.float32).contiguous()
        nnz = g.nnz if profiler.enabled else 0
        with profiler.region(f"laplacian_bwd[d={d}]", 1, nnz * 8 + 2 * n * d * 4, 4 * nnz * d):
            _lib.call("gda_laplacian_bwd_f32", g.t_rowptr, g.t_colidx, g.rowptr, g.colidx, n, d, f, d, dinv, gl, gf, d,
                      _lib.stream())
        return gf, None


def laplacian_loss(features, edge_index):
    """TDSS.compute_laplacian_loss (pygda/models/tdss.py:390-454).  ``edge_index`` is the
    ``[2, E]`` smoothing edge list (ingested once, cached by identity) or a ready
    :class:`~pygda_amd.graph.CSRGraph` built with ``add_self_loops=False, normalize=False``."""
    from .graph import as_graph
    graph = as_graph(edge_index, features.size(0), None, False, False, False, "col")
    return _Laplacian.apply(features, graph)


# ------------------------------------------- polynomial graph filters (DGSDA BernProp) --
def spmm_axpby(graph: CSRGraph, x, alpha, beta, z=None, gamma=1.0, gamma_dev=None, transposed=False, out=None):
    """``alpha * x + beta * (A x) + gamma * z`` in one aggregation launch (no autograd).
    ``gamma_dev``: one-element device tensor multiplied into ``gamma`` (a learnable coefficient);
    ``out``: contiguous ``[n, d]`` fp32 destination (e.g. a slice of a chain buffer)."""
    x = _f32c(x, "x")
    if x.dim() != 2 or x.size(0) != graph.num_nodes:
        raise ValueError(f"x must be [num_nodes={graph.num_nodes}, d], got {tuple(x.shape)}")
    rp, ci, va = (graph.t_rowptr, graph.t_colidx, graph.t_val) if transposed else \
                 (graph.rowptr, graph.colidx, graph.val)
    n, d = x.shape
    if z is not None:
        z = _f32c(z, "z")
        if z.shape != x.shape:
            raise ValueError("z must have the shape of x")
    if out is None:
        y = torch.empty_like(x)
    else:
        y = out
        if y.shape != x.shape or y.dtype != torch.float32 or not y.is_contiguous() or y.device != x.device:
            raise ValueError("out must be a contiguous fp32 tensor of the shape of x on its device")
    if aggregation_log is not None:
        aggregation_log.append((_logged(graph), 1))
    if profiler.enabled:
        global aggregated_edges
        aggregated_edges += graph.nnz
        ctx = profiler.region(f"spmm_csr_axpby_f32[d={d}]", 1,
                              graph.nnz * 8 + (n + 1) * 4 + (2 + (z is not None)) * n * d * 4, 2 * graph.nnz * d)
    else:
        ctx = profiler.region("", 0)
    sp = graph.split(transposed).struct(d)
    with ctx:
        _lib.call("gda_spmm_csr_axpby_f32", rp, ci, va, n, d, x, d, y, d, float(alpha), float(beta), z, d, float(gamma),
                  gamma_dev, ctypes.byref(sp) if sp is not None else None, _lib.stream())
    return y


class _BernFilter(torch.autograd.Function):
    """``out = sum_k w_k (I + A)^(K-k) (I - A)^k x`` with ``w = relu(temp) * binom(K, k) / 2^K``: the
    Bernstein-basis filter of BernProp.forward (pygda/nn/dgsda_base.py:101-151), where
    L = I - A and 2I - L = I + A for the self-loop-free symmetric normalisation A.

    The reference spends K + K(K+1)/2 propagations forward (and as many again in autograd).  L and
    2I - L commute, so the same polynomial is evaluated as one chain v_k = L^k x and one Horner
    sweep s_j = (I + A) s_{j-1} + w_j v_j: 2K launches forward, 2K backward (adjoint chain
    q_j = (I + A^T)^j g, Horner in (I - A^T)), the accumulation riding in the SpMM epilogue and the
    coefficients read from device memory.  Every term is a product of positive semi-definite
    factors with non-negative weights, so the reordering costs rounding only (tested at 1e-5)."""

    @staticmethod
    def forward(ctx, x, temp, graph, coefs):
        K = temp.numel() - 1
        w = (torch.relu(temp.detach()) * coefs).contiguous()
        x = _f32c(x.detach(), "x")
        v = torch.empty((K + 1,) + tuple(x.shape), dtype=torch.float32, device=x.device)   # the chain L^k x
        v[0].copy_(x)
        for k in range(1, K + 1):
            spmm_axpby(graph, v[k - 1], 1.0, -1.0, out=v[k])
        s = v[0] * w[0]
        for j in range(1, K + 1):
            s = spmm_axpby(graph, s, 1.0, 1.0, z=v[j], gamma=1.0, gamma_dev=w[j:j + 1])
        ctx.graph, ctx.K = graph, K
        ctx.save_for_backward(temp, coefs, w, v)
        return s

    @staticmethod
    def backward(ctx, g):
        temp, coefs, w, v = ctx.saved_tensors
        graph, K = ctx.graph, ctx.K
        q = torch.empty_like(v)                     # q[K - j] = (I + A^T)^j g: slot k pairs with v[k]
        q[K].copy_(g)
        for j in range(1, K + 1):
            spmm_axpby(graph, q[K - j + 1], 1.0, 1.0, transposed=True, out=q[K - j])
        g_temp = None
        if ctx.needs_input_grad[1]:                 # <(I+A^T)^(K-k) g, L^k x> for all k at once
            dots = (q.view(K + 1, -1) * v.view(K + 1, -1)).sum(dim=1)
            g_temp = dots * coefs * (temp > 0).to(dots.dtype)
        g_x = None
        if ctx.needs_input_grad[0]:
            t = q[K] * w[K]
            for j in range(1, K + 1):
                t = spmm_axpby(graph, t, 1.0, -1.0, z=q[K - j], gamma=1.0, gamma_dev=w[K - j:K - j + 1],
                               transposed=True)
            g_x = t
        return g_x, g_temp, None, None


def bern_filter(x, temp, graph: CSRGraph, coefs):
    return _BernFilter.apply(x, temp, graph, coefs)


# ------------------------------------------------- view attention (UDAGCN's dual-view encoder) --
class _AttentionFuse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, b, *views):
        xs = [_f32c(v, "view") for v in views]
        n, h = xs[0].shape
        K = len(xs)
        w1 = _f32c(w, "dense_weight.weight").reshape(-1)
        b1 = _f32c(b, "dense_weight.bias").reshape(-1)
        out = torch.empty(n, h, dtype=torch.float32, device=xs[0].device)
        att = torch.empty(n, K, dtype=torch.float32, device=xs[0].device)
        ptrs = (ctypes.c_void_p * K)(*[x.data_ptr() for x in xs])
        lds = (ctypes.c_int64 * K)(*[h] * K)
        _lib.call("gda_attention_fuse_fwd_f32", K, ptrs, lds, n, h, w1, b1, out, h, att, _lib.stream())
        ctx.save_for_backward(w1, att, *xs)
        ctx.w_shape, ctx.b_shape = w.shape, b.shape
        return out

    @staticmethod
    def backward(ctx, g):
        w1, att, *xs = ctx.saved_tensors
        n, h = xs[0].shape
        K = len(xs)
        g = _f32c(g, "grad")
        gxs = [torch.empty_like(x) if ctx.needs_input_grad[2 + k] else None for k, x in enumerate(xs)]
        gw = torch.empty(h, dtype=torch.float32, device=g.device)
        gb = torch.empty(1, dtype=torch.float32, device=g.device)
        ws, _ = _lib.scratch("gda_attention_workspace_bytes", g.device, "attention", n, h)
        ptrs = (ctypes.c_void_p * K)(*[x.data_ptr() for x in xs])
        gptrs = (ctypes.c_void_p * K)(*[None if t is None else t.data_ptr() for t in gxs])
        lds = (ctypes.c_int64 * K)(*[h] * K)
        _lib.call("gda_attention_fuse_bwd_f32", K, ptrs, lds, n, h, w1, att, g, h, gptrs, gw, gb, ws,
                  ws.numel() if ws is not None else 0, _lib.stream())
        return (gw.view(ctx.w_shape), gb.view(ctx.b_shape), *gxs)


def attention_fuse_ok(views, w):
    """Shapes the fused view-attention kernels cover (csrc/gda_attention.hip)."""
    if not (2 <= len(views) <= 4):
        return False
    v0 = views[0]
    return (all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float32 and v.dim() == 2 and v.shape == v0.shape
                for v in views) and v0.size(1) % 4 == 0 and 0 < v0.size(1) <= 512 and w.numel() == v0.size(1))


def attention_fuse(views, w, b):
    """``sum(stack(views, 1) * softmax(Linear(h, 1)(stack(views, 1)), 1), 1)`` (pygda/nn/attention.py:51-54), fused."""
    return _AttentionFuse.apply(w, b, *views)



# ------------------------------------------------- FAConv aggregation (SAGDA's SAGNN layer) --
def faconv_bytes(n, nnz, d):
    """Algorithmic bytes of the FAConv forward and backward (csrc/gda_faconv.hip) at ``n`` rows, ``nnz`` CSR entries
    (self loops included) and width ``d``: every index, weight and per-edge scalar once, one ``d``-wide row gathered
    per entry, the dense rows read or written once."""
    fwd = 4 * (n + 1) + nnz * (4 + 4 + 4 + 4) + 4 * n + 4 * nnz * d + 4 * n * d * 2
    bwd_dst = 4 * (n + 1) + nnz * (4 + 4 + 4 + 4) + 4 * nnz * d + 4 * n * d + 4 * n
    bwd_src = 4 * (n + 1) + nnz * (4 + 4 + 4 + 4 + 4) + 4 * nnz * d + 4 * n * d * 2 + 4 * n
    return fwd, bwd_dst + bwd_src


class _FAConvAggregate(torch.autograd.Function):
    """``out = A_att h + eps h + bias``, ``A_att[i, j] = tanh(s_j + r_i) w_ij`` over the FAConv graph (gcn_norm with
    remaining self loops and the destination degree, plus the edge map), on csrc/gda_faconv.hip.  With ``s is None``
    ``p`` is the packed projection ``[h | s | r]`` (``[n, >= d + 2]``: s = column d, r = column d + 1) and the gradient
    comes back packed the same way, one tensor; otherwise ``p`` is ``h`` and the three gradients come back apart."""

    @staticmethod
    def forward(ctx, p, s, r, d, graph, eps, bias):
        _lib.require_gpu_tensor(p, "h")
        if p.dtype != torch.float32 or p.dim() != 2:
            raise _lib.GdaError(f"faconv_aggregate: h must be a 2-D fp32 tensor, got {p.dtype} {tuple(p.shape)}")
        if p.stride(1) != 1:
            p = p.contiguous()
        n = p.size(0)
        if n != graph.num_nodes or graph.t_to_fwd is None:
            raise _lib.GdaError("faconv_aggregate: the graph must have one row per node and its edge map")
        packed = s is None
        if packed:
            if p.size(1) < d + 2:
                raise _lib.GdaError(f"faconv_aggregate: a packed projection needs d + 2 = {d + 2} columns")
            sp, rp, ldsr = p.data_ptr() + 4 * d, p.data_ptr() + 4 * (d + 1), p.stride(0)
        else:
            s, r = _f32c(s.reshape(-1), "s"), _f32c(r.reshape(-1), "r")
            if s.numel() != n or r.numel() != n or p.size(1) != d:
                raise _lib.GdaError("faconv_aggregate: h [n, d], s [n], r [n] expected")
            sp, rp, ldsr = s.data_ptr(), r.data_ptr(), 1
        b = None if bias is None else _f32c(bias, "bias")
        out = torch.empty(n, d, dtype=torch.float32, device=p.device)
        t = torch.empty(max(graph.nnz_cap, 1), dtype=torch.float32, device=p.device)
        with profiler.region("faconv_fwd", 1, faconv_bytes(n, graph.nnz, d)[0] if profiler.enabled else 0):
            _lib.call("gda_faconv_fwd_f32", graph.rowptr, graph.colidx, graph.val, n, d, p, p.stride(0), sp, rp, ldsr,
                      float(eps), b, out, d, t, _lib.stream())
        ctx.save_for_backward(p, t)
        ctx.graph, ctx.eps, ctx.d, ctx.packed, ctx.has_bias = graph, float(eps), int(d), packed, b is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        p, t = ctx.saved_tensors
        g, d = ctx.graph, ctx.d
        n = p.size(0)
        gout = gout.contiguous()
        if ctx.packed:
            width = p.size(1)
            gp = (torch.empty if width == d + 2 else torch.zeros)(n, width, dtype=torch.float32, device=p.device)
            ghp, gsp, grp, ldgh, ldgsr = gp.data_ptr(), gp.data_ptr() + 4 * d, gp.data_ptr() + 4 * (d + 1), width, width
        else:
            gh = torch.empty(n, d, dtype=torch.float32, device=p.device)
            gs = torch.empty(n, dtype=torch.float32, device=p.device)
            gr = torch.empty(n, dtype=torch.float32, device=p.device)
            ghp, gsp, grp, ldgh, ldgsr = gh.data_ptr(), gs.data_ptr(), gr.data_ptr(), d, 1
        dpre = torch.empty_like(t)
        with profiler.region("faconv_bwd", 2, faconv_bytes(n, g.nnz, d)[1] if profiler.enabled else 0):
            _lib.call("gda_faconv_bwd_f32", g.rowptr, g.colidx, g.val, g.t_rowptr, g.t_colidx, g.t_to_fwd, n, d, p,
                      p.stride(0), t, gout, d, ctx.eps, ghp, ldgh, gsp, grp, ldgsr, dpre, _lib.stream())
        gb = colsum(gout) if ctx.has_bias and ctx.needs_input_grad[6] else None
        if ctx.packed:
            return gp, None, None, None, None, None, gb
        return gh, gs, gr, None, None, None, gb


def faconv_aggregate(h, s, r, graph, eps, bias=None):
    """FAConv's aggregation on a projected input (pygda/nn/sagda_base.py:87-88 reassociated): ``out_i = sum_k tanh(s[j_k]
    + r_i) w_k h[j_k] + eps h_i + bias`` over the entries of row i of ``graph`` (``nn.sagda_base.faconv_graph``).
    ``h [n, d]``, ``s [n]``, ``r [n]``; differentiable in all three and in ``bias``."""
    return _FAConvAggregate.apply(h, s, r, h.size(1), graph, eps, bias)


def faconv_aggregate_packed(p, d, graph, eps, bias=None):
    """Same, on the packed projection ``p = [h | s | r]`` (``[n, d + 2]``): the gradient is one ``[n, d + 2]`` tensor,
    what the projection's own backward takes -- no slicing of three gradients back together."""
    return _FAConvAggregate.apply(p, None, None, int(d), graph, eps, bias)


# ------------------------------------------------- CWGCN's losses (csrc/gda_cwgcn.hip) --
def _cwgcn_rows(x, name):
    _lib.require_gpu_tensor(x, name)
    if x.dtype != torch.float32 or x.dim() != 2 or x.size(0) < 1 or x.size(1) < 1:
        raise _lib.GdaError(f"{name}: a non-empty 2-D fp32 tensor expected, got {x.dtype} {tuple(x.shape)}")
    return x if x.stride(1) == 1 else x.contiguous()


def cwgcn_bytes(n, c, d):
    """Algorithmic bytes of CWGCN's kernels at ``n`` rows, ``c`` classes and hidden width ``d``: (c_loss forward,
    c_loss backward, weighted moments, matching forward, matching backward).  Every input read once (the statistics
    kernels read x twice by design: the second pass is counted), every output written once."""
    closs_f = 4 * n * c + 8 * n + 4 * n * 2 + 4
    closs_b = 4 * n * c + 8 * n + 4 * n + 4 * n * c + 4
    moments = 2 * (4 * n * d + 4 * n) + 4 * 2 * d
    match_f = 2 * 4 * n * d + 4 * 2 * d + 4 * 4 * d + 4
    match_b = 4 * n * d + 4 * 3 * d + 4 * n * d + 4
    return closs_f, closs_b, moments, match_f, match_b


class _CorrentropyLoss(torch.autograd.Function):
    """gda_closs_{fwd,bwd}_f32: ``(mean_i(1 - exp(-d_i / 100)), exp(-d / 10))``, ``d_i = |z_i - onehot(y_i)|^2``."""

    @staticmethod
    def forward(ctx, z, y):
        z = _cwgcn_rows(z, "logits")
        _lib.require_gpu_tensor(y, "labels", torch.int64)
        y = y.contiguous()
        n, c = z.shape
        if y.dim() != 1 or y.numel() != n:
            raise _lib.GdaError(f"correntropy_loss: {n} labels expected, got {tuple(y.shape)}")
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        weight = torch.empty(n, dtype=torch.float32, device=z.device)
        factor = torch.empty(n, dtype=torch.float32, device=z.device)
        ws, nbytes = _lib.scratch("gda_closs_workspace_bytes", z.device, "closs", n, c)
        launches = 1 if nbytes <= 4 else 2          # one workgroup's partial sum is the result (gda_cwgcn.hip)
        with profiler.region("closs_fwd", launches, cwgcn_bytes(n, c, 0)[0] if profiler.enabled else 0):
            _lib.call("gda_closs_fwd_f32", z, z.stride(0), y, n, c, loss, weight, factor, ws, nbytes, _lib.stream())
        ctx.save_for_backward(z, y, factor)
        ctx.mark_non_differentiable(weight)
        return loss, weight

    @staticmethod
    def backward(ctx, gloss, _gweight):
        z, y, factor = ctx.saved_tensors
        n, c = z.shape
        gloss = gloss.contiguous()
        gz = torch.empty(n, c, dtype=torch.float32, device=z.device)
        with profiler.region("closs_bwd", 1, cwgcn_bytes(n, c, 0)[1] if profiler.enabled else 0):
            _lib.call("gda_closs_bwd_f32", z, z.stride(0), y, factor, gloss, n, c, gz, c, _lib.stream())
        return gz, None


def correntropy_loss(logits, labels):
    """CWGCNBase.c_loss (pygda/nn/cwgcn_base.py:193-219): ``(loss, weight)`` with ``d_i = sum_c (z_ic - onehot_ic)^2``,
    ``loss = mean(1 - exp(-d / 100))``, ``weight = exp(-d / 10)`` (not differentiable).  Host tensors: the
    reference's torch lines, which raise when ``max(labels) + 1`` is not the logits' width."""
    if logits.is_cuda:
        return _CorrentropyLoss.apply(logits, labels)
    import torch.nn.functional as F
    onehot = F.one_hot(labels).to(logits.device)
    distance = torch.sum(torch.square(logits - onehot), dim=1)
    loss = torch.mean(1 - torch.exp(torch.div(-distance, 100)))
    return loss, torch.exp(torch.div(-distance, 10)).detach()


def weighted_moments(x, w, out=None):
    """CWGCN.get_src_mean_std (pygda/models/cwgcn.py:423-458), detached: ``w' = w / sum w``, ``mean = sum w' x``,
    ``std = sqrt(sum w' (x - mean)^2 / (1 - sum w'^2))`` per column of ``x [n, d]``.  ``out = (mean, std)``: device
    buffers written in place (a captured step keeps its source statistics there)."""
    x, w = x.detach(), w.detach()
    if not x.is_cuda:
        sum_w = torch.sum(w)
        wn = w.view(-1, 1) * (1 / sum_w)
        mean = torch.sum(x * wn, dim=0)
        var = torch.sum(torch.pow(x - mean, 2) * wn, dim=0)
        std = torch.pow(var / (1 - torch.sum(torch.pow(wn, 2))), 1 / 2)
        if out is not None:
            out[0].copy_(mean)
            out[1].copy_(std)
            return out
        return mean, std
    x = _cwgcn_rows(x, "x")
    _lib.require_gpu_tensor(w, "weight", torch.float32)
    n, d = x.shape
    w = w.contiguous()
    if w.numel() != n:
        raise _lib.GdaError(f"weighted_moments: {n} weights expected, got {w.numel()}")
    if out is None:
        out = (torch.empty(d, dtype=torch.float32, device=x.device), torch.empty(d, dtype=torch.float32, device=x.device))
    mean, std = out
    if not (mean.is_contiguous() and std.is_contiguous() and mean.numel() == d and std.numel() == d):
        raise _lib.GdaError("weighted_moments: out must be two contiguous [d] buffers")
    ws, nbytes = _lib.scratch("gda_colstats_workspace_bytes", x.device, "colstats", n, d)
    with profiler.region("weighted_moments", 2, cwgcn_bytes(n, 0, d)[2] if profiler.enabled else 0):
        _lib.call("gda_weighted_moments_f32", x, x.stride(0), w, n, d, mean, std, ws, nbytes, _lib.stream())
    return out


class _StdMeanMatch(torch.autograd.Function):
    """gda_std_mean_match_{fwd,bwd}_f32: ``sum (mean_s - mean_t)^2 + sum (std_s - std_t)^2`` with
    ``std_t, mean_t = torch.std_mean(x, dim=0)``; differentiable in ``x`` only."""

    @staticmethod
    def forward(ctx, x, mean_s, std_s):
        x = _cwgcn_rows(x, "x")
        n, d = x.shape
        mean_s, std_s = _f32c(mean_s.detach().reshape(-1), "mean_s"), _f32c(std_s.detach().reshape(-1), "std_s")
        if mean_s.numel() != d or std_s.numel() != d:
            raise _lib.GdaError(f"std_mean_match: source statistics of width {d} expected")
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        stats = torch.empty(4, d, dtype=torch.float32, device=x.device)     # mean_t, std_t, coef (2 rows)
        ws, nbytes = _lib.scratch("gda_colstats_workspace_bytes", x.device, "colstats", n, d)
        with profiler.region("match_fwd", 3, cwgcn_bytes(n, 0, d)[3] if profiler.enabled else 0):
            _lib.call("gda_std_mean_match_fwd_f32", x, x.stride(0), n, d, mean_s, std_s, loss, stats[0], stats[1],
                      stats[2], ws, nbytes, _lib.stream())
        ctx.save_for_backward(x, stats)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        x, stats = ctx.saved_tensors
        n, d = x.shape
        gloss = gloss.contiguous()
        gx = torch.empty(n, d, dtype=torch.float32, device=x.device)
        with profiler.region("match_bwd", 1, cwgcn_bytes(n, 0, d)[4] if profiler.enabled else 0):
            _lib.call("gda_std_mean_match_bwd_f32", x, x.stride(0), n, d, stats[0], stats[2], gloss, gx, d,
                      _lib.stream())
        return gx, None, None


def std_mean_match(x, mean_s, std_s):
    """The stage-2 loss of CWGCN (pygda/models/cwgcn.py:327-328): ``std_t, mean_t = torch.std_mean(x, dim=0)``
    (unbiased), ``sum (mean_s - mean_t)^2 + sum (std_s - std_t)^2`` with the source statistics detached."""
    if x.is_cuda:
        return _StdMeanMatch.apply(x, mean_s, std_s)
    std_t, mean_t = torch.std_mean(x, dim=0)
    return torch.sum(torch.square(mean_s.detach() - mean_t)) + torch.sum(torch.square(std_s.detach() - std_t))


# ---------------------------------------------------- ACDNE: PPMI preprocessing and step losses (csrc/gda_acdne.hip) --
ACDNE_MEMORY_FRACTION = 0.9       # process_graph's buffers must fit under this share of the device's free memory
ACDNE_MAX_HALF = 128              # GDA_ACDNE_MAX_HALF: rows per domain in one step


def acdne_bytes(n, nnz, f, xnnz, h, e, c, step=3):
    """Algorithmic bytes of ACDNE's kernels: (PPMI of an n-node graph with nnz coalesced edges at ``step``, X_nei with
    ``xnnz`` feature non-zeros and f features, the proximity loss of 2h rows of width e, the heads with c classes).
    Dense N x N passes are counted once per read or write; the powers read a_{k-1} once per edge."""
    nn_ = 4 * n * n
    ppmi = (12 * nnz + 2 * nn_) + (step - 1) * (4 * nnz * n + 3 * nn_) + 2 * nn_ + 2 * nn_ + nn_ + 3 * nn_
    xnei = nn_ + 8 * xnnz + 4 * n * f                         # n_A_ppmi once, X's CSR, X_nei written
    prox = 2 * (4 * h * h + 8 * h + 4 * h * e) + 4 * 2 * h * e + 16
    heads = 4 * (2 * h * e) * 3 + 4 * (c * e + c + 128 * e + 128 + 128 * 128 + 128 + 2 * 128 + 2) * 2 + 8 * 2 * h
    return ppmi, xnei, prox, heads


def _count_csr(src, dst, n):
    """The adjacency ``adj[i, j]`` = number of edges i -> j (duplicates summed, to_dense_adj) as a coalesced CSR by
    source row: (rowptr int32 [n + 1], col int32, cnt fp32).  Index plumbing only."""
    key, cnt = torch.unique(src * n + dst, sorted=True, return_counts=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=src.device)
    rowptr[1:] = torch.cumsum(torch.bincount(key // n, minlength=n), 0)
    return rowptr.to(torch.int32), (key % n).to(torch.int32), cnt.to(torch.float32)


def _acdne_csr(edge_index, n):
    ei = edge_index.to(torch.int64)
    if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= n):
        raise ValueError(f"ACDNE: edge_index refers to nodes outside [0, {n})")
    return _count_csr(ei[0], ei[1], n)


def _row_scale(w):
    """my_scale_sim_mat's factors in fp32 numpy: ``1 / (row sum + 1e-12)``, 0 where that is infinite."""
    import numpy as np
    rowsum = np.array(np.sum(w, axis=1), dtype=np.float32)
    r_inv = np.power(rowsum + np.float32(1e-12), np.float32(-1)).flatten()
    r_inv[np.isinf(r_inv)] = 0.
    return r_inv


def _ppmi_dense(edge_index, n, step, dev, extra, who, what, region, f=None):
    """gda_acdne_ppmi_f32 on an n-node graph: ``(buf_a, buf_b)``, the PPMI and its row-scaled form, each
    [n, round_up(n, 4)].  Its dense buffers, its workspace and ``extra`` further bytes of the caller must fit under
    ACDNE_MEMORY_FRACTION of the free device memory, else MemoryError before any allocation."""
    ld = (n + 3) // 4 * 4
    ws_bytes = _lib.lib().gda_acdne_ppmi_workspace_bytes(n)
    need = (3 if step >= 3 else 2) * n * ld * 4 + ws_bytes + extra
    free = torch.cuda.mem_get_info(dev)[0]
    if need > ACDNE_MEMORY_FRACTION * free:
        raise MemoryError(f"{who}: process_graph on {n} nodes needs {need / 2**30:.2f} GiB of {what}, more than "
                          f"{ACDNE_MEMORY_FRACTION:.0%} of the {free / 2**30:.2f} GiB free on {dev}")
    rowptr, col, cnt = _acdne_csr(edge_index.to(dev), n)
    pval = torch.empty_like(cnt)
    buf_a = torch.empty(n, ld, dtype=torch.float32, device=dev)
    buf_b = torch.empty(n, ld, dtype=torch.float32, device=dev)
    buf_c = torch.empty(n, ld, dtype=torch.float32, device=dev) if step >= 3 else None
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    nbytes = acdne_bytes(n, cnt.numel(), f, 0, 1, 1, 1, step)[0] if f is not None and profiler.enabled else 0
    with profiler.region(region, 2 + step + 2, nbytes):
        _lib.call("gda_acdne_ppmi_f32", rowptr, col, cnt, n, step, pval, buf_a, buf_b, buf_c, ws, ws_bytes,
                  _lib.stream())
    return buf_a, buf_b


def _acdne_process_graph_host(edge_index, x, n, step):
    """pygda/models/acdne.py process_graph in fp32 throughout (the numpy 1.x semantics the reference was written for:
    ``a_k / k`` stays fp32), adjacency sized by ``n``."""
    import numpy as np
    ei = edge_index.detach().cpu().numpy()
    adj = np.zeros((n, n), dtype=np.float32)
    np.add.at(adj, (ei[0], ei[1]), np.float32(1))

    def scale(w):
        return (_row_scale(w)[:, None] * w).astype(np.float32)

    g = scale(adj)
    a_k, a = g, g
    for k in range(2, step + 1):
        a_k = np.matmul(a_k, g)
        a = a + a_k / np.float32(k)
    a = a.copy()
    np.fill_diagonal(a, 0)
    a = scale(a)
    col = np.sum(a, axis=0)
    col[col == 0] = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        ppmi = np.log((np.float32(n) * a) / col[None, :] + np.float32(1e-12))
    ppmi[np.isnan(ppmi)] = 0
    ppmi[ppmi < 0] = 0
    x_nei = np.matmul(scale(ppmi), x.detach().cpu().numpy().astype(np.float32))
    return torch.from_numpy(ppmi), torch.from_numpy(x_nei)


def acdne_process_graph(edge_index, x, n, step, out=None):
    """ACDNE.process_graph (pygda/models/acdne.py): ``(A_ppmi [n, n], X_nei [n, f])``.  GPU tensors: the PPMI on
    gda_acdne_ppmi_f32 (returned as a view of its [n, round_up(n, 4)] buffer) and ``X_nei = n_A_ppmi @ X`` on
    gda_acdne_xnei_f32 into ``out`` (a [n, f] row-contiguous view) when given.  The three dense N x N buffers and X_nei
    must fit under ACDNE_MEMORY_FRACTION of the free device memory, else MemoryError before any allocation.  Host
    tensors: the reference's numpy lines in fp32."""
    if not x.is_cuda:
        return _acdne_process_graph_host(edge_index, x, n, step)
    x = _f32c(x, "x")
    n, step, f = int(n), int(step), x.size(1)
    if x.size(0) != n or step < 1:
        raise ValueError(f"acdne_process_graph: x must have {n} rows and step >= 1")
    buf_a, buf_b = _ppmi_dense(edge_index, n, step, x.device, 0 if out is not None else n * f * 4, "ACDNE",
                               "dense N x N buffers and X_nei", "acdne_ppmi", f)
    ld = buf_b.stride(0)
    nz = x.nonzero()                                       # X as a row-major CSR (index plumbing)
    xval = x[nz[:, 0], nz[:, 1]].contiguous()
    xrp = torch.zeros(n + 1, dtype=torch.int64, device=x.device)
    xrp[1:] = torch.cumsum(torch.bincount(nz[:, 0], minlength=n), 0)
    xrp, xcol = xrp.to(torch.int32), nz[:, 1].to(torch.int32).contiguous()
    if out is None:
        out = torch.empty(n, f, dtype=torch.float32, device=x.device)
    if out.shape != (n, f) or out.stride(1) != 1:
        raise ValueError("acdne_process_graph: out must be a row-contiguous [n, f] view")
    with profiler.region("acdne_xnei", 1, acdne_bytes(n, 0, f, xval.numel(), 1, 1, 1, step)[1] if profiler.enabled else 0):
        _lib.call("gda_acdne_xnei_f32", buf_b, n, ld, xrp, xcol, xval, f, out, out.stride(0), _lib.stream())
    return buf_a[:, :n], out


def _batch_ppmi_host(ppmi_s, ppmi_t, pidx, h):
    """The reference's batch_ppmi (ACDNE's and DMGNN's alike): per domain the float64 block at the batch's PPMI indices
    with a zero diagonal, scaled by my_scale_sim_mat (the row sum rounded to float32).  Two float64 numpy blocks."""
    import numpy as np
    out = []
    for dom, P in enumerate((ppmi_s, ppmi_t)):
        ix = pidx[dom * h:(dom + 1) * h].cpu().numpy()
        blk = P.detach().cpu().numpy()[np.ix_(ix, ix)].astype(np.float64)
        np.fill_diagonal(blk, 0)
        out.append(_row_scale(blk).astype(np.float64)[:, None] * blk)
    return out


def _acdne_prox_host(ppmi_s, ppmi_t, pidx, z, h, pair_weight):
    """The reference's lines: batch_ppmi (float64 blocks) and net_pro_loss of each domain."""
    emb = torch.relu(z.detach()).requires_grad_(True)
    losses = []
    for dom, blk in enumerate(_batch_ppmi_host(ppmi_s, ppmi_t, pidx, h)):
        a = torch.tensor(blk)
        e = emb[dom * h:(dom + 1) * h]
        r = torch.sum(e * e, 1).reshape(-1, 1)
        dis = r - 2 * torch.matmul(e, e.T) + r.T
        losses.append(torch.mean(torch.sum(a * dis, 1)))
    total = pair_weight * (losses[0] + losses[1])
    (g,) = torch.autograd.grad(total, emb)
    return torch.stack([l.detach() for l in losses]), g.to(torch.float32)


def acdne_prox(ppmi_s, ppmi_t, pidx, z, h, pair_weight):
    """ACDNE's proximity loss of one step (pygda/models/acdne.py batch_ppmi, acdne_base.py net_pro_loss) on the 2h rows
    of ``z`` (the embedding before its ReLU): ``(losses [2] float64 -- source, target; unscaled --, gemb [2h, e] =
    pair_weight * d(ls + lt)/d emb)``.  ``pidx`` (int64 [2h]) holds the PPMI row of each batch row."""
    h = int(h)
    if not z.is_cuda:
        return _acdne_prox_host(ppmi_s, ppmi_t, pidx, z, h, pair_weight)
    z = _f32c(z, "z")
    _lib.require_gpu_tensor(pidx, "pidx", torch.int64)
    e = z.size(1)
    if z.size(0) != 2 * h or pidx.numel() != 2 * h or not 1 <= h <= ACDNE_MAX_HALF:
        raise _lib.GdaError(f"acdne_prox: 2h = {2 * h} rows (h <= {ACDNE_MAX_HALF}) expected")
    for P in (ppmi_s, ppmi_t):
        if P.dtype != torch.float32 or P.stride(1) != 1 or P.size(0) != P.size(1):
            raise _lib.GdaError("acdne_prox: square fp32 row-contiguous PPMI matrices expected")
    loss = torch.empty(2, dtype=torch.float64, device=z.device)
    gz = torch.empty_like(z)
    ws, nbytes = _lib.scratch("gda_acdne_prox_workspace_bytes", z.device, "acdne_prox", h)
    with profiler.region("acdne_prox", 3, acdne_bytes(1, 0, 0, 0, h, e, 0)[2] if profiler.enabled else 0):
        _lib.call("gda_acdne_prox_f32", ppmi_s, ppmi_s.stride(0), ppmi_s.size(0), ppmi_t, ppmi_t.stride(0),
                  ppmi_t.size(0), pidx, z, h, e, pair_weight, loss, gz, ws, nbytes, _lib.stream())
    return loss, gz


def _heads_host(z, gprox, a_blocks, params, y, rows, alpha, prox, pair_weight):
    """The reference's lines: the logits (DMGNN: of each half with ``a @ logits`` added), the classifier CE against
    float64 one-hot rows of the source half, GradReverse(alpha) into the discriminator with the domain CE, and the three
    losses summed; gradients by autograd."""
    import torch.nn.functional as F
    leaves = [p.detach().requires_grad_(True) for p in params]
    Wc, bc, W1, b1, W2, b2, W3, b3 = leaves
    z = z.detach().requires_grad_(True)
    h = z.size(0) // 2
    emb = torch.relu(z)
    emb_r = emb.detach().requires_grad_(True)                  # the discriminator's side of GradReverse
    logit = F.linear(emb, Wc, bc)
    if a_blocks is not None:
        logit = logit + torch.cat((torch.mm(a_blocks[0], logit[:h]), torch.mm(a_blocks[1], logit[h:])), dim=0)
    clf = F.cross_entropy(logit[:h], F.one_hot(y[rows[:h]], Wc.size(0)).double())
    d = F.linear(F.relu(F.linear(F.relu(F.linear(emb_r, W1, b1)), W2, b2)), W3, b3)
    dom = F.cross_entropy(d, torch.cat([torch.zeros(h, dtype=torch.int64), torch.ones(z.size(0) - h, dtype=torch.int64)]))
    total = clf + dom + pair_weight * (prox[0] + prox[1])
    g = torch.autograd.grad(clf + dom, [emb, emb_r] + leaves)
    ge = g[0] + g[1].neg() * float(alpha) + gprox
    dz = ge * (z.detach() > 0)
    return total.detach(), dz.to(torch.float32), [t.to(torch.float32) for t in g[2:]]


def _heads(z, gprox, a_blocks, params, y, rows, alpha, prox, pair_weight, loss_acc, out):
    """:func:`acdne_heads` (``a_blocks`` None) and :func:`dmgnn_heads`: one kernel, run with or without the blocks."""
    if not z.is_cuda:
        return _heads_host(z, gprox, a_blocks, params, y, rows, alpha, prox, pair_weight)
    name = "acdne_heads" if a_blocks is None else "dmgnn_heads"
    z, gprox = _f32c(z, "z"), _f32c(gprox, "gprox")
    blocks = () if a_blocks is None else (_f32c(a_blocks, "a_blocks"),)
    h, e = z.size(0) // 2, z.size(1)
    c = params[0].size(0)
    if z.size(0) != 2 * h or gprox.shape != z.shape or not 1 <= h <= ACDNE_MAX_HALF or params[2].shape != (128, e):
        raise _lib.GdaError(f"{name}: 2h rows (h <= 128), a 128-wide discriminator expected")
    if blocks and blocks[0].shape != (2, h, h):
        raise _lib.GdaError(f"{name}: a_blocks must be [2, {h}, {h}], got {tuple(a_blocks.shape)}")
    ws_params = [p.detach() for p in params]
    for p in ws_params:
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise _lib.GdaError(f"{name}: contiguous fp32 parameters expected")
    if out is None:
        out = (torch.empty_like(z), [torch.empty_like(p) for p in ws_params])
    dz, grads = out
    loss = torch.empty((), dtype=torch.float64, device=z.device)
    P8 = ctypes.c_void_p * 8
    ws, nbytes = _lib.scratch(f"gda_{name}_workspace_bytes", z.device, name, h, e, c)
    moved = dmgnn_bytes(1, 1, h, e, c)[1] if blocks else acdne_bytes(1, 0, 0, 0, h, e, c)[3]
    with profiler.region(name, 6, moved if profiler.enabled else 0):
        _lib.call(f"gda_{name}_f32", z, gprox, *blocks, h, e, c, P8(*[p.data_ptr() for p in ws_params]), y, y.numel(),
                  rows, alpha, prox, pair_weight, dz, P8(*[g.data_ptr() for g in grads]), loss, loss_acc, ws, nbytes,
                  _lib.stream())
    return loss, dz, grads


def acdne_heads(z, gprox, params, y, rows, alpha, prox, pair_weight, loss_acc=None, out=None):
    """ACDNE's heads over the step's 2h rows of ``z`` (the embedding before its ReLU), forward and backward in one launch
    (gda_acdne_heads_f32): ``(loss, dz, grads)`` with ``loss`` (float64, 0-dim) = clf + domain + pair_weight (ls + lt),
    ``dz`` the gradient of the whole step loss in ``z`` (``gprox`` added), ``grads`` the gradients of ``params`` =
    (Wc, bc, W1, b1, W2, b2, W3, b3).  The source labels are ``y[rows[:h]]``; ``alpha`` is a device scalar (GPU) or a
    float.  ``loss_acc`` (float64 [1], GPU) accumulates the loss; ``out = (dz, grads)`` are written in place."""
    return _heads(z, gprox, None, params, y, rows, alpha, prox, pair_weight, loss_acc, out)


def _predict_operands(z, weight, bias):
    return _f32c(z, "z"), _f32c(weight.detach(), "weight"), _f32c(bias.detach(), "bias")


def acdne_predict(z, weight, bias):
    """``softmax(relu(z) W^T + b)``: ACDNE.predict's probabilities (gda_acdne_predict_f32 on the GPU)."""
    if not z.is_cuda:
        import torch.nn.functional as F
        return F.softmax(F.linear(torch.relu(z), weight, bias), dim=1)
    z, w, b = _predict_operands(z, weight, bias)
    prob = torch.empty(z.size(0), w.size(0), dtype=torch.float32, device=z.device)
    _lib.call("gda_acdne_predict_f32", z, z.size(0), z.size(1), w, b, w.size(0), prob, _lib.stream())
    return prob


# --------------------------------------- DMGNN: neighbour-propagated step losses and predict (csrc/gda_dmgnn.hip) --
def dmgnn_bytes(n, ld, h, e, c):
    """Algorithmic bytes of DMGNN's kernels: (the proximity loss of 2h rows of width e, the heads with c classes,
    predict's ``P + M P`` over an n x n PPMI of leading dimension ld)."""
    prox = 2 * (2 * 4 * h * h + 8 * h + 4 * h * e) + 4 * 2 * h * e + 16
    heads = acdne_bytes(1, 0, 0, 0, h, e, c)[3] + 4 * h * h
    predict = 4 * n * ld + 4 * n * e + 4 * (c * e + c) + 4 * n * c
    return prox, heads, predict


def _dmgnn_prox_host(ppmi_s, ppmi_t, pidx, z, h, pair_weight):
    """The reference's lines: batch_ppmi (its blocks through ``torch.FloatTensor``: ``[2, h, h]`` float32) and
    nei_prox_loss (``norm(emb - a @ emb) / h``) of each domain."""
    a = torch.stack([torch.FloatTensor(blk) for blk in _batch_ppmi_host(ppmi_s, ppmi_t, pidx, h)])
    emb = torch.relu(z.detach()).requires_grad_(True)
    losses = []
    for dom in range(2):
        e = emb[dom * h:(dom + 1) * h]
        nei_emb = torch.mm(a[dom], e)
        losses.append(torch.norm(e - nei_emb) / e.shape[0])
    total = pair_weight * (losses[0] + losses[1])
    (g,) = torch.autograd.grad(total, emb)
    return torch.stack([l.detach() for l in losses]).double(), g.to(torch.float32), a


def dmgnn_prox(ppmi_s, ppmi_t, pidx, z, h, pair_weight):
    """DMGNN's proximity loss of one step (pygda/models/dmgnn.py batch_ppmi, nei_prox_loss) on the 2h rows of ``z`` (the
    embedding before its ReLU): ``(losses [2] float64 -- source, target; unscaled --, gemb [2h, e] = pair_weight *
    d(ls + lt)/d emb, a_blocks [2, h, h])``, the row-normalised PPMI blocks that :func:`dmgnn_heads` propagates the
    logits with.  ``pidx`` (int64 [2h]) holds the PPMI row of each batch row.  One launch (gda_dmgnn_prox_f32)."""
    h = int(h)
    if not z.is_cuda:
        return _dmgnn_prox_host(ppmi_s, ppmi_t, pidx, z, h, pair_weight)
    z = _f32c(z, "z")
    _lib.require_gpu_tensor(pidx, "pidx", torch.int64)
    e = z.size(1)
    if z.size(0) != 2 * h or pidx.numel() != 2 * h or not 1 <= h <= ACDNE_MAX_HALF:
        raise _lib.GdaError(f"dmgnn_prox: 2h = {2 * h} rows (h <= {ACDNE_MAX_HALF}) expected")
    for P in (ppmi_s, ppmi_t):
        if P.dim() != 2 or P.dtype != torch.float32 or P.stride(1) != 1 or P.size(0) != P.size(1):
            raise _lib.GdaError("dmgnn_prox: square fp32 row-contiguous PPMI matrices expected")
    loss = torch.empty(2, dtype=torch.float64, device=z.device)
    gz = torch.empty_like(z)
    a_blocks = torch.empty(2, h, h, dtype=torch.float32, device=z.device)
    ws, nbytes = _lib.scratch("gda_dmgnn_prox_workspace_bytes", z.device, "dmgnn_prox", h, e)
    with profiler.region("dmgnn_prox", 1, dmgnn_bytes(1, 1, h, e, 1)[0] if profiler.enabled else 0):
        _lib.call("gda_dmgnn_prox_f32", ppmi_s, ppmi_s.stride(0), ppmi_s.size(0), ppmi_t, ppmi_t.stride(0),
                  ppmi_t.size(0), pidx, z, h, e, pair_weight, loss, gz, a_blocks, ws, nbytes, _lib.stream())
    return loss, gz, a_blocks


def dmgnn_heads(z, gprox, a_blocks, params, y, rows, alpha, prox, pair_weight, loss_acc=None, out=None):
    """DMGNN's heads over the step's 2h rows of ``z``: :func:`acdne_heads` with the classifier logits of the source half
    propagated, ``L' = L + a_blocks[0] L``, before the cross-entropy, so that their gradient returns through
    ``I + a_blocks[0]^T`` (gda_dmgnn_heads_f32: the same kernel).  Same results and arguments as :func:`acdne_heads`
    otherwise; ``a_blocks [2, h, h]`` comes from :func:`dmgnn_prox`."""
    return _heads(z, gprox, a_blocks, params, y, rows, alpha, prox, pair_weight, loss_acc, out)


def dmgnn_predict(z, weight, bias, ppmi):
    """DMGNN.predict's output ``P + ppmi @ P`` with ``P = softmax(relu(z) W^T + b)`` over the rows of one domain and
    ``ppmi`` its dense [n, n] PPMI (gda_dmgnn_predict_f32 on the GPU: one streaming pass over ``ppmi``, which must be a
    view of a buffer whose rows are 16-byte aligned, as :func:`acdne_process_graph` returns it)."""
    if not z.is_cuda:
        probs = acdne_predict(z, weight, bias)
        return probs + torch.mm(ppmi, probs)
    z, w, b = _predict_operands(z, weight, bias)
    n, e, c = z.size(0), z.size(1), w.size(0)
    _lib.require_gpu_tensor(ppmi, "ppmi", torch.float32)
    if ppmi.dim() != 2 or ppmi.shape != (n, n) or ppmi.stride(1) != 1:
        raise _lib.GdaError(f"dmgnn_predict: a row-contiguous [{n}, {n}] PPMI expected, got {tuple(ppmi.shape)}")
    if ppmi.stride(0) % 4 or ppmi.data_ptr() % 16:
        raise _lib.GdaError("dmgnn_predict: the PPMI's rows must start on 16-byte boundaries (leading dimension a "
                            "multiple of 4, as acdne_process_graph returns it)")
    if w.size(1) != e or b.numel() != c:
        raise _lib.GdaError("dmgnn_predict: weight [c, e] and bias [c] expected")
    out = torch.empty(n, c, dtype=torch.float32, device=z.device)
    ws, nbytes = _lib.scratch("gda_dmgnn_predict_workspace_bytes", z.device, "dmgnn_predict", n, c)
    with profiler.region("dmgnn_predict", 2, dmgnn_bytes(n, ppmi.stride(0), 1, e, c)[2] if profiler.enabled else 0):
        _lib.call("gda_dmgnn_predict_f32", z, n, e, w, b, c, ppmi, ppmi.stride(0), out, ws, nbytes, _lib.stream())
    return out


# ---------------------------------------------- ASN: reconstruction, VAE row kernels, PPMI graph (csrc/gda_asn.hip) --
ASN_MAX_K = 128                   # GDA_ASN_MAX_K: decoder width of the reconstruction kernel
ASN_DIFF_MAX_K = 32               # DiffLoss widths of gda_asn_diff_*


class AsnLabels:
    """``adj_label = to_dense_adj(edge_index) + I`` of one domain as the coalesced CSR the reconstruction kernel walks
    (and its transpose), with the reference's ``pos_weight`` and ``norm`` (fp32 scalars, asn_base.py
    adj_label_for_reconstruction).  Index plumbing only."""

    def __init__(self, edge_index, n):
        ei = edge_index.to(torch.int64)
        n = int(n)
        E = ei.size(1)
        if E == 0 or int(ei.min()) < 0 or int(ei.max()) + 1 != n:
            raise ValueError(f"ASN: edge_index must span exactly the {n} nodes (to_dense_adj sizes the label matrix by "
                             "edge_index.max() + 1; the reference fails on a trailing isolated node)")
        self.n = n
        loops = torch.arange(n, device=ei.device, dtype=torch.int64)
        self.fwd = _count_csr(torch.cat([ei[0], loops]), torch.cat([ei[1], loops]), n)
        self.bwd = _count_csr(torch.cat([ei[1], loops]), torch.cat([ei[0], loops]), n)
        s = torch.tensor(float(E), dtype=torch.float32)                      # A.sum(): the edges, duplicates counted
        nn_ = n * n
        self.pos_weight = float((nn_ - s) / s)
        self.norm = float(nn_ / ((nn_ - s) * 2))

    def dense(self):
        """The dense label matrix (host tests and the host path only)."""
        rp, col, val = (t.cpu() for t in self.fwd)
        out = torch.zeros(self.n, self.n, dtype=torch.float32)
        rows = torch.repeat_interleave(torch.arange(self.n), (rp[1:] - rp[:-1]).to(torch.int64))
        out[rows, col.to(torch.int64)] = val
        return out


class _PairRecon(torch.autograd.Function):
    """The all-pairs reconstruction loss of csrc/gda_recon.h.  ``launch = (entry, tag, labels)``: the C call
    ``gda_<entry>_f32(z, ldz, n, k, *labels, loss, dz, lddz, workspace, bytes, stream)``, its workspace query
    ``gda_<entry>_workspace_bytes(n, k)`` and the workspace's cache entry ``tag``."""

    @staticmethod
    def forward(ctx, z, launch):
        entry, tag, labels = launch
        z = _f32c(z, "z")
        n, k = z.shape
        ws, nbytes = _lib.scratch(f"gda_{entry}_workspace_bytes", z.device, tag, n, k)
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z)
        with profiler.region(f"{entry}[{k}]", 3, 4 * n * k * 3, 4 * n * n * k):
            _lib.call(f"gda_{entry}_f32", z, k, n, k, *labels, loss, dz, k, ws, nbytes, _lib.stream())
        ctx.save_for_backward(dz)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return dz * g, None


def _asn_recon_host(z, labels):
    import torch.nn.functional as F
    preds = torch.mm(z, z.t())
    pw = torch.tensor([[labels.pos_weight]], dtype=torch.float32, device=z.device)
    return labels.norm * F.binary_cross_entropy_with_logits(preds, labels.dense().to(z.device), pos_weight=pw)


def asn_recon_loss(z, labels):
    """ASN's reconstruction cost ``norm * BCEWithLogits(z z^T, A + I, pos_weight)`` (asn_base.py recon_loss) for the
    decoder input ``z [N, K]`` (after its dropout) and the domain's :class:`AsnLabels`.  Device tensors: one pass over
    the pairs (gda_asn_recon_f32) that never forms the N x N matrix, K <= ASN_MAX_K (ValueError before any launch);
    host tensors: the reference's dense lines."""
    if not z.is_cuda:
        return _asn_recon_host(z, labels)
    if z.dim() != 2 or z.size(0) != labels.n:
        raise ValueError(f"asn_recon_loss: z must be [{labels.n}, K], got {tuple(z.shape)}")
    if not 1 <= z.size(1) <= ASN_MAX_K:
        raise ValueError(f"asn_recon_loss: the kernel covers 1 <= K <= {ASN_MAX_K}, got K = {z.size(1)}")
    return _PairRecon.apply(z, ("asn_recon", "asn_recon",
                                (*labels.fwd, *labels.bwd, labels.norm, labels.pos_weight)))


class _AsnKLD(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, lv, n_nodes):
        mu, lv = _f32c(mu, "mu"), _f32c(lv, "logvar")
        n, d = mu.shape
        ws, nbytes = _lib.scratch("gda_asn_rows_workspace_bytes", mu.device, "asn_rows", n, 1, 1)
        loss = torch.empty(1, dtype=torch.float32, device=mu.device)
        gmu, glv = torch.empty_like(mu), torch.empty_like(lv)
        _lib.call("gda_asn_kld_f32", mu, d, lv, d, n, d, float(n_nodes), loss, gmu, glv, ws, nbytes, _lib.stream())
        ctx.save_for_backward(gmu, glv)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        gmu, glv = ctx.saved_tensors
        return gmu * g, glv * g, None


def asn_kld(mu, logvar, n_nodes):
    """``-0.5 / n_nodes * mean(sum(1 + 2 logvar - mu^2 - exp(logvar)^2, 1))`` (asn_base.py recon_loss's KLD)."""
    if not mu.is_cuda:
        return -0.5 / n_nodes * torch.mean(torch.sum(1 + 2 * logvar - mu.pow(2) - logvar.exp().pow(2), 1))
    return _AsnKLD.apply(mu, logvar, n_nodes)


class _AsnReparam(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, lv, eps):
        mu, lv = _f32c(mu, "mu"), _f32c(lv, "logvar")
        n, d = mu.shape
        draw = eps is None
        if draw:
            eps = torch.empty_like(mu)
            seed, step, site = dropout_state.generator(mu.device)
        else:
            eps = _f32c(eps, "eps")
            seed, step, site = 0, None, 0
        z = torch.empty_like(mu)
        _lib.call("gda_asn_reparam_fwd_f32", mu, d, lv, d, n, d, eps, int(draw), seed, step, site, z, _lib.stream())
        ctx.save_for_backward(eps, lv)
        return z

    @staticmethod
    def backward(ctx, g):
        eps, lv = ctx.saved_tensors
        g = _f32c(g, "grad")
        n, d = g.shape
        glv = torch.empty_like(g)
        _lib.call("gda_asn_reparam_bwd_f32", g, eps, lv, d, n, d, glv, _lib.stream())
        return g, glv, None


def asn_reparam(mu, logvar, eps=None):
    """GNNVAE.reparameterize in training: ``eps * exp(logvar) + mu`` (exp of logvar, not of logvar / 2, as written).
    ``eps`` None draws standard normals (Philox on the device, ``torch.randn_like`` on the host)."""
    if not mu.is_cuda:
        if eps is None:
            eps = torch.randn_like(mu)
        return eps.mul(torch.exp(logvar)).add_(mu)
    return _AsnReparam.apply(mu, logvar, eps)


class _AsnDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        x = _f32c(x, "x")
        mask, y = torch.empty_like(x), torch.empty_like(x)
        _lib.call("gda_asn_dropout_fwd_f32", x, x.numel(), float(p), *dropout_state.generator(x.device), mask, y,
                  _lib.stream())
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        g = _f32c(g, "grad")
        gx = torch.empty_like(g)
        _lib.call("gda_asn_mask_mul_f32", g, mask, g.numel(), gx, _lib.stream())
        return gx, None


def asn_dropout(x, p):
    """``F.dropout(x, p)`` in training (the decoder's dropout; no ReLU in front of it)."""
    if not x.is_cuda:
        import torch.nn.functional as F
        return F.dropout(x, p, training=True)
    if p == 0:
        return x
    return _AsnDropout.apply(x, p)


class _AsnDiff(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32c(a, "input1"), _f32c(b, "input2")
        n, k1 = a.shape
        k2 = b.size(1)
        ws, nbytes = _lib.scratch("gda_asn_rows_workspace_bytes", a.device, "asn_rows", n, k1, k2)
        loss = torch.empty(1, dtype=torch.float32, device=a.device)
        gram = torch.empty(k1, k2, dtype=torch.float32, device=a.device)
        _lib.call("gda_asn_diff_fwd_f32", a, k1, b, k2, n, k1, k2, loss, gram, ws, nbytes, _lib.stream())
        ctx.save_for_backward(a, b, gram)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        a, b, gram = ctx.saved_tensors
        n, k1 = a.shape
        k2 = b.size(1)
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        g = g.reshape(1).to(torch.float32).contiguous()
        _lib.call("gda_asn_diff_bwd_f32", a, k1, b, k2, n, k1, k2, gram, g, ga, gb, _lib.stream())
        return ga, gb


def _asn_diff_host(input1, input2):
    n = input1.size(0)
    input1, input2 = input1.view(n, -1), input2.view(n, -1)
    n1 = torch.norm(input1, p=2, dim=1, keepdim=True).detach()
    a = input1.div(n1.expand_as(input1) + 1e-6)
    n2 = torch.norm(input2, p=2, dim=1, keepdim=True).detach()
    b = input2.div(n2.expand_as(input2) + 1e-6)
    return torch.mean((a.t().mm(b)).pow(2))


def asn_diff_loss(input1, input2):
    """DiffLoss (asn_base.py): ``mean((An^T Bn)^2)``, rows scaled by their detached L2 norm + 1e-6."""
    if not input1.is_cuda:
        return _asn_diff_host(input1, input2)
    if input1.size(1) > ASN_DIFF_MAX_K or input2.size(1) > ASN_DIFF_MAX_K:
        raise ValueError(f"asn_diff_loss: widths up to {ASN_DIFF_MAX_K} on the device")
    return _AsnDiff.apply(input1, input2)


def _asn_ppmi_host(edge_index, n, step):
    """ASN.process_graph's lines on the host: ACDNE's PPMI (the same code), row-scaled, as a float32 CSR tensor."""
    ppmi, _ = _acdne_process_graph_host(edge_index, torch.zeros(n, 1), n, step)
    import numpy as np
    a = ppmi.numpy()
    return torch.from_numpy((_row_scale(a)[:, None] * a).astype(np.float32))


def asn_gcn_norm_sparse(adj):
    """PyG's gcn_norm on a torch sparse adjacency (torch_geometric 2.3 - 2.6, gcn_conv.py, the ``is_torch_sparse_tensor``
    branch): self loops added and SUMMED with an existing diagonal, ``deg`` the row sums, ``deg^-1/2[j] v deg^-1/2[i]``.
    Returns the dense normalised matrix (host path and tests)."""
    d = adj.to_dense() if adj.layout != torch.strided else adj
    d = d + torch.eye(d.size(0), dtype=d.dtype)
    deg = d.sum(1)
    dis = deg.pow(-0.5)
    dis.masked_fill_(dis == float("inf"), 0)
    return dis[None, :] * d * dis[:, None]


def asn_ppmi_graph(edge_index, n, step):
    """ASN.process_graph as the global encoders' adjacency.  Device: ACDNE's PPMI kernels give the row-scaled PPMI
    densely, gda_asn_ppmi_count / _fill compact it with the summed self loops and the symmetric degree normalisation,
    and the result is a :class:`CSRGraph` for the SpMM (edge j -> i carries row i's entry j).  Host: the dense
    normalised matrix."""
    n, step = int(n), int(step)
    if not edge_index.is_cuda:
        return asn_gcn_norm_sparse(_asn_ppmi_host(edge_index, n, step))
    dev = edge_index.device
    buf_b = _ppmi_dense(edge_index, n, step, dev, 0, "ASN", "dense N x N buffers", "asn_ppmi")[1]
    ld = buf_b.stride(0)
    counts = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.call("gda_asn_ppmi_count", buf_b, n, ld, counts, _lib.stream())
    rp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rp[1:] = torch.cumsum(counts, 0)
    nnz = int(rp[-1])
    row = torch.empty(nnz, dtype=torch.int64, device=dev)
    cols = torch.empty(nnz, dtype=torch.int64, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    dis = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.call("gda_asn_ppmi_fill", buf_b, n, ld, rp, nnz, row, cols, val, dis, _lib.stream())
    del buf_b
    g = build_csr(torch.stack([cols, row]), n, val, add_self_loops=False, normalize=False)
    g.static = True
    return g


# ------------------------------------------------- DGDA: the bit-packed manipulated adjacency (csrc/gda_dgda.hip) --
DGDA_MAX_N = 1 << 20              # GDA_DGDA_MAX_N
DGDA_MAX_C = 1 << 16              # GDA_DGDA_MAX_C: widths of the bit-adjacency GEMM
DGDA_MAX_K = ASN_MAX_K            # decoder width of the reconstruction kernel


class DgdaBits:
    """One domain's manipulated adjacency on the device: ``bits [N, ceil(N / 32)]`` (int32 storage of the uint32 words,
    bit b of word w of row i = pair (i, 32 w + b)), ``deg = popcount(row) + 1``, ``dis = deg^-1/2`` and the scalars
    ``scal = [n_lab, pos_weight, norm, 0]``.  The buffers are refilled in place every epoch."""

    def __init__(self, n, device):
        n = int(n)
        if not 1 <= n <= DGDA_MAX_N:
            raise ValueError(f"DGDA: the bit adjacency covers 1 <= N <= {DGDA_MAX_N}, got N = {n}")
        self.n, self.words = n, (n + 31) // 32
        self.bits = torch.zeros(n, self.words, dtype=torch.int32, device=device)
        self.deg = torch.empty(n, dtype=torch.float32, device=device)
        self.dis = torch.empty(n, dtype=torch.float32, device=device)
        self.scal = torch.empty(4, dtype=torch.float32, device=device)

    def dense(self):
        """The 0/1 matrix (diagonal 1) as floats: tests and tools only."""
        sh = torch.arange(32, device=self.bits.device, dtype=torch.int32)
        b = (self.bits.unsqueeze(-1) >> sh) & 1
        return b.reshape(self.n, -1)[:, :self.n].to(torch.float32)


def dgda_p_add(labels, add_rate):
    """``sparsity * add_rate`` of drop_edges: ``sparsity = (adj.sum() + N^2) / N^2`` with ``adj = A + I`` (counts)."""
    if getattr(labels, "n_edges", None) is None:
        labels.n_edges = float(labels.fwd[2].sum())
    nn_ = float(labels.n) * float(labels.n)
    return (labels.n_edges + nn_) / nn_ * add_rate


def dgda_manip_bits(labels, drop_rate, add_rate, out=None):
    """drop_edges of one domain as a :class:`DgdaBits` (gda_dgda_manip_bits): Philox draws keyed by the seed, the device
    step counter and a call site; nothing is read back."""
    rp, ci, cnt = labels.fwd
    dev = rp.device
    p_drop, p_add = float(drop_rate), float(dgda_p_add(labels, add_rate))
    if not (0.0 <= p_drop <= 1.0 and 0.0 <= p_add <= 1.0):
        raise ValueError(f"DGDA: drop and add probabilities must lie in [0, 1], got {p_drop}, {p_add}")
    out = DgdaBits(labels.n, dev) if out is None else out
    ws, nbytes = _lib.scratch("gda_dgda_bits_workspace_bytes", dev, "dgda_bits", labels.n)
    _lib.call("gda_dgda_manip_bits", rp, ci, cnt, labels.n, p_drop, p_add, *dropout_state.generator(dev), out.bits,
              out.deg, out.dis, out.scal, ws, nbytes, _lib.stream())
    return out


def dgda_pack_bits(adj, out=None):
    """A dense ``[N, N]`` matrix (``> 0`` is an edge, the diagonal is set) as a :class:`DgdaBits`."""
    adj = _f32c(adj, "adj")
    n = adj.size(0)
    if adj.dim() != 2 or adj.size(1) != n:
        raise ValueError(f"dgda_pack_bits: a square matrix expected, got {tuple(adj.shape)}")
    out = DgdaBits(n, adj.device) if out is None else out
    if out.n != n:
        raise ValueError(f"dgda_pack_bits: the matrix has {n} rows, the bit buffers {out.n}")
    ws, nbytes = _lib.scratch("gda_dgda_bits_workspace_bytes", adj.device, "dgda_bits", n)
    _lib.call("gda_dgda_pack_bits_f32", adj, n, n, out.bits, out.deg, out.dis, out.scal, ws, nbytes, _lib.stream())
    return out


def dgda_manip_host(adj, drop_mask, add_mask):
    """The bit rule on dense host tensors: ``adj = A + I`` (counts), the two masks as drop_edges draws them over all
    pairs.  For i > j: ``add OR (adj - drop > 0)``, mirrored, diagonal 1."""
    keep = ((adj - drop_mask) > 0) | (add_mask > 0)
    low = torch.tril(keep, -1)
    return (low | low.t() | torch.eye(adj.size(0), dtype=torch.bool, device=adj.device)).to(adj.dtype)


def _bitadj_gemm(h, bits, bias):
    n, c = h.shape
    out = torch.empty(n, c, dtype=torch.float32, device=h.device)
    with profiler.region(f"dgda_bitadj_gemm[{c}]", 1, 4 * 2 * n * c + 4 * n * bits.words, 2 * n * n * c):
        _lib.call("gda_dgda_bitadj_gemm_f32", bits.bits, n, bits.dis, h, c, c, bias, out, c, _lib.stream())
    return out


class _BitPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, bias, bits):
        ctx.bits = bits
        return _bitadj_gemm(_f32c(h, "h"), bits, None if bias is None else _f32c(bias, "bias"))

    @staticmethod
    def backward(ctx, g):
        g = _f32c(g, "grad")
        gh = _bitadj_gemm(g, ctx.bits, None) if ctx.needs_input_grad[0] else None     # the matrix is symmetric
        gb = colsum(g) if ctx.needs_input_grad[1] else None
        return gh, gb, None


def dgda_bit_propagate(h, bits, bias=None):
    """``dis * (B~ (dis * h)) + bias`` for the bit adjacency ``bits`` (diagonal weight 2): the GCN aggregation of the
    manipulated pass as a GEMM over the nodes (gda_dgda_bitadj_gemm_f32).  The backward is the same call on the
    gradient."""
    if h.dim() != 2 or h.size(0) != bits.n:
        raise ValueError(f"dgda_bit_propagate: h must be [{bits.n}, C], got {tuple(h.shape)}")
    if not 1 <= h.size(1) <= DGDA_MAX_C:
        raise ValueError(f"dgda_bit_propagate: the kernel covers 1 <= C <= {DGDA_MAX_C}, got C = {h.size(1)}")
    return _BitPropagate.apply(h, bias, bits)


def dgda_recon_loss(z, bits):
    """``norm * BCEWithLogits(z z^T, nadj + I, pos_weight)`` of the manipulated pass: labels from the bit tile (2 on the
    diagonal), ``norm`` and ``pos_weight`` from the device scalars of ``bits``.  K <= DGDA_MAX_K."""
    if z.dim() != 2 or z.size(0) != bits.n:
        raise ValueError(f"dgda_recon_loss: z must be [{bits.n}, K], got {tuple(z.shape)}")
    if not 1 <= z.size(1) <= DGDA_MAX_K:
        raise ValueError(f"dgda_recon_loss: the kernel covers 1 <= K <= {DGDA_MAX_K}, got K = {z.size(1)}")
    return _PairRecon.apply(z, ("dgda_recon_bits", "dgda_recon", (bits.bits, bits.scal)))


def dgda_walks(rowptr, col, start, length):
    """Uniform random walks ``[len(start), length + 1]`` over the int64 CSR (gda_dgda_walks): one lane per walk, the
    steps from Philox; a node without out-edges stays put.  ``start`` must lie in ``[0, N)``: host tensors are checked,
    device tensors are the caller's to keep in range (DWPretrain's come from ``randperm(N)``)."""
    dev = rowptr.device
    n = rowptr.numel() - 1
    if not start.is_cuda and start.numel() and (int(start.min()) < 0 or int(start.max()) >= n):
        raise ValueError(f"dgda_walks: start nodes outside [0, {n})")       # (a device tensor is not read back)
    start = start.to(dev, torch.int64).contiguous()
    out = torch.empty(start.numel(), int(length) + 1, dtype=torch.int64, device=dev)
    _lib.call("gda_dgda_walks", rowptr, col, n, start, start.numel(), int(length), *dropout_state.generator(dev), out,
              _lib.stream())
    return out


def dgda_norm_graph(labels, loops=1):
    """The plain pass's adjacency ``D^-1/2 (A + loops I) D^-1/2`` (vectorized_sym_norm: duplicate edges count, rows =
    ``edge_index[0]``, row-sum degrees on both sides) as a :class:`CSRGraph` for ``propagate``.  ``labels`` is the
    domain's :class:`AsnLabels` (the CSR of ``A + I``); ``loops > 1`` adds the further ``I`` that every ``predict`` call
    stacks onto the stored target adjacency."""
    rp, ci, cnt = labels.fwd
    n = labels.n
    rows = torch.repeat_interleave(torch.arange(n, device=rp.device), (rp[1:] - rp[:-1]).to(torch.int64))
    cols = ci.to(torch.int64)
    val = cnt + (rows == cols).to(torch.float32) * float(loops - 1)
    deg = torch.zeros(n, dtype=torch.float32, device=rp.device).index_add_(0, rows, val)
    dis = 1.0 / deg.sqrt()
    dis.masked_fill_(torch.isinf(dis), 0.0)
    g = build_csr(torch.stack([cols, rows]), n, dis[rows] * val * dis[cols], add_self_loops=False, normalize=False)
    g.static = True
    return g


# ------------------------------------------------------------------------------------------------------------ JHGDA --
JHGDA_PROX_MAX_N = 1 << 20        # GDA_JHGDA_PROX_MAX_N
JHGDA_PROX_MAX_K = 4096           # GDA_JHGDA_PROX_MAX_K: pooled widths the proximity kernel covers


class JhgdaEdges:
    """Level 0's adjacency for the proximity kernel: the edge list as a CSR by source row and its transpose (int32,
    columns ascending inside a row, duplicate edges kept: each occurrence counts, as ``pos_adj[A[0], A[1]]`` does).
    Built once per graph; ``edge_index`` stays for the host lines."""

    def __init__(self, edge_index, n):
        self.n, self.edge_index = int(n), edge_index
        self.fwd = self._csr(edge_index[0], edge_index[1]) if edge_index.is_cuda else None
        self.bwd = self._csr(edge_index[1], edge_index[0]) if edge_index.is_cuda else None

    def _csr(self, row, col):
        n = self.n
        order = torch.argsort(row * n + col, stable=True)
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=row.device)
        rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
        return rowptr.to(torch.int32), col[order].to(torch.int32).contiguous()


def _jhgda_prox_host(A, S):
    """proximity_loss(A, S) of jhgda_base.py:337-377, adj_hop = 1: ``A`` an edge list [2, E] or a dense matrix."""
    eps = 1e-7
    n = S.size(0)
    p = torch.min(S @ S.T, torch.ones(1, dtype=S.dtype, device=S.device))
    pos, neg = torch.log(p + eps), torch.log(1 - p + eps)
    if A.shape[0] < A.shape[1]:
        return (-torch.sum(pos[A[0], A[1]]) - (torch.sum(neg) - torch.sum(neg[A[0], A[1]]))) / float(n * n)
    return torch.sum(-A * pos - (1 - A) * neg) / float(n * n)


class _JhgdaProx(torch.autograd.Function):
    """Loss and gradients in one launch sequence (gda_jhgda_prox_f32); the backward scales them by the incoming
    scalar gradient."""

    @staticmethod
    def forward(ctx, S, A, edges):
        S = _f32c(S, "S")
        n, k = S.shape
        ws, nbytes = _lib.scratch("gda_jhgda_prox_workspace_bytes", S.device, "jhgda_prox", n, k)
        loss = torch.empty(1, dtype=torch.float32, device=S.device)
        dS = torch.empty_like(S) if ctx.needs_input_grad[0] else None      # None: the loss alone, no strip, no GEMM
        dA = None
        if edges is not None:
            (rp, ci), (trp, tci) = edges.fwd, edges.bwd
            args = (rp, ci, trp, tci, None, 0, loss, dS, k, None, 0)
        else:
            A = _f32c(A, "A")
            dA = torch.empty_like(A) if ctx.needs_input_grad[1] else None
            args = (None, None, None, None, A, n, loss, dS, k, dA, n)
        with profiler.region(f"jhgda_prox[{k}]", 3, 4 * n * k * 4, 4 * n * n * k):
            _lib.call("gda_jhgda_prox_f32", S, k, n, k, *args, ws, nbytes, _lib.stream())
        ctx.save_for_backward(dS, dA)
        ctx.has_dS, ctx.has_dA = dS is not None, dA is not None
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dS, dA = ctx.saved_tensors
        return (dS * g if ctx.has_dS else None), (dA * g if ctx.has_dA else None), None


def jhgda_prox(A, S, edges=None):
    """``JHGDABase.proximity_loss(A, S)`` (jhgda_base.py:337-377).  ``A``: level 0's ``edge_index`` [2, E] (pass its
    :class:`JhgdaEdges` as ``edges`` on the device) or a pooled dense [N, N] adjacency (differentiable).  Device
    tensors: gda_jhgda_prox_f32 -- loss, dS (and dA) from one pass over the pairs, no N x N buffer; host tensors: the
    reference's dense lines."""
    if not S.is_cuda:
        return _jhgda_prox_host(A, S)
    n, k = S.shape
    if n > JHGDA_PROX_MAX_N or k > JHGDA_PROX_MAX_K:
        raise ValueError(f"jhgda_prox: the kernel covers N <= {JHGDA_PROX_MAX_N}, K <= {JHGDA_PROX_MAX_K}; "
                         f"got S of shape {tuple(S.shape)}")
    if A.shape[0] < A.shape[1]:
        if edges is None:
            edges = JhgdaEdges(A, n)
        return _JhgdaProx.apply(S, None, edges)
    if A.shape != (n, n):
        raise ValueError(f"jhgda_prox: a dense A must be [{n}, {n}], got {tuple(A.shape)}")
    return _JhgdaProx.apply(S, A, None)


class _JhgdaPoolRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X):
        X = _f32c(X, "X")
        n, k = X.shape
        S = torch.empty_like(X)
        ent = torch.empty(n, dtype=torch.float32, device=X.device)
        ce = torch.empty(1, dtype=torch.float32, device=X.device)
        with profiler.region(f"jhgda_pool_rows[{k}]", 2, 4 * n * k * 2, 0):
            _lib.call("gda_jhgda_pool_rows_fwd_f32", X, k, n, k, S, k, ent, ce, _lib.stream())
        ctx.save_for_backward(X, S)
        return S, ce.reshape(())

    @staticmethod
    def backward(ctx, gS, gce):
        X, S = ctx.saved_tensors
        n, k = X.shape
        gS = gS.contiguous() if gS is not None else None
        gce = gce.reshape(1).contiguous() if gce is not None else None
        dX = torch.empty_like(X)
        _lib.call("gda_jhgda_pool_rows_bwd_f32", X, k, S, k, gS, k, gce, n, k, dX, k, _lib.stream())
        return dX


def jhgda_pool_rows(X):
    """``(S, entropy(S))`` with ``S = softmax(relu(X), dim=1)`` and ``JHGDABase.entropy`` (eps 1e-7): GCNPooling's
    assignment and its ``ce`` term.  Device: one row kernel each way (gda_jhgda_pool_rows_*_f32)."""
    if not X.is_cuda:
        S = torch.softmax(torch.relu(X), dim=1)
        return S, torch.mean(torch.sum(-S * torch.log(S + 1e-7), dim=1))
    return _JhgdaPoolRows.apply(X)


def _tn(a, b):
    """``a^T b`` on the project's GEMM.  The TN kernel splits the row reduction into slabs whose partial products sit in
    its workspace: ``slabs x M x N`` floats, gigabytes for the wide products here (S^T (A S) at [1,872 x 1,872] from
    9,360 rows: 990 MB; a [1,872 x 6,775] weight gradient: 3.6 GB).  Where that workspace is larger than ``a`` itself,
    ``a`` is transposed once and the product runs as NN, which needs no workspace at these widths."""
    K, M = a.shape
    N = b.size(1)
    L = _lib.lib()
    if (L.gda_gemm_workspace_bytes(GEMM_TN, M, N, K) > 4 * a.numel()
            and L.gda_gemm_workspace_bytes(GEMM_NN, M, N, K) == 0):
        return gemm(GEMM_NN, a.t().contiguous(), b)
    return gemm(GEMM_TN, a, b)


class _MatTN(torch.autograd.Function):
    """``a^T b`` for ``a [N, M]``, ``b [N, P]`` on the project's GEMM (_tn); gradients ``b gy^T`` (NT) and ``a gy``
    (NN)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _tn(a, b)

    @staticmethod
    def backward(ctx, gy):
        a, b = ctx.saved_tensors
        gy = gy.contiguous()
        ga = gemm(GEMM_NT, b, gy) if ctx.needs_input_grad[0] else None
        gb = gemm(GEMM_NN, a, gy) if ctx.needs_input_grad[1] else None
        return ga, gb


def mat_tn(a, b):
    """``a.T @ b``: the project's GEMM on device tensors, torch on host tensors."""
    return _MatTN.apply(a, b) if a.is_cuda else a.T @ b


class _LinearNT(torch.autograd.Function):
    """``x W^T`` with the weight gradient ``gy^T x`` through _tn (no split-K slabs for wide weights)."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return gemm(GEMM_NT, x, weight)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gemm(GEMM_NN, gy, weight) if ctx.needs_input_grad[0] else None
        gw = _tn(gy, x) if ctx.needs_input_grad[1] else None
        return gx, gw


def linear_nt(x, weight):
    """``x @ weight.T`` on the project's GEMM (device tensors)."""
    return _LinearNT.apply(_f32c(x, "x"), weight)


# ------------------------------------------------------------------ SEPA: structure-enhanced prototypes (gda_sepa.hip) --
SEPA_MAX_CLASSES, SEPA_MAX_WIDTH = 32, 1024


def sepa_bytes(n, c, h):
    """Device memory of one ``sepa_term`` beyond its inputs: the row buffers (P, dPu, X, dZ [N, C]; U, R, dR, dU, dF
    [N, h]; pred, e, w, de [N]) and the grouped reductions' partials: ``O(N (h + C) + blocks C (h + C))``."""
    blocks = (n + 63) // 64
    return 4 * (4 * n * c + 5 * n * h + 4 * n + blocks * c * (h + c + 2))


def _sepa_ws(n, c, d, dev):
    return _lib.scratch("gda_sepa_workspace_bytes", dev, "sepa", n, c, d)[0]


def _sepa_check(c, d, what):
    if c > SEPA_MAX_CLASSES or d > SEPA_MAX_WIDTH:
        raise ValueError(f"{what}: the SEPA kernels cover up to {SEPA_MAX_CLASSES} classes and widths up to "
                         f"{SEPA_MAX_WIDTH}, got {c} classes and width {d}")


def _sepa_group_sum(x, idx, c, w=None, divide=False, eps=0.0, add=None):
    """``(out [C, d], cnt [C])`` of gda_sepa_group_sum_f32 (no autograd)."""
    n, d = x.shape
    out = torch.empty(c, d, dtype=torch.float32, device=x.device)
    cnt = torch.empty(c, dtype=torch.float32, device=x.device)
    ws = _sepa_ws(n, c, d, x.device)
    _lib.call("gda_sepa_group_sum_f32", x, d, idx, w, n, d, c, int(divide), float(eps), add, out, cnt, ws, ws.numel(),
              _lib.stream())
    return out, cnt


def _sepa_class_mean_bwd(g, cnt, idx, n, eps, g0=None):
    c, d = g.shape
    dx = torch.empty(n, d, dtype=torch.float32, device=g.device)
    _lib.call("gda_sepa_class_mean_bwd_f32", g, cnt, idx, g0, n, d, c, float(eps), dx, _lib.stream())
    return dx


class _SepaClassMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, c, eps):
        x = _f32c(x, "x")
        out, cnt = _sepa_group_sum(x, idx, c, divide=True, eps=eps)
        ctx.save_for_backward(idx, cnt)
        ctx.n, ctx.eps = x.size(0), eps
        return out

    @staticmethod
    def backward(ctx, g):
        idx, cnt = ctx.saved_tensors
        return _sepa_class_mean_bwd(g.contiguous(), cnt, idx, ctx.n, ctx.eps), None, None, None


def sepa_class_mean(x, idx, num_classes, eps=0.0):
    """``(x^T onehot(idx) / (count + eps))^T``: the class-grouped mean ``[C, d]`` of the rows of ``x [N, d]``, with its
    gather backward.  Device: gda_sepa_group_sum_f32 / gda_sepa_class_mean_bwd_f32 (ordered, no atomics)."""
    if not x.is_cuda:
        onehot = torch.eye(num_classes, dtype=x.dtype, device=x.device)[idx.long()]
        return ((x.t() @ onehot) / (onehot.sum(dim=0) + eps)).t()
    _sepa_check(num_classes, x.size(1), "sepa_class_mean")
    return _SepaClassMean.apply(x, idx.to(torch.int32).contiguous(), int(num_classes), float(eps))


def _ppr_steps(x, graph, k, alpha, transposed):
    out = x
    for _ in range(k):                       # t <- (1 - alpha) A t + alpha x: the restart rides in the z operand
        out = spmm_axpby(graph, out, 0.0, 1.0 - alpha, z=x, gamma=alpha, transposed=transposed)
    return out


class _PPR(torch.autograd.Function):
    """``x_{j+1} = (1 - alpha) A x_j + alpha x_0``, ``k`` times.  The gradient is the same recurrence on the transposed
    CSR (``G_j = (1 - alpha) A^T G_{j+1}``, ``dx_0 = G_0 + alpha sum_{j >= 1} G_j``, in Horner form): k launches each
    way, nothing saved but the graph."""

    @staticmethod
    def forward(ctx, x, graph, k, alpha):
        ctx.graph, ctx.k, ctx.alpha = graph, k, alpha
        return _ppr_steps(_f32c(x, "x"), graph, k, alpha, False)

    @staticmethod
    def backward(ctx, g):
        return _ppr_steps(g.contiguous(), ctx.graph, ctx.k, ctx.alpha, True), None, None, None


def ppr(x, graph: CSRGraph, k=5, alpha=0.9):
    """SEPA's personalised PageRank: ``k`` steps of ``x <- (1 - alpha) A x + alpha x_0`` on the normalised graph."""
    if k < 1:
        return x
    return _PPR.apply(x, graph, int(k), float(alpha))


def _sepa_proto_launch(T, S, tau, wpp, wsep, want_grad=True):
    c, h = T.shape
    losses = torch.empty(2, dtype=torch.float32, device=T.device)
    dT = torch.empty_like(T) if want_grad else None
    dS = torch.empty_like(S) if want_grad else None
    _lib.call("gda_sepa_proto_f32", T, S, c, h, float(tau), float(wpp), float(wsep), losses, dT, dS, _lib.stream())
    return losses, dT, dS


class _SepaProto(torch.autograd.Function):
    @staticmethod
    def forward(ctx, T, S, tau, which):
        T, S = _f32c(T, "target_proto"), _f32c(S, "source_proto")
        losses, dT, dS = _sepa_proto_launch(T, S, tau, 1.0 - which, float(which))
        ctx.save_for_backward(dT, dS)
        return losses[which].reshape(())

    @staticmethod
    def backward(ctx, g):
        dT, dS = ctx.saved_tensors
        return (g * dT if ctx.needs_input_grad[0] else None), (g * dS if ctx.needs_input_grad[1] else None), None, None


def sepa_proto_alignment(target_proto, source_proto, tau):
    """SEPA's ``proto_alignment`` on device prototypes ``[C, h]`` (gda_sepa_proto_f32, forward and gradients in one
    launch)."""
    _sepa_check(*target_proto.shape, "sepa_proto_alignment")
    return _SepaProto.apply(target_proto, source_proto, float(tau), 0)


def sepa_separate(center, tau):
    """SEPA's ``seperate_center`` on device prototypes ``[C, h]`` (gda_sepa_proto_f32)."""
    _sepa_check(*center.shape, "sepa_separate")
    return _SepaProto.apply(center.detach(), center, float(tau), 1)


class _SepaTerm(torch.autograd.Function):
    """``lam_im loss_im + lam_pp loss_pp + lam_sep loss_sep`` of SEPA from the target logits ``Z``, the target
    features ``F`` and the source features ``Fs``: 18 launches forward (5 of them the PageRank's SpMMs), 14 backward,
    every reduction ordered.  Also returns the three parts (detached)."""

    @staticmethod
    def forward(ctx, Z, F, Fs, ys, graph, lam_im, lam_pp, lam_sep, tau, k, alpha):
        Z, F, Fs = _f32c(Z.detach(), "Z"), _f32c(F.detach(), "F"), _f32c(Fs.detach(), "Fs")
        n, c = Z.shape
        h = F.size(1)
        dev = Z.device
        st = _lib.stream
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        P, pred, e = new(n, c), torch.empty(n, dtype=torch.int32, device=dev), new(n)
        _lib.call("gda_sepa_stats_f32", Z, n, c, P, pred, e, st())
        SP, cnt = _sepa_group_sum(P, pred, c)
        SF, _ = _sepa_group_sum(F, pred, c)
        B, M, parts = new(c, h), new(c, c), new(3)
        _lib.call("gda_sepa_mid_f32", SP, cnt, SF, e, n, c, h, B, M, parts, st())
        U = new(n, h)
        _lib.call("gda_sepa_unbias_rows_f32", P, pred, M, B, n, c, h, U, st())
        R = _ppr_steps(U, graph, k, alpha, False)
        w = new(n)
        _lib.call("gda_sepa_row_weight_f32", R, e, n, h, w, st())
        center, _ = _sepa_group_sum(R, pred, c, w=w, divide=True, eps=1e-12, add=B)
        sproto, cnt_s = _sepa_group_sum(Fs, ys, c, divide=True, eps=0.0)
        dcenter, dsproto = new(c, h), new(c, h)
        _lib.call("gda_sepa_proto_f32", center, sproto, c, h, float(tau), float(lam_pp), float(lam_sep), parts[1:],
                  dcenter, dsproto, st())
        ctx.save_for_backward(P, pred, e, SP, cnt, B, M, R, dcenter, dsproto, cnt_s, ys)
        ctx.graph, ctx.k, ctx.alpha, ctx.lam_im, ctx.ns = graph, k, alpha, float(lam_im), Fs.size(0)
        total = lam_im * parts[0] + lam_pp * parts[1] + lam_sep * parts[2]
        ctx.mark_non_differentiable(parts, pred)
        return total, parts, pred

    @staticmethod
    def backward(ctx, g, _gparts, _gpred):
        P, pred, e, SP, cnt, B, M, R, dcenter, dsproto, cnt_s, ys = ctx.saved_tensors
        n, c = P.shape
        h = B.size(1)
        dev = P.device
        st = _lib.stream
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        g0 = g.reshape(1).to(torch.float32).contiguous()
        dR, de = new(n, h), new(n)
        _lib.call("gda_sepa_center_rows_bwd_f32", R, e, pred, dcenter, cnt, g0, n, c, h, dR, de, st())
        dU = _ppr_steps(dR, ctx.graph, ctx.k, ctx.alpha, True)
        dPu, X, dBf = new(n, c), new(n, c), new(c, h)
        ws = _sepa_ws(n, c, h, dev)
        _lib.call("gda_sepa_unbias_rows_bwd_f32", dU, P, pred, M, B, n, c, h, dPu, X, dBf, ws, ws.numel(), st())
        dMn, _ = _sepa_group_sum(X, pred, c)
        dBt, GP, gim = new(c, h), new(c, c), new(c + 1)
        _lib.call("gda_sepa_mid_bwd_f32", dMn, SP, cnt, dBf, dcenter, g0, ctx.lam_im, n, c, h, dBt, GP, gim, st())
        dZ = new(n, c)
        _lib.call("gda_sepa_dz_rows_f32", P, pred, dPu, GP, gim, de, n, c, dZ, st())
        dF = _sepa_class_mean_bwd(dBt, cnt, pred, n, 1e-12)
        dFs = _sepa_class_mean_bwd(dsproto, cnt_s, ys, ctx.ns, 0.0, g0)
        return (dZ, dF, dFs) + (None,) * 8


def sepa_term(target_logits, target_feat, source_feat, source_labels, graph, lam_im, lam_pp, lam_sep, tau, k=5,
              alpha=0.9):
    """SEPA's prototype term on the device: ``(lam_im loss_im + lam_pp loss_pp + lam_sep loss_sep, parts [3], pred)``
    from the target's logits and bottleneck features and the source's bottleneck features; ``graph`` is the target's
    gcn-normalised :class:`CSRGraph`, ``source_labels`` int32.  ``parts`` and ``pred`` carry no gradient."""
    n, c = target_logits.shape
    _sepa_check(c, target_feat.size(1), "sepa_term")
    return _SepaTerm.apply(target_logits, target_feat, source_feat, source_labels, graph, float(lam_im),
                           float(lam_pp), float(lam_sep), float(tau), int(k), float(alpha))


# ------------------------------------------------- SOGA: smoothed CE and the contrastive adaptation term (gda_soga.hip) --
SOGA_MAX_CLASSES = 64
SOGA_MIN_SEGMENT = 16
SOGA_SEGMENT = 64        # entries of the reverse index per lane group


def soga_bytes(n, c, m, k, v=2):
    """Device memory of one ``soga_adapt`` beyond its inputs and the plan: P [N, G], sigma [V, M, K], the centre
    gradients [V, M, G], the segment partials and dlogits; ``(bytes written, bytes gathered)`` with G = next_pow2(C)."""
    g = 1 << max(int(c) - 1, 0).bit_length()
    rev = v * m * (k + 2)
    return 4 * (n * g + v * m * (k + g) + n * g + n * c), 4 * (v * m * (k + 2) * g + rev * (g + 3) + n * g)


def _soga_smooth_ce_host(logits, labels, epsilon):
    logp = torch.log_softmax(logits, dim=1)
    c = logits.size(1)
    t = torch.zeros_like(logp).scatter_(1, labels.long().unsqueeze(1), 1.0)
    t = (1 - epsilon) * t + epsilon / c
    return (-t * logp).sum(dim=1).mean()


class _SogaSmoothCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, epsilon):
        x = _f32c(logits.detach(), "logits")
        _lib.require_gpu_tensor(labels, "labels", torch.int64)
        n, c = x.shape
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        stats = torch.empty(2, dtype=torch.float64, device=x.device)
        gx = torch.empty_like(x)
        ws, nbytes = _lib.scratch("gda_soga_ce_workspace_bytes", x.device, "soga_ce", n, c)
        _lib.call("gda_soga_smooth_ce_f32", x, labels.contiguous(), n, c, float(epsilon), loss, gx, stats, ws, nbytes,
                  _lib.stream())
        global _ce_stats
        _ce_stats = (weakref.ref(logits), weakref.ref(labels), n, stats, logits._version, labels._version)
        ctx.save_for_backward(gx)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        (gx,) = ctx.saved_tensors
        return gx * gl, None, None


def soga_smooth_ce(logits, labels, epsilon=0.1):
    """SOGA's ``CustomizedCrossEntropy`` (pygda/nn/soga_base.py): the mean over rows of ``-(t * log_softmax).sum(1)``
    with ``t = (1 - epsilon) onehot + epsilon / C``.  Device: gda_soga_smooth_ce_f32, which also leaves
    ``[loss, correct arg-maxes]`` for :func:`ce_stats_for`; host tensors take the torch composition (any dtype)."""
    if logits.dim() != 2 or labels.dim() != 1 or labels.numel() != logits.size(0):
        raise ValueError(f"logits [N, C] and labels [N] expected, got {tuple(logits.shape)} and {tuple(labels.shape)}")
    if not logits.is_cuda:
        return _soga_smooth_ce_host(logits, labels, float(epsilon))
    if logits.size(1) > SOGA_MAX_CLASSES:
        raise _lib.GdaError(f"soga_smooth_ce: up to {SOGA_MAX_CLASSES} classes, got {logits.size(1)}")
    return _SogaSmoothCE.apply(logits, labels, float(epsilon))


class SogaPlan:
    """SOGA's fixed tables on a device and the reverse index of their entries (:func:`soga_plan`).

    ``center`` / ``positive`` ``[V, M]`` and ``negative`` ``[V, M, K]`` hold node ids.  The reverse index is a CSR by
    node over the ``V M (K + 2)`` entries ``(view, row, role, k)``: ``rev_ptr [N + 1]``, ``rev_row`` (``view * M +
    row``) and ``rev_code`` (0 the centre, 1 the positive, ``2 + k`` negative ``k``) as numpy arrays, sorted by that
    tuple inside a node.  On the device it lives in the form the kernel gathers with (``rev_src``, ``rev_sig``) beside
    its cut into segments of ``segment`` entries (``seg_off``, ``node_seg``)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def soga_plan(tables, n, device="cpu", segment=None):
    """The plan for ``tables`` -- one ``(center [M] or [M, 1], positive, negative [M, K])`` triple per view, one or two
    views, as numpy arrays or tensors -- on ``n`` nodes.  The reverse index is built once here by a stable counting
    sort on the host.  Raises GdaError for an id outside ``[0, n)``, views of different shapes and more than two views."""
    n = int(n)
    segment = max(int(SOGA_SEGMENT if segment is None else segment), SOGA_MIN_SEGMENT)
    import numpy as np
    as_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if not 1 <= len(tables) <= 2:
        raise _lib.GdaError(f"soga_plan: one or two views expected, got {len(tables)}")
    cen = [as_np(t[0]).reshape(-1).astype(np.int64) for t in tables]
    pos = [as_np(t[1]).reshape(-1).astype(np.int64) for t in tables]
    neg = [as_np(t[2]).astype(np.int64) for t in tables]
    m = cen[0].size
    if any(x.ndim != 2 for x in neg):
        raise _lib.GdaError("soga_plan: negative tables [M, K] expected")
    k = neg[0].shape[1]
    for c_, p_, n_ in zip(cen, pos, neg):
        if c_.size != m or p_.size != m or n_.shape[0] != m:
            raise _lib.GdaError(f"soga_plan: every table needs the same {m} rows")
        if n_.shape[1] != k:
            raise _lib.GdaError(f"soga_plan: K mismatch, the views have {k} and {n_.shape[1]} negatives per row")
    if m < 1 or k < 1 or n < 1:
        raise _lib.GdaError("soga_plan: empty tables")
    cen, pos, neg = np.stack(cen), np.stack(pos), np.stack(neg)                     # [V, M], [V, M], [V, M, K]
    v = cen.shape[0]
    entries = np.concatenate([cen[:, :, None], pos[:, :, None], neg], axis=2)       # (view, row, role / k) order
    if entries.min() < 0 or entries.max() >= n:
        raise _lib.GdaError(f"soga_plan: a table holds an index outside [0, {n})")
    if entries.size >= 2 ** 31:
        raise _lib.GdaError("soga_plan: more than 2^31 table entries")
    node = entries.reshape(-1)
    order = np.argsort(node, kind="stable")                                         # by node, the tuple's order inside
    counts = np.bincount(node, minlength=n)
    rev_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rev_row, rev_code = order // (k + 2), order % (k + 2)
    view = rev_row // m
    rev_src = np.where(rev_code == 0, rev_row, cen.reshape(-1)[rev_row])
    rev_sig = np.where(rev_code >= 2, rev_row * k + rev_code - 2, np.where(rev_code == 1, -1 - view, -3 - view))
    per_node = (counts + segment - 1) // segment
    node_seg = np.concatenate([[0], np.cumsum(per_node)]).astype(np.int64)
    seg_node = np.repeat(np.arange(n), per_node)
    seg_off = rev_ptr[seg_node] + (np.arange(seg_node.size) - node_seg[seg_node]) * segment
    seg_off = np.concatenate([seg_off, [node.size]])
    dev = torch.device(device)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
    on_dev = dev.type == "cuda"
    return SogaPlan(n=n, m=m, k=k, v=v, segment=segment, device=dev, rev_ptr=rev_ptr, rev_row=rev_row, rev_code=rev_code,
                    center=(i32 if on_dev else i64)(cen), positive=(i32 if on_dev else i64)(pos),
                    negative=(i32 if on_dev else i64)(neg), node_seg=i32(node_seg), seg_off=i32(seg_off),
                    nseg=int(seg_node.size), rev_src=i32(rev_src), rev_sig=i32(rev_sig), nrev=int(node.size))


def _soga_adapt_host(logits, plan, lam_struct, lam_neigh):
    """The reference's lines (pygda/models/soga.py ``train_target`` / ``NCE_loss`` / ``ent`` / ``div``), any dtype."""
    prob = torch.softmax(logits, dim=-1)
    ent = torch.mean(torch.sum(-prob * torch.log(prob + 1e-5), dim=1))
    mean = prob.mean(dim=0)
    im = ent - torch.sum(-mean * torch.log(mean + 1e-8))
    nce = []
    for v in range(plan.v):
        c, p, ng = prob[plan.center[v]], prob[plan.positive[v]], prob[plan.negative[v]]          # [M, C], [M, C], [M, K, C]
        pos_score = torch.exp((c * p).sum(-1))
        neg_score = torch.exp((c.unsqueeze(1) * ng).sum(-1)).sum(dim=1)
        nce.append((-torch.log(pos_score / neg_score)).mean())
    if plan.v == 1:
        nce.append(torch.zeros((), dtype=logits.dtype, device=logits.device))
        loss = im + lam_struct * nce[0]
    else:
        loss = im + lam_struct * nce[0] + lam_neigh * nce[1]
    return loss, torch.stack([loss, im, nce[0], nce[1]]).detach()


class _SogaAdapt(torch.autograd.Function):
    """``IM + lam_struct NCE_struct + lam_neigh NCE_neigh`` and its gradient in five launches (gda_soga_adapt_f32);
    backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, logits, plan, lam_struct, lam_neigh):
        x = _f32c(logits.detach(), "logits")
        n, c = x.shape
        out = torch.empty(4, dtype=torch.float32, device=x.device)
        gx = torch.empty_like(x)
        ws, nbytes = _lib.scratch("gda_soga_workspace_bytes", x.device, "soga_adapt", n, c, plan.m, plan.k, plan.v)
        with profiler.region("soga_adapt", 5, sum(soga_bytes(n, c, plan.m, plan.k, plan.v)) if profiler.enabled else 0):
            _lib.call("gda_soga_adapt_f32", x, n, c, plan.center, plan.positive, plan.negative, plan.v, plan.m, plan.k,
                      lam_struct, lam_neigh, plan.node_seg, plan.seg_off, plan.nseg, plan.rev_src, plan.rev_sig,
                      plan.nrev, out, gx, ws, nbytes, _lib.stream())
        ctx.save_for_backward(gx)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, gl, _gparts):
        (gx,) = ctx.saved_tensors
        return gx * gl, None, None, None


def soga_adapt(logits, plan, lam_struct=1.0, lam_neigh=1.0):
    """SOGA's adaptation loss of one epoch from the target logits ``[N, C]`` and a :class:`SogaPlan`:
    ``(loss, parts)`` with ``parts = [loss, IM, NCE_struct, NCE_neigh]`` (detached; the last is 0 for a one-view
    plan).  Differentiable with respect to the logits.  Host tensors take the torch composition (any dtype)."""
    if logits.dim() != 2 or logits.size(0) != plan.n:
        raise _lib.GdaError(f"soga_adapt: logits [{plan.n}, C] expected, got {tuple(logits.shape)}")
    if logits.device.type != plan.device.type:
        raise _lib.GdaError(f"soga_adapt: the plan lives on {plan.device}, the logits on {logits.device}")
    if not logits.is_cuda:
        return _soga_adapt_host(logits, plan, float(lam_struct), float(lam_neigh))
    if logits.size(1) > SOGA_MAX_CLASSES:
        raise _lib.GdaError(f"soga_adapt: up to {SOGA_MAX_CLASSES} classes, got {logits.size(1)}")
    return _SogaAdapt.apply(logits, plan, float(lam_struct), float(lam_neigh))


# ----------------------------------- GTrans: differentiable edge-weight GCN, cosine loss, budget projection (gda_gtrans.hip) --
WGCN_SEGMENT = 128       # GDA_WGCN_SEGMENT: graph.SPLIT_THRESHOLD, the hub-row cut of the SpMM
WGCN_MAX_WIDTH = 256


def gtrans_bytes(n, f, nnz, m, d):
    """Device memory of a GTrans adaptation: ``(resident, per loss evaluation)`` bytes.  Resident: the dense ``[N, F]``
    perturbation with its gradient and two Adam moments, the layer-0 projection of the features, the flip weights with
    gradient and moments, the plan's sixteen index arrays (about ``10 nnz + 6 N`` entries) and the two views' value
    arrays.  Per evaluation: two norm
    calls (five per-entry arrays each), the three passes' activations and edge gradients at width ``d``."""
    resident = 4 * (4 * n * f + n * d + 4 * m + 10 * nnz + 6 * n + 4 * nnz)
    per_loss = 4 * (2 * 5 * nnz + 3 * 2 * 4 * n * d + 3 * 2 * nnz)
    return resident, per_loss


class WgcnPlan:
    """The fixed structure of a GTrans fit (:func:`wgcn_plan`; ``gda_wgcn_plan`` of include/gda_hip.h).

    ``edge_index [2, Ec]`` is the coalesced edge list, sorted by (source, destination) -- what ``get_modified_adj``
    returns from its first call on --, ``w0 [Ec]`` the coalesced initial weights (0 for an edge that only a parameter
    creates).  Per stored entry of the by-destination CSR: ``erow``, ``col``, ``epos`` (the listed edge, -1 for a
    self-loop slot without one), ``kidx`` (the parameter group); ``entry_of_edge [Ec]`` inverts ``epos``.  On a device
    ``graphs`` holds ``views`` :class:`CSRGraph` objects over one pattern with their own value arrays, which
    :func:`wgcn_norm` refreshes in place."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def keep_factors(self, mask):
        """A keep mask over the coalesced list (one bit per edge) or over the edges AS GIVEN (one bit per listed copy:
        what ``dropout_adj`` sees before the first coalesce) as one float32 factor per coalesced edge."""
        mask = torch.as_tensor(mask)
        if mask.numel() == self.ec:
            return mask.to(torch.float32)
        if mask.numel() != self.raw_to_edge.numel():
            raise _lib.GdaError(f"keep_factors: a mask over {self.ec} coalesced or {self.raw_to_edge.numel()} given edges "
                                f"expected, got {mask.numel()}")
        kept = torch.zeros(self.ec, dtype=torch.float64).index_add_(0, self.raw_to_edge, mask.double() * self.w_in)
        return torch.where(self.w0 != 0, kept / torch.where(self.w0 != 0, self.w0, torch.ones_like(self.w0)),
                           torch.zeros_like(kept)).to(torch.float32)

    def entry_weights(self, w_edges):
        """Per-entry raw weights from per-edge ones: a self-loop slot without a listed edge holds gcn_norm's 1."""
        w = torch.ones(self.nnz, dtype=w_edges.dtype, device=w_edges.device)
        w[self.entry_of_edge] = w_edges
        return w


def wgcn_plan(edge_index, n, modified_edge_index, edge_weight=None, make_undirected=True, device="cpu", views=2):
    """The plan of a fit: ``edge_index [2, E]`` the target's edges as given (duplicates, self loops and one-directional
    edges allowed), ``modified_edge_index [2, m]`` the node pair of every flip weight.  Built once, on the host."""
    import numpy as np
    n = int(n)
    ei = edge_index.detach().cpu().long()
    mei = modified_edge_index.detach().cpu().long()
    m = int(mei.size(1))
    if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= n) or m and (int(mei.min()) < 0 or int(mei.max()) >= n):
        raise _lib.GdaError(f"wgcn_plan: an edge names a node outside [0, {n})")
    w_in = torch.ones(ei.size(1), dtype=torch.float64) if edge_weight is None else edge_weight.detach().cpu().double()
    # the parameter groups: one per distinct pair, in first-listed order of the sorted keys
    pkey = (mei[0] * n + mei[1]).numpy()
    ukey, pgrp = np.unique(pkey, return_inverse=True)
    mu = int(ukey.size)
    order = np.argsort(pgrp, kind="stable")
    gptr = np.concatenate([[0], np.cumsum(np.bincount(pgrp, minlength=mu))]).astype(np.int64)
    # the coalesced pattern: the edges and either direction (or the listed one) of every pair
    pr, pc = ukey // n, ukey % n
    fed = [np.stack([pr, pc])] + ([np.stack([pc, pr])] if make_undirected else [])
    all_key = np.concatenate([(ei[0] * n + ei[1]).numpy()] + [f[0] * n + f[1] for f in fed])
    ekey = np.unique(all_key)
    ec = int(ekey.size)
    inv = np.searchsorted(ekey, (ei[0] * n + ei[1]).numpy())
    w0 = torch.zeros(ec, dtype=torch.float64).index_add_(0, torch.from_numpy(inv), w_in)
    esrc, edst = ekey // n, ekey % n
    # stored entries: by destination, listed order inside one, self loops merged into the slot every node has
    listed_loop = esrc == edst
    has_loop = np.zeros(n, dtype=bool)
    has_loop[esrc[listed_loop]] = True
    slot_nodes = np.nonzero(~has_loop)[0]
    a_src = np.concatenate([esrc, slot_nodes])
    a_dst = np.concatenate([edst, slot_nodes])
    a_pos = np.concatenate([np.arange(ec), np.full(slot_nodes.size, -1)])
    by_dst = np.lexsort((a_src, a_dst))
    erow, col, epos = a_dst[by_dst], a_src[by_dst], a_pos[by_dst]
    nnz = int(erow.size)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(erow, minlength=n))]).astype(np.int64)
    by_src = np.lexsort((erow, col))                        # by-source CSR: position -> by-destination entry
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))]).astype(np.int64)
    t_colidx, t_to_fwd = erow[by_src], by_src
    entry_of_edge = np.empty(ec, dtype=np.int64)
    entry_of_edge[epos[epos >= 0]] = np.nonzero(epos >= 0)[0]
    # entry -> group, group -> entries
    kidx = np.full(nnz, -1, dtype=np.int64)
    pent = np.full((mu, 2), -1, dtype=np.int64)
    for j, f in enumerate(fed):
        e = entry_of_edge[np.searchsorted(ekey, f[0] * n + f[1])]
        kidx[e] = np.arange(mu)
        pent[:, j] = e

    def segments(ptr):
        cnt = np.diff(ptr)
        per = (cnt + WGCN_SEGMENT - 1) // WGCN_SEGMENT
        row_seg = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        seg_row = np.repeat(np.arange(n), per)
        off = ptr[seg_row] + (np.arange(seg_row.size) - row_seg[seg_row]) * WGCN_SEGMENT
        return np.concatenate([off, [ptr[-1]]]), row_seg, int(seg_row.size)

    seg_off, row_seg, nseg = segments(rowptr)
    t_seg_off, t_row_seg, t_nseg = segments(t_rowptr)
    dev = torch.device(device)
    on_dev = dev.type == "cuda"
    idx = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32 if on_dev else np.int64)).to(dev)
    plan = WgcnPlan(n=n, nnz=nnz, m=m, mu=mu, ec=ec, mean=bool(make_undirected), device=dev, nseg=nseg, t_nseg=t_nseg,
                    edge_index=torch.from_numpy(np.stack([esrc, edst])).to(dev), w0=w0, w_in=w_in,
                    raw_to_edge=torch.from_numpy(inv),
                    rowptr=idx(rowptr), col=idx(col), t_rowptr=idx(t_rowptr), t_colidx=idx(t_colidx),
                    t_to_fwd=idx(t_to_fwd), erow=idx(erow), epos=idx(epos), kidx=idx(kidx), pent=idx(pent),
                    gptr=idx(gptr), gidx=idx(order), pgrp=idx(pgrp), seg_off=idx(seg_off), row_seg=idx(row_seg),
                    t_seg_off=idx(t_seg_off), t_row_seg=idx(t_row_seg),
                    entry_of_edge=torch.from_numpy(entry_of_edge).to(dev), graphs=None, struct=None, gen=[0] * views)
    if on_dev:
        from .graph import KSTEP_LDS_MIN_K
        assert 1 < KSTEP_LDS_MIN_K        # K = 1 never takes the LDS K-step plan, which bakes the values into its program
        plan.struct = _lib.WgcnPlanStruct(n, nnz, m, mu, nseg, t_nseg, int(plan.mean), ec, *(
            getattr(plan, k).data_ptr() for k in ("rowptr", "col", "t_rowptr", "t_colidx", "t_to_fwd", "erow", "epos",
                                                  "kidx", "pent", "gptr", "gidx", "pgrp", "seg_off", "row_seg",
                                                  "t_seg_off", "t_row_seg")))
        plan.graphs = []
        for _ in range(views):
            plan.graphs.append(wgcn_view(plan))
    return plan


def wgcn_view(plan, val=None):
    """A further :class:`CSRGraph` over a device plan's pattern with value arrays of its own -- ``val [nnz]`` by
    destination (zeros when None; the by-source twin starts at zero and is refreshed only by :func:`wgcn_norm` on the
    plan's own views) -- on the hub-row layout of the plan's first view: one pattern, one layout."""
    dev = plan.device
    val = torch.zeros(plan.nnz, dtype=torch.float32, device=dev) if val is None else _f32c(val, "val").clone()
    g = CSRGraph(plan.n, plan.nnz, plan.rowptr, plan.col, val, plan.t_rowptr, plan.t_colidx,
                 torch.zeros(plan.nnz, dtype=torch.float32, device=dev))
    g._nnz, g.t_to_fwd = plan.nnz, plan.t_to_fwd
    if plan.graphs:
        g._split, g._t_split = plan.graphs[0].split(False), plan.graphs[0].split(True)
    else:
        g.split(False), g.split(True)
    return g


def _wgcn_norm_host(plan, w_prev, p, keep):
    """The torch composition (any dtype): the reference's coalesce-and-fold and gcn_norm on the plan's pattern."""
    x = w_prev
    if p is not None and plan.m:
        pm = torch.zeros(plan.mu, dtype=p.dtype, device=p.device).index_add(0, plan.pgrp.long(), p)
        if plan.mean:
            pm = pm / (plan.gptr[1:] - plan.gptr[:-1]).to(p.dtype)
        fed = plan.kidx >= 0
        x = w_prev + torch.where(fed, pm[plan.kidx.clamp(min=0).long()], torch.zeros((), dtype=p.dtype, device=p.device))
    w = torch.where(x > 1, 2 - x, x)
    erow, col = plan.erow.long(), plan.col.long()
    kw = w
    if keep is not None:
        kp = torch.ones(plan.nnz, dtype=w.dtype, device=w.device)
        listed = plan.epos >= 0
        kp[listed] = keep.to(w.device, w.dtype)[plan.epos[listed].long()]
        kw = torch.where((kp == 0) & (erow == col), torch.ones_like(w), kp * w)
    deg = torch.zeros(plan.n, dtype=w.dtype, device=w.device).index_add(0, erow, kw)
    s = torch.where(deg > 0, deg.clamp(min=1e-300 if w.dtype == torch.float64 else 1e-30).pow(-0.5), torch.zeros_like(deg))
    return (s[col] * kw) * s[erow], w


class _WgcnNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, plan, w_prev, keep, p_drop, view):
        dev = w_prev.device
        w_prev = _f32c(w_prev, "w_prev")
        g = plan.graphs[view]
        new = lambda k: torch.empty(k, dtype=torch.float32, device=dev)
        w, dsign, kw, deg, s = new(plan.nnz), new(plan.nnz), new(plan.nnz), new(plan.n), new(plan.n)
        seed, step, site = 0, None, 0
        if keep is None and p_drop > 0:
            seed, step, site = dropout_state.generator(dev)
        elif keep is not None:
            keep = _f32c(keep, "keep")
            if keep.numel() != plan.ec:
                raise _lib.GdaError(f"wgcn_norm: one keep factor per listed edge ({plan.ec}) expected, got {keep.numel()}")
        ws, nbytes = _lib.scratch("gda_wgcn_workspace_bytes", dev, "wgcn", plan.n, plan.nnz)
        with profiler.region("wgcn_norm", 3, 4 * 9 * plan.nnz if profiler.enabled else 0):
            _lib.call("gda_wgcn_norm_f32", ctypes.byref(plan.struct), w_prev, None if p is None else _f32c(p.detach(), "p"),
                      keep, float(p_drop), seed, step, site, w, dsign, kw, deg, s, g.val, g.t_val, ws, nbytes,
                      _lib.stream())
        plan.gen[view] += 1                                  # the view's values changed: see _WeightedPropagate.backward
        ctx.plan = plan
        ctx.save_for_backward(kw, s, dsign)
        ctx.mark_non_differentiable(w)
        return g.val.detach(), w

    @staticmethod
    def backward(ctx, gv, _gw):
        kw, s, dsign = ctx.saved_tensors
        plan = ctx.plan
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        dp = torch.empty(plan.m, dtype=torch.float32, device=kw.device)
        ws, nbytes = _lib.scratch("gda_wgcn_workspace_bytes", kw.device, "wgcn", plan.n, plan.nnz)
        with profiler.region("wgcn_norm_bwd", 3, 4 * 8 * plan.nnz if profiler.enabled else 0):
            _lib.call("gda_wgcn_norm_bwd_f32", ctypes.byref(plan.struct), gv.contiguous(), kw, s, dsign, dp, ws, nbytes,
                      _lib.stream())
        return dp, None, None, None, None, None


def wgcn_norm(plan, w_prev, p=None, keep=None, p_drop=0.0, view=0):
    """``(val, w)``: the new raw weights ``w = fold(w_prev + P)`` per stored entry (``P`` the flip weight of the entry's
    pair; ``p=None``: the weights as they stand) and the GCN-normalised values of the graph whose dropped edges weigh 0
    -- ``keep`` one factor per listed edge (0 / 1, or the kept share of an edge that coalesces several listed copies:
    :meth:`WgcnPlan.keep_factors`), or on a device ``p_drop`` for bits from the fused-dropout stream.
    Differentiable with respect to ``p``.  Device: ``val`` is the value array of ``plan.graphs[view]``, refreshed in
    place with its by-source twin (gda_wgcn_norm_f32), and ``weighted_propagate``'s backward reads both arrays as they
    stand: a view must not be refreshed again before every backward pass over it has run (it raises if it was).  Host
    tensors take the torch composition (any dtype)."""
    if w_prev.numel() != plan.nnz or (p is not None and p.numel() != plan.m):
        raise _lib.GdaError(f"wgcn_norm: w_prev [{plan.nnz}] and p [{plan.m}] expected")
    if w_prev.device.type != plan.device.type:
        raise _lib.GdaError(f"wgcn_norm: the plan lives on {plan.device}, the weights on {w_prev.device}")
    if not w_prev.is_cuda:
        if keep is None and p_drop > 0:
            raise _lib.GdaError("wgcn_norm: host tensors need the keep mask itself")
        return _wgcn_norm_host(plan, w_prev, p, keep)
    return _WgcnNorm.apply(p, plan, w_prev, keep, float(p_drop), int(view))


class _WeightedPropagate(torch.autograd.Function):
    """``A(val) h + bias``: forward and the gradient to ``h`` are the SpMM kernels on the view's two CSRs, the gradient
    to ``val`` is the SDDMM ``<G[dst], h[src]>`` per stored entry (gda_wgcn_edge_grad_f32)."""

    @staticmethod
    def forward(ctx, h, val, bias, plan, view):
        g = plan.graphs[view]
        if val.data_ptr() != g.val.data_ptr():
            raise _lib.GdaError("weighted_propagate: val must be the array wgcn_norm refreshed for this view")
        h = _f32c(h, "h")
        ctx.plan, ctx.view, ctx.has_bias, ctx.gen = plan, view, bias is not None, plan.gen[view]
        ctx.save_for_backward(h)
        return spmm_kstep(g, h, 1, bias)

    @staticmethod
    def backward(ctx, gy):
        (h,) = ctx.saved_tensors
        plan, g = ctx.plan, ctx.plan.graphs[ctx.view]
        if plan.gen[ctx.view] != ctx.gen:
            raise _lib.GdaError("weighted_propagate: wgcn_norm refreshed this view's values between the forward and the "
                                "backward pass; the backward reads them in place (use another view)")
        gy = gy.contiguous()
        gh = spmm_kstep(g, gy, 1, None, transposed=True) if ctx.needs_input_grad[0] else None
        gval = None
        if ctx.needs_input_grad[1]:
            gval = torch.empty(plan.nnz, dtype=torch.float32, device=gy.device)
            d = h.size(1)
            with profiler.region(f"wgcn_edge_grad[d={d}]", 1, 4 * (2 * plan.nnz * d + 3 * plan.nnz) if profiler.enabled else 0,
                                 2 * plan.nnz * d):
                _lib.call("gda_wgcn_edge_grad_f32", ctypes.byref(plan.struct), gy, h, d, gval, _lib.stream())
        gb = colsum(gy) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return gh, gval, gb, None, None


def weighted_propagate(h, plan, val, bias=None, view=0):
    """``out[i] = sum over the entries e into i of val_e h[src_e] (+ bias)`` with the gradient to ``h`` and to the
    normalised values ``val`` of :func:`wgcn_norm` (and to ``bias``).  Widths up to ``WGCN_MAX_WIDTH`` on a device."""
    if h.dim() != 2 or h.size(0) != plan.n or val.numel() != plan.nnz:
        raise _lib.GdaError(f"weighted_propagate: h [{plan.n}, d] and val [{plan.nnz}] expected")
    if not h.is_cuda:
        out = torch.zeros_like(h).index_add(0, plan.erow.long(), val[:, None] * h[plan.col.long()])
        return out if bias is None else out + bias
    if h.size(1) > WGCN_MAX_WIDTH:
        raise _lib.GdaError(f"weighted_propagate: widths up to {WGCN_MAX_WIDTH}, got {h.size(1)}")
    return _WeightedPropagate.apply(h, val, bias, plan, int(view))


def _gtrans_loss_host(o1, o2, o3, margin):
    from .utils.perturb import inner, inner_margin
    a = inner(o1, o2)
    b = inner(o2, o3) if margin == -1 else inner_margin(o2, o3, margin)
    return a - b, torch.stack([a - b, a, b]).detach()


class _GtransLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o1, o2, o3, margin):
        o1, o2, o3 = (_f32c(o.detach(), "o") for o in (o1, o2, o3))
        n, d = o1.shape
        out = torch.empty(3, dtype=torch.float32, device=o1.device)
        g1, g2, g3 = torch.empty_like(o1), torch.empty_like(o1), torch.empty_like(o1)
        ws, nbytes = _lib.scratch("gda_gtrans_loss_workspace_bytes", o1.device, "gtrans_loss", n)
        with profiler.region("gtrans_loss", 2, 4 * 9 * n * d if profiler.enabled else 0):
            _lib.call("gda_gtrans_loss_f32", o1, o2, o3, n, d, margin, out, g1, g2, g3, ws, nbytes, _lib.stream())
        ctx.save_for_backward(g1, g2, g3)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, gl, _gparts):
        g1, g2, g3 = ctx.saved_tensors
        return g1 * gl, g2 * gl, g3 * gl, None


def gtrans_loss(o1, o2, o3, margin=-1):
    """GTrans's ``test_time_loss`` from the three views' outputs ``[N, d]``: ``(loss, parts)`` with ``parts = [loss,
    inner(o1, o2), inner(o2, o3)]`` -- the last ``inner_margin`` when ``margin != -1`` -- detached.  Differentiable with
    respect to all three.  Host tensors take the torch composition (any dtype)."""
    if o1.dim() != 2 or o1.shape != o2.shape or o1.shape != o3.shape:
        raise _lib.GdaError(f"gtrans_loss: three [N, d] outputs expected, got {tuple(o1.shape)}, {tuple(o2.shape)}, "
                            f"{tuple(o3.shape)}")
    if not o1.is_cuda:
        return _gtrans_loss_host(o1, o2, o3, margin)
    return _GtransLoss.apply(o1, o2, o3, float(margin))


def gtrans_project(p, n_perturbations, eps=1e-7):
    """In place and without gradient: ``p = max(p, eps)`` (the clamp that follows GTrans's Adam step), then
    ``perturb.project(n_perturbations, p, eps)``.  Device: gda_gtrans_project_f32, no host read of any sum."""
    if p.dim() != 1 or p.numel() < 1:
        raise _lib.GdaError(f"gtrans_project: a non-empty vector expected, got {tuple(p.shape)}")
    with torch.no_grad():
        if not p.is_cuda:
            from .utils.perturb import project
            p.copy_(project(n_perturbations, p.clamp(min=eps), eps))
            return p
        _f32c(p, "p")
        if not p.is_contiguous():
            raise _lib.GdaError("gtrans_project: p must be contiguous (it is updated in place)")
        ws, nbytes = _lib.scratch("gda_gtrans_project_workspace_bytes", p.device, "gtrans_project", p.numel())
        _lib.call("gda_gtrans_project_f32", p, p.numel(), float(n_perturbations), float(eps), ws, nbytes, _lib.stream())
    return p


# ------------------- GraphCTA: model loss, per-row top-(K+1), test-time loss without an [N, N] array (gda_graphcta.hip) --
CTA_MAX_CLASSES, CTA_MAX_K1 = 64, 16


def graphcta_bytes(n, f, nnz, m, d, c, k=5):
    """Device memory of a GraphCTA adaptation: ``(resident, per loss evaluation)`` bytes.  Resident: what a GTrans fit
    keeps (:func:`gtrans_bytes`) and the two memory banks ``[N, d]``, ``[N, C]``.  Per evaluation: GTrans's share, the
    model loss's workspace (the normalised features and up to eight ``[N, d]`` gradient partials, one per column split),
    the candidate lists of the top-k and the row buffers of the test-time loss -- nothing of size ``N^2``."""
    resident, per_loss = gtrans_bytes(n, f, nnz, m, d)
    splits = min(8, max(1, -(-256 // -(-n // 64))), -(-n // 64))
    return (resident + 4 * n * (d + c),
            per_loss + 4 * ((splits + 3) * n * d + (splits + 8) * n + 2 * splits * n * (k + 1) + 2 * n * (k + 1) + 2 * n * c))


def _cta_check(d, c, what):
    if d > WGCN_MAX_WIDTH or c > CTA_MAX_CLASSES:
        raise _lib.GdaError(f"{what}: widths up to {WGCN_MAX_WIDTH} and up to {CTA_MAX_CLASSES} classes, got width {d} "
                            f"and {c} classes")


def _cta_model_loss_host(feat, logits, proto, pred, tau, lamb):
    """The reference's lines (instance_proto_alignment, the weighted cross-entropy) in torch, any dtype."""
    import torch.nn.functional as F
    pred = pred.long()
    rows = torch.arange(feat.size(0), device=feat.device)
    feat_norm, center_norm = F.normalize(feat, dim=1), F.normalize(proto, dim=1)
    sim = feat_norm @ center_norm.t()
    weight = sim[rows, pred]
    sim = torch.exp(sim / tau)
    pos_sim = sim[rows, pred]
    sim_feat = torch.exp(feat_norm @ feat_norm.t() / tau)
    logit = pos_sim / (sim.sum(dim=1) - pos_sim + sim_feat.sum(dim=1) - sim_feat.diagonal() + 1e-8)
    cl = -torch.log(logit + 1e-8).mean()
    ce = F.cross_entropy(logits, pred, reduction='none')
    local = torch.sum(weight * ce) / torch.sum(weight).detach()
    loss = local * (1 - lamb) + cl * lamb
    return loss, torch.stack([loss, local, cl]).detach()


class _CtaModelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, logits, proto, pred, tau, lamb):
        feat, logits, proto = (_f32c(t.detach(), "cta_model_loss") for t in (feat, logits, proto))
        n, d = feat.shape
        c = logits.size(1)
        out = torch.empty(3, dtype=torch.float32, device=feat.device)
        dfeat, dlogits = torch.empty_like(feat), torch.empty_like(logits)
        ws, nbytes = _lib.scratch("gda_cta_loss_workspace_bytes", feat.device, "cta_loss", n, d, c)
        with profiler.region(f"cta_model_loss[d={d}]", 7, 4 * 6 * n * d if profiler.enabled else 0, 6 * n * n * d):
            _lib.call("gda_cta_model_loss_f32", feat, logits, proto, pred, n, d, c, tau, lamb, out, dfeat, dlogits, ws,
                      nbytes, _lib.stream())
        ctx.save_for_backward(dfeat, dlogits)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, gl, _gparts):
        dfeat, dlogits = ctx.saved_tensors
        return dfeat * gl, dlogits * gl, None, None, None, None


def cta_model_loss(feat, logits, proto, pred, tau=0.2, lamb=0.2):
    """GraphCTA's model loss: ``(loss, parts)`` with ``parts = [loss, loss_local, cl]`` detached -- ``cl`` the
    instance-prototype contrast of ``instance_proto_alignment(feat [N, d], proto [C, d], pred [N])``, ``loss_local`` the
    cross-entropy of ``logits [N, C]`` against ``pred`` weighted by the cosine to the predicted prototype and divided by
    the (constant, unguarded) sum of the weights, ``loss = (1 - lamb) loss_local + lamb cl``.  Differentiable with respect
    to ``feat`` and ``logits``; ``proto`` is a constant.  Device: gda_cta_model_loss_f32, which streams ``F^ F^^T`` twice
    and stores no ``[N, N]`` array.  Host tensors take the torch composition (any dtype)."""
    if feat.dim() != 2 or logits.dim() != 2 or proto.dim() != 2 or feat.size(0) != logits.size(0) \
            or proto.shape != (logits.size(1), feat.size(1)) or pred.shape != (feat.size(0),):
        raise _lib.GdaError(f"cta_model_loss: feat [N, d], logits [N, C], proto [C, d], pred [N] expected, got "
                            f"{tuple(feat.shape)}, {tuple(logits.shape)}, {tuple(proto.shape)}, {tuple(pred.shape)}")
    if not feat.is_cuda:
        return _cta_model_loss_host(feat, logits, proto, pred, tau, lamb)
    _cta_check(feat.size(1), logits.size(1), "cta_model_loss")
    return _CtaModelLoss.apply(feat, logits, proto, pred.to(torch.int32).contiguous(), float(tau), float(lamb))


def cta_knn(feat, mem, k1):
    """``(idx [N, k1], val [N, k1])``: per row of ``feat [N, d]`` the ``k1`` rows of ``mem [Nm, d]`` of largest inner
    product, values descending, ties to the lower index.  No gradient.  A NaN product ranks as +inf, as in
    ``torch.topk``; the device kernel also RETURNS +inf for it in ``val`` (torch and the host fallback return the NaN).  Device: gda_cta_knn_f32 (int32 indices, no
    ``[N, Nm]`` array); host tensors: a stable descending sort of ``feat mem^T`` (int64 indices, any dtype)."""
    if feat.dim() != 2 or mem.dim() != 2 or feat.size(1) != mem.size(1):
        raise _lib.GdaError(f"cta_knn: feat [N, d] and mem [Nm, d] expected, got {tuple(feat.shape)}, {tuple(mem.shape)}")
    k1 = int(k1)
    if k1 < 1 or mem.size(0) < k1:
        raise _lib.GdaError(f"cta_knn: k1 = {k1} out of range for {mem.size(0)} memory rows")
    with torch.no_grad():
        if not feat.is_cuda:
            val, idx = torch.sort(feat @ mem.t(), dim=1, descending=True, stable=True)
            return idx[:, :k1].contiguous(), val[:, :k1].contiguous()
        if k1 > CTA_MAX_K1:
            raise _lib.GdaError(f"cta_knn: up to {CTA_MAX_K1} neighbours, got {k1}")
        _cta_check(feat.size(1), 1, "cta_knn")
        feat, mem = _f32c(feat.detach(), "feat"), _f32c(mem.detach(), "mem")
        n, d = feat.shape
        idx = torch.empty(n, k1, dtype=torch.int32, device=feat.device)
        val = torch.empty(n, k1, dtype=torch.float32, device=feat.device)
        ws, nbytes = _lib.scratch("gda_cta_knn_workspace_bytes", feat.device, "cta_knn", n, mem.size(0), k1)
        with profiler.region(f"cta_knn[d={d}]", 2, 4 * 2 * n * d if profiler.enabled else 0, 2 * n * mem.size(0) * d):
            _lib.call("gda_cta_knn_f32", feat, mem, n, mem.size(0), d, k1, idx, val, ws, nbytes, _lib.stream())
    return idx, val


def first_argmax(x):
    """The first index of every row's maximum: torch's CPU rule for ties, which ``argmax`` on a device does not
    promise.  GraphCTA's class memory starts at exactly ``1 / C``, every row a tie."""
    c = x.size(1)
    cols = torch.arange(c, device=x.device).expand_as(x)
    return torch.where(x == x.max(dim=1, keepdim=True).values, cols, torch.full_like(cols, c - 1)).min(dim=1).values


def _cta_class_sums(x, idx, c):
    """``(sum [C, d], count [C])`` of the rows of ``x`` per class ``idx``: the ordered grouped sum of the SEPA kernels up
    to their class limit, the one-hot product on the project's GEMM beyond (and torch on the host)."""
    if x.is_cuda and c <= SEPA_MAX_CLASSES:
        return _sepa_group_sum(_f32c(x, "x"), idx.to(torch.int32).contiguous(), c)
    onehot = (idx[:, None] == torch.arange(c, device=idx.device)[None, :]).to(x.dtype)
    return mat_tn(onehot, x.contiguous()), onehot.sum(dim=0)


def _cta_memory_classes(mem_fea, mem_cls):
    """``(csum [C, d], ccnt [C])``: the memory rows summed per arg-max class of ``mem_cls``, and how many each has."""
    return _cta_class_sums(mem_fea, first_argmax(mem_cls), mem_cls.size(1))


def cta_prototypes(mem_fea, idx, num_classes):
    """GraphCTA's prototypes ``(mem_fea^T onehot(idx) / (count + 1e-8))^T`` ``[C, d]``; no gradient."""
    with torch.no_grad():
        csum, ccnt = _cta_class_sums(mem_fea, idx, int(num_classes))
        return csum / (ccnt + 1e-8)[:, None]


def _cta_test_time_host(logits, feat, mem_fea, mem_cls, idx_near):
    import torch.nn.functional as F
    n, c = logits.shape
    p = F.softmax(logits, dim=1)
    pred = p.argmax(dim=1)
    ent = -(p * torch.log(p + 1e-8)).sum(dim=1)
    est_p = (ent < ent.mean()).sum().double() / n
    by_ent = torch.sort(ent.detach(), stable=True).indices            # (entropy, index)
    grouped = by_ent[torch.sort(pred[by_ent], stable=True).indices]   # ... within the predicted class
    cnum = torch.bincount(pred, minlength=c)
    start = torch.cumsum(cnum, 0) - cnum
    rank = torch.empty(n, dtype=torch.long)
    rank[grouped] = torch.arange(n) - start[pred[grouped]]
    quota = (cnum.double() * est_p / 5).long()                        # int(c_num * est_p / 5), float64
    sel = rank < quota[pred]
    ce = F.cross_entropy(logits[sel], pred[sel])
    k = idx_near.size(1) - 1
    near = mem_fea[idx_near[:, 1:].long()]
    nb = ((feat.unsqueeze(1) * near).sum(-1).sum(1) / k).mean()
    csum, ccnt = _cta_memory_classes(mem_fea, mem_cls)
    other = (1 - torch.eye(c, dtype=csum.dtype)) @ csum               # the other classes' sums, not total - own
    neg = mem_fea.size(0) - ccnt[pred]
    ng = ((feat * other[pred]).sum(dim=1) / neg).mean()
    loss = ce - nb * 0.1 + ng * 0.1
    return loss, torch.stack([loss, ce, nb, ng]).detach(), pred, sel


class _CtaTestTime(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, feat, mem_fea, idx_near, csum, ccnt):
        logits, feat = _f32c(logits.detach(), "logits"), _f32c(feat.detach(), "feat")
        n, c = logits.shape
        d, nm, k1 = feat.size(1), mem_fea.size(0), idx_near.size(1)
        dev = feat.device
        out = torch.empty(4, dtype=torch.float32, device=dev)
        dlogits, dfeat = torch.empty_like(logits), torch.empty_like(feat)
        pred, sel = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        ws, nbytes = _lib.scratch("gda_cta_tt_workspace_bytes", dev, "cta_tt", n, d, c)
        with profiler.region(f"cta_test_time[d={d}]", 6, 4 * (k1 + 2) * n * d if profiler.enabled else 0):
            _lib.call("gda_cta_test_time_f32", logits, feat, mem_fea, idx_near, csum, ccnt, n, nm, d, c, k1, out, dlogits,
                      dfeat, pred, sel, ws, nbytes, _lib.stream())
        ctx.save_for_backward(dlogits, dfeat)
        ctx.mark_non_differentiable(out, pred, sel)
        return out[0].clone(), out, pred, sel

    @staticmethod
    def backward(ctx, gl, *_):
        dlogits, dfeat = ctx.saved_tensors
        return dlogits * gl, dfeat * gl, None, None, None, None


def cta_test_time_loss(logits, feat, mem_fea, mem_cls, idx_near):
    """The rest of GraphCTA's ``test_time_loss`` from the classifier's ``logits [N, C]``, the bottleneck's output
    ``feat [N, d]``, the memory banks ``mem_fea [Nm, d]``, ``mem_cls [Nm, C]`` and ``idx_near [N, K + 1]`` of
    :func:`cta_knn` (rank 1 is dropped, whichever row it is): ``(loss, parts, pred, selected)`` with ``parts = [loss,
    ce, nb, ng]`` detached and ``loss = ce - 0.1 nb + 0.1 ng`` -- the cross-entropy of the per class
    ``int(c_num * est_p / 5)`` rows of lowest ``(entropy, index)`` against their own arg-max (NaN when none is selected),
    the mean inner product with the ``K`` neighbours, the mean inner product with the memory rows of the other classes
    (0 / 0 = NaN when the memory holds one class).  Differentiable with respect to ``logits`` and ``feat``; the banks and
    every discrete choice carry no gradient.  Device: gda_cta_test_time_f32, no host read (``pred``, ``selected`` int32);
    host tensors take the torch composition (any dtype; int64 / bool)."""
    if logits.dim() != 2 or feat.dim() != 2 or mem_fea.dim() != 2 or logits.size(0) != feat.size(0) \
            or mem_fea.size(1) != feat.size(1) or mem_cls.shape != (mem_fea.size(0), logits.size(1)) \
            or idx_near.dim() != 2 or idx_near.size(0) != feat.size(0) or idx_near.size(1) < 2:
        raise _lib.GdaError(f"cta_test_time_loss: logits [N, C], feat [N, d], mem_fea [Nm, d], mem_cls [Nm, C], idx_near "
                            f"[N, K + 1] expected, got {tuple(logits.shape)}, {tuple(feat.shape)}, {tuple(mem_fea.shape)}, "
                            f"{tuple(mem_cls.shape)}, {tuple(idx_near.shape)}")
    if not feat.is_cuda:
        return _cta_test_time_host(logits, feat, mem_fea, mem_cls, idx_near)
    if idx_near.size(1) > CTA_MAX_K1:
        raise _lib.GdaError(f"cta_test_time_loss: up to {CTA_MAX_K1} neighbours, got {idx_near.size(1)}")
    _cta_check(feat.size(1), logits.size(1), "cta_test_time_loss")
    with torch.no_grad():
        mem_fea = _f32c(mem_fea.detach(), "mem_fea")
        csum, ccnt = _cta_memory_classes(mem_fea, mem_cls.detach())
    return _CtaTestTime.apply(logits, feat, mem_fea, idx_near.to(torch.int32).contiguous(), _f32c(csum, "csum"),
                              _f32c(ccnt, "ccnt"))


# ------------------- KBL: the pair-similarity loss and the global bridge top-k without their big arrays (gda_kbl.hip) --
KBL_MAX_WIDTH, KBL_MAX_PAIR_ROWS, KBL_MAX_K = 256, 1024, 256


def _kbl_pair_bce_host(u, ia, ib, y):
    """The reference's lines in torch, any dtype: the two ``[ma mb]`` gathers, ``CosineSimilarity``, the sigmoid,
    ``binary_cross_entropy``.  The pair ``(p, q)`` sits at ``q ma + p``, the reference's ``pair_enumeration``."""
    import torch.nn.functional as F
    i1, i2 = ia.long().repeat(ib.numel()), ib.long().repeat_interleave(ia.numel())
    probs = torch.sigmoid(F.cosine_similarity(u[i1], u[i2], dim=1))
    return F.binary_cross_entropy(probs, (y[i1] == y[i2]).to(u.dtype))


class _KblPairBce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, ia, ib, y):
        u = _f32c(u.detach(), "kbl_pair_bce")
        n, d = u.shape
        out = torch.empty(1, dtype=torch.float32, device=u.device)
        du = torch.empty_like(u)
        ws, nbytes = _lib.scratch("gda_kbl_pair_bce_workspace_bytes", u.device, "kbl_pair", d, ia.numel(), ib.numel())
        with profiler.region(f"kbl_pair_bce[d={d}]", 6, 4 * 2 * n * d if profiler.enabled else 0,
                             6 * ia.numel() * ib.numel() * d):
            _lib.call("gda_kbl_pair_bce_f32", u, ia, ib, y, n, d, ia.numel(), ib.numel(), out, du, ws, nbytes,
                      _lib.stream())
        ctx.save_for_backward(du)
        return out[0].clone()

    @staticmethod
    def backward(ctx, gl):
        (du,) = ctx.saved_tensors
        return du * gl, None, None, None


def kbl_pair_bce(u, ia, ib, y):
    """KBL's ``loss_sim_within_src``: the mean over all ``ma mb`` pairs of ``BCE(sigmoid(cos(u[ia[p]], u[ib[q]])),
    [y[ia[p]] == y[ib[q]]])`` for ``u [n, d]``, index lists ``ia [ma]``, ``ib [mb]`` (entries may repeat) and labels
    ``y [n]``; cosine and BCE as torch defines them (norms clamped at 1e-8, logarithms at -100).  Differentiable with
    respect to ``u``.  Device: gda_kbl_pair_bce_f32 (``d <= 256``, ``ma, mb <= 1024``), which never forms the
    ``[ma mb, d]`` gathers; host tensors take the torch composition (any dtype)."""
    if u.dim() != 2 or ia.dim() != 1 or ib.dim() != 1 or y.shape != (u.size(0),) or ia.numel() < 1 or ib.numel() < 1:
        raise _lib.GdaError(f"kbl_pair_bce: u [n, d], ia [ma], ib [mb], y [n] expected, got {tuple(u.shape)}, "
                            f"{tuple(ia.shape)}, {tuple(ib.shape)}, {tuple(y.shape)}")
    if not u.is_cuda:
        return _kbl_pair_bce_host(u, ia, ib, y)
    return _KblPairBce.apply(u, ia.to(torch.int32).contiguous(), ib.to(torch.int32).contiguous(),
                             y.to(torch.int32).contiguous())


def _kbl_bridge_topk_chunked(a, b, k, rows=1024):
    """The reference's formulation, a chunk of rows at a time: the cosine of ``rows`` rows of ``a`` against all of
    ``b``, the chunk's candidates joined to the running ``k`` and cut back by (cosine descending, flat index
    ascending).  Stores ``[rows, nb]``, never ``[na, nb]``."""
    na, nb = a.size(0), b.size(0)
    ah = a / a.norm(dim=1, keepdim=True).clamp_min(1e-8)
    bh = b / b.norm(dim=1, keepdim=True).clamp_min(1e-8)
    val = torch.empty(0, dtype=a.dtype, device=a.device)
    flat = torch.empty(0, dtype=torch.long, device=a.device)
    for i0 in range(0, na, rows):
        c = torch.nan_to_num(ah[i0:i0 + rows] @ bh.t(), nan=float("inf"), posinf=float("inf"), neginf=float("-inf"))
        c = c.reshape(-1)
        kk = min(k, c.numel())
        idx = (c >= torch.topk(c, kk).values[-1]).nonzero().squeeze(1)       # ascending: every tie of the k-th is in
        val, flat = torch.cat([val, c[idx]]), torch.cat([flat, idx + i0 * nb])
        order = torch.sort(val, descending=True, stable=True).indices[:k]   # flat is ascending within equal values
        val, flat = val[order], flat[order]
    return flat // nb, flat % nb, torch.sigmoid(val)


def kbl_bridge_topk(a, b, k):
    """KBL's bridge edges: ``(row [k], col [k], val [k])``, the ``k`` pairs of largest ``cos(a[i], b[j])`` over all
    ``na nb`` pairs of ``a [na, d]``, ``b [nb, d]`` with ``val = sigmoid(cos)``, ordered by (cosine descending, flat
    index ``i nb + j`` ascending); NaN counts as +inf.  No gradient.  Device, ``k <= 256``: gda_kbl_bridge_topk_f32
    (int32 indices, no ``[na, nb]`` array); a larger ``k`` on the device and host tensors (any dtype) take the
    row-chunked torch path, which stores no full array either (int64 indices)."""
    if a.dim() != 2 or b.dim() != 2 or a.size(1) != b.size(1) or a.size(0) < 1 or b.size(0) < 1 or a.size(1) < 1:
        raise _lib.GdaError(f"kbl_bridge_topk: a [na, d] and b [nb, d] expected, got {tuple(a.shape)}, {tuple(b.shape)}")
    k = int(k)
    if k < 1 or k > a.size(0) * b.size(0):
        raise _lib.GdaError(f"kbl_bridge_topk: k = {k} out of range for {a.size(0)} x {b.size(0)} pairs")
    with torch.no_grad():
        if not a.is_cuda or k > KBL_MAX_K:
            return _kbl_bridge_topk_chunked(a.detach(), b.detach(), k)
        a, b = _f32c(a.detach(), "a"), _f32c(b.detach(), "b")
        na, nb, d = a.size(0), b.size(0), a.size(1)
        row, col = (torch.empty(k, dtype=torch.int32, device=a.device) for _ in range(2))
        val = torch.empty(k, dtype=torch.float32, device=a.device)
        ws, nbytes = _lib.scratch("gda_kbl_bridge_topk_workspace_bytes", a.device, "kbl_topk", na, nb, d, k)
        with profiler.region(f"kbl_bridge_topk[d={d}]", 4, 4 * 2 * (na + nb) * d if profiler.enabled else 0, 2 * na * nb * d):
            _lib.call("gda_kbl_bridge_topk_f32", a, b, na, nb, d, k, row, col, val, ws, nbytes, _lib.stream())
    return row, col, val


# ------------------- GraphATA: gate, sparsemax blend, head loss, memory vote and update (gda_graphata.hip) --
ATA_MAX_SOURCES, ATA_MAX_CLASSES = 8, 64


class _SparsemaxHost(torch.autograd.Function):
    """The reference's ``SparsemaxFunction`` over dim 1 of a 2-D input in torch (any dtype, either device), without its
    in-place shift of the caller's tensor."""

    @staticmethod
    def forward(ctx, a):
        z = a - a.max(dim=1, keepdim=True).values
        srt = torch.sort(z, descending=True, dim=1).values
        cumsum = srt.cumsum(1) - 1
        rhos = torch.arange(1, a.size(1) + 1, device=a.device, dtype=a.dtype)[None, :]
        supp = (rhos * srt > cumsum).sum(dim=1, keepdim=True)
        tau = cumsum.gather(1, supp - 1) / supp.to(a.dtype)
        out = torch.clamp(z - tau, min=0)
        ctx.save_for_backward(supp, out)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        supp, out = ctx.saved_tensors
        grad = grad_output.clone()
        grad[out == 0] = 0
        v_hat = grad.sum(dim=1, keepdim=True) / supp.to(out.dtype)
        return torch.where(out != 0, grad - v_hat, grad)


def _ata_sources(s, what):
    if s > ATA_MAX_SOURCES:
        raise _lib.GdaError(f"{what}: up to {ATA_MAX_SOURCES} sources on the device, got {s}")


class _Sparsemax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        a = _f32c(a.detach(), "sparsemax")
        w = torch.empty_like(a)
        _lib.call("gda_ata_sparsemax_f32", a, a.size(0), a.size(1), w, _lib.stream())
        ctx.save_for_backward(w)
        return w

    @staticmethod
    def backward(ctx, dw):
        (w,) = ctx.saved_tensors
        da = torch.empty_like(w)
        _lib.call("gda_ata_sparsemax_bwd_f32", w, _f32c(dw, "dw"), w.size(0), w.size(1), da, _lib.stream())
        return da


def sparsemax(a, host=False):
    """Sparsemax over the columns of ``a [N, S]`` as the reference's ``SparsemaxFunction`` computes it (subtract the row
    maximum, sort descending, support ``#{k : k z_(k) > cumsum_k - 1}``, ``tau = (cumsum_support - 1) / support``,
    ``max(z - tau, 0)``), differentiable.  Device: gda_ata_sparsemax_f32 (``S <= 8``); host tensors, and any tensor with
    ``host=True``, take the torch composition (any dtype)."""
    if a.dim() != 2 or a.size(0) < 1 or a.size(1) < 1:
        raise _lib.GdaError(f"sparsemax: a [N, S] expected, got {tuple(a.shape)}")
    if host or not a.is_cuda:
        return _SparsemaxHost.apply(a)
    _ata_sources(a.size(1), "sparsemax")
    return _Sparsemax.apply(a)


class _AtaGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nr):
        nr = _f32c(nr.detach(), "ata_gate")
        g = torch.empty_like(nr)
        _lib.call("gda_ata_gate_f32", nr, g, nr.numel(), _lib.stream())
        ctx.save_for_backward(nr)
        return g

    @staticmethod
    def backward(ctx, dg):
        (nr,) = ctx.saved_tensors
        dnr = torch.empty_like(nr)
        _lib.call("gda_ata_gate_bwd_f32", nr, _f32c(dg, "dg"), None, dnr, nr.numel(), _lib.stream())
        return dnr


def ata_gate(nr, host=False):
    """``sigmoid(nr) * nr``: what NodeCentricConv's gated mean aggregation ``propagate(x, gamma=sigmoid(nr))`` equals
    row by row when ``nr`` is the mean aggregation over the same edge list.  Device: gda_ata_gate_f32."""
    if nr.numel() < 1:
        raise _lib.GdaError(f"ata_gate: a non-empty tensor expected, got {tuple(nr.shape)}")
    if host or not nr.is_cuda:
        return torch.sigmoid(nr) * nr
    return _AtaGate.apply(nr)


class _AtaMix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, Q, a, lamb):
        P, Q, a = (_f32c(t.detach(), "ata_mix") for t in (P, Q, a))
        n, h = Q.shape
        s = a.size(1)
        y, w = torch.empty_like(Q), torch.empty_like(a)
        with profiler.region(f"ata_mix[h={h}]", 1, 4 * (s + 2) * n * h if profiler.enabled else 0):
            _lib.call("gda_ata_mix_f32", P, Q, a, n, h, s, lamb, y, w, _lib.stream())
        ctx.save_for_backward(P, w)
        ctx.lamb = lamb
        ctx.mark_non_differentiable(w)
        return y, w

    @staticmethod
    def backward(ctx, gy, _gw):
        P, w = ctx.saved_tensors
        n, s = w.shape
        h = P.size(1) // s
        gy = _f32c(gy, "gy")
        dP = torch.empty_like(P)
        dQ = torch.empty(n, h, dtype=torch.float32, device=P.device)
        da = torch.empty_like(w)
        with profiler.region(f"ata_mix_bwd[h={h}]", 1, 4 * (2 * s + 2) * n * h if profiler.enabled else 0):
            _lib.call("gda_ata_mix_bwd_f32", gy, P, w, n, h, s, ctx.lamb, dP, dQ, da, _lib.stream())
        return dP, dQ, da, None


def ata_mix(P, Q, a, lamb=0.2, host=False):
    """The blend of a NodeCentricConv layer: ``(y, w)`` with ``w = sparsemax(a)`` over the ``S`` sources (detached) and
    ``y = sum_s w_s P_s + lamb Q`` for ``P [N, S h]`` (block ``s`` the projection by source ``s``), ``Q [N, h]``,
    ``a [N, S]``.  Differentiable with respect to ``P``, ``Q`` and ``a``.  Device: gda_ata_mix_f32 / _bwd_f32 (``S <=
    8``, ``h <= 256``); host tensors (and ``host=True``) take the torch composition (any dtype)."""
    if P.dim() != 2 or Q.dim() != 2 or a.dim() != 2 or Q.size(0) != P.size(0) or a.size(0) != P.size(0) \
            or a.size(1) < 1 or P.size(1) != a.size(1) * Q.size(1) or P.size(0) < 1 or Q.size(1) < 1:
        raise _lib.GdaError(f"ata_mix: P [N, S h], Q [N, h], a [N, S] expected, got {tuple(P.shape)}, {tuple(Q.shape)}, "
                            f"{tuple(a.shape)}")
    if host or not P.is_cuda:
        n, h = Q.shape
        w = sparsemax(a, host=True)
        gamma = P.view(n, a.size(1), h).transpose(0, 1)
        return torch.sum(w.t().unsqueeze(-1) * gamma, dim=0) + Q * lamb, w.detach()
    _ata_sources(a.size(1), "ata_mix")
    if Q.size(1) > WGCN_MAX_WIDTH:
        raise _lib.GdaError(f"ata_mix: widths up to {WGCN_MAX_WIDTH}, got {Q.size(1)}")
    return _AtaMix.apply(P, Q, a, float(lamb))


def _ata_head_layout(Z):
    """``(tensor to pass, src_stride, row_stride)`` of ``Z [S, N, C]``: the column blocks of an ``[N, S C]`` array are
    taken as they lie, anything else is made contiguous."""
    s, n, c = Z.shape
    if Z.stride() == (c, s * c, 1) and s > 1:
        return Z, c, s * c
    return Z.contiguous(), n * c, c


class _AtaHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z, att, pred):
        Z, zs, zr = _ata_head_layout(_lib.require_gpu_tensor(Z.detach(), "Z", torch.float32))
        s, n, c = Z.shape
        a = _f32c(att.detach().reshape(-1), "att")
        dev = Z.device
        logits = torch.empty(n, c, dtype=torch.float32, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        datt = torch.empty(c, dtype=torch.float32, device=dev)
        if zs == c:                                                        # the blocks of an [N, S C] array
            dZ = torch.empty(n, s * c, dtype=torch.float32, device=dev).view(n, s, c).transpose(0, 1)
        else:
            dZ = torch.empty(s, n, c, dtype=torch.float32, device=dev)
        ws, nbytes = _lib.scratch("gda_ata_head_workspace_bytes", dev, "ata_head", n, c)
        with profiler.region(f"ata_head[C={c}]", 4, 4 * 3 * s * n * c if profiler.enabled else 0):
            _lib.call("gda_ata_head_f32", Z, zs, zr, a, pred, n, c, s, logits, out, dZ, datt, ws, nbytes, _lib.stream())
        ctx.save_for_backward(dZ, datt)
        ctx.att_shape = att.shape
        ctx.mark_non_differentiable(out, logits)
        return out[0].clone(), out, logits

    @staticmethod
    def backward(ctx, gl, *_):
        dZ, datt = ctx.saved_tensors
        return dZ * gl, (datt * gl).reshape(ctx.att_shape), None


def _ata_head_host(Z, att, pred):
    """NodeCentricMLP's blend and the loss of graphata.py:423-437 in torch (any dtype)."""
    import torch.nn.functional as F
    att = att.reshape(-1, 1)
    scores = torch.cat([torch.matmul(Z[s], att) for s in range(Z.size(0))], dim=1)
    w = sparsemax(scores, host=True)
    logits = torch.sum(w.t().unsqueeze(-1) * Z, dim=0)
    if pred is None:
        return logits
    softmax_out = F.softmax(logits, dim=1)
    ent = torch.mean(torch.sum(-softmax_out * torch.log(softmax_out + 1e-8), dim=1))
    mean_softmax = softmax_out.mean(dim=0)
    div = torch.sum(mean_softmax * torch.log(mean_softmax + 1e-5))
    ce = F.cross_entropy(logits, pred.long())
    loss = ent + div + ce
    return loss, torch.stack([loss, ent, div, ce]).detach(), logits.detach()


def ata_head_loss(Z, att, pred=None, host=False):
    """GraphATA's head from the ``S`` classifier outputs ``Z [S, N, C]`` (a view of the column blocks of an ``[N, S C]``
    array is read in place), NodeCentricMLP's ``att [C]`` or ``[C, 1]`` and the pseudo labels ``pred [N]``:
    ``w = sparsemax_s(<Z_si, att>)``, ``logits = sum_s w_s Z_s`` and ``(loss, parts, logits)`` with ``parts = [loss,
    ent, div, ce]`` detached -- ``ent = mean_i -sum_c p log(p + 1e-8)``, ``div = sum_c m_c log(m_c + 1e-5)``, ``ce`` the
    cross-entropy against ``pred``, ``loss`` their sum.  Differentiable with respect to ``Z`` and ``att``; ``logits``
    comes back detached.  With ``pred=None`` the logits alone are returned, without a gradient (the eval pass).
    Device: gda_ata_head_f32 (``S <= 8``, ``C <= 64``); host tensors (and ``host=True``): the torch composition, any
    dtype, whose ``pred=None`` logits stay differentiable."""
    if Z.dim() != 3 or att.numel() != Z.size(2) or min(Z.shape) < 1 \
            or (pred is not None and pred.shape != (Z.size(1),)):
        raise _lib.GdaError(f"ata_head_loss: Z [S, N, C], att [C], pred [N] expected, got {tuple(Z.shape)}, "
                            f"{tuple(att.shape)}, {None if pred is None else tuple(pred.shape)}")
    if host or not Z.is_cuda:
        return _ata_head_host(Z, att, pred)
    _ata_sources(Z.size(0), "ata_head_loss")
    if Z.size(2) > ATA_MAX_CLASSES:
        raise _lib.GdaError(f"ata_head_loss: up to {ATA_MAX_CLASSES} classes on the device, got {Z.size(2)}")
    if pred is None:
        with torch.no_grad():
            Zc, zs, zr = _ata_head_layout(_lib.require_gpu_tensor(Z.detach(), "Z", torch.float32))
            s, n, c = Zc.shape
            logits = torch.empty(n, c, dtype=torch.float32, device=Z.device)
            _lib.call("gda_ata_head_f32", Zc, zs, zr, _f32c(att.detach().reshape(-1), "att"), None, n, c, s, logits, None,
                      None, None, None, 0, _lib.stream())
        return logits
    return _AtaHead.apply(Z, att, pred.to(torch.int32).contiguous())


def ata_vote(nn_idx, mem_cls, host=False):
    """GraphATA's pseudo labels: per row of ``nn_idx [N, K + 1]`` (:func:`cta_knn`'s; rank 1 is dropped whichever row
    it is) the FIRST arg-max of the mean of ``mem_cls [Nm, C]`` over the remaining ``K`` rows -- torch's CPU rule for
    ties, which decides every row while the memory still holds exactly ``1 / C``.  No gradient.  Device:
    gda_ata_vote_f32 (int32, an index outside ``[0, Nm)`` adds nothing); host tensors: the torch composition (int64)."""
    if nn_idx.dim() != 2 or mem_cls.dim() != 2 or nn_idx.size(1) < 2 or nn_idx.size(0) < 1 or min(mem_cls.shape) < 1:
        raise _lib.GdaError(f"ata_vote: nn_idx [N, K + 1] with K >= 1 and mem_cls [Nm, C] expected, got "
                            f"{tuple(nn_idx.shape)}, {tuple(mem_cls.shape)}")
    with torch.no_grad():
        if host or not mem_cls.is_cuda:
            return first_argmax(torch.mean(mem_cls[nn_idx[:, 1:].long()], dim=1))
        if nn_idx.size(1) > CTA_MAX_K1 or mem_cls.size(1) > ATA_MAX_CLASSES:
            raise _lib.GdaError(f"ata_vote: up to {CTA_MAX_K1 - 1} neighbours and {ATA_MAX_CLASSES} classes on the "
                                f"device, got {nn_idx.size(1) - 1} and {mem_cls.size(1)}")
        mem_cls = _f32c(mem_cls.detach(), "mem_cls")
        n, k1 = nn_idx.shape
        pred = torch.empty(n, dtype=torch.int32, device=mem_cls.device)
        _lib.call("gda_ata_vote_f32", nn_idx.to(torch.int32).contiguous(), mem_cls, n, mem_cls.size(0), mem_cls.size(1),
                  k1, pred, _lib.stream())
    return pred


def ata_memory_update(logits, feat, mem_cls, mem_fea, momentum=0.9, host=False):
    """GraphATA's memory update, in place and without a gradient: with ``p = softmax(logits [N, C])`` and ``q = p^2 /
    sum_i p^2``, ``mem_cls <- (1 - momentum) mem_cls + momentum q`` and ``mem_fea <- (1 - momentum) mem_fea + momentum
    feat`` (``feat``, ``mem_fea`` ``[N, d]``).  Device: gda_ata_memory_f32, the column sums in two ordered phases; host
    tensors: the reference's lines (any dtype)."""
    if logits.dim() != 2 or feat.dim() != 2 or mem_cls.shape != logits.shape or mem_fea.shape != feat.shape \
            or feat.size(0) != logits.size(0) or min(logits.shape) < 1 or feat.size(1) < 1:
        raise _lib.GdaError(f"ata_memory_update: logits / mem_cls [N, C] and feat / mem_fea [N, d] expected, got "
                            f"{tuple(logits.shape)}, {tuple(mem_cls.shape)}, {tuple(feat.shape)}, {tuple(mem_fea.shape)}")
    with torch.no_grad():
        if host or not logits.is_cuda:
            softmax_out = torch.softmax(logits, dim=1)
            outputs_target = softmax_out ** 2 / ((softmax_out ** 2).sum(dim=0))
            mem_cls.copy_((1.0 - momentum) * mem_cls + momentum * outputs_target)
            mem_fea.copy_((1.0 - momentum) * mem_fea + momentum * feat)
            return
        n, c = logits.shape
        d = feat.size(1)
        if c > ATA_MAX_CLASSES or d > WGCN_MAX_WIDTH:
            raise _lib.GdaError(f"ata_memory_update: up to {ATA_MAX_CLASSES} classes and widths up to {WGCN_MAX_WIDTH} on "
                                f"the device, got {c} and {d}")
        for t, name in ((mem_cls, "mem_cls"), (mem_fea, "mem_fea")):
            if _f32c(t, name).data_ptr() != t.data_ptr():
                raise _lib.GdaError(f"ata_memory_update: {name} is updated in place and must be contiguous")
        ws, nbytes = _lib.scratch("gda_ata_memory_workspace_bytes", logits.device, "ata_memory", n, c)
        _lib.call("gda_ata_memory_f32", _f32c(logits.detach(), "logits"), _f32c(feat.detach(), "feat"), n, c, d,
                  1.0 - momentum, momentum, mem_cls, mem_fea, ws, nbytes, _lib.stream())


# ------------------------------------------------------------------------------------------------ PairAlign --
PA_MAX_CLASSES = 24               # GDA_PA_MAX_CLASSES: 8 C^2 K + 64 C K + 32 C bytes of LDS at C = K, 144.75 of 160 KiB
PA_SEGMENT = 64                   # GDA_PA_SEGMENT: neighbours of one row per lane group (a hub row is cut into these)
PA_MAX_ITEMS = 4096               # GDA_PA_MAX_ITEMS
_PA_ITEMS = 256                   # workgroups a plan aims at: one per CU


def _pa_check_classes(c, k, what):
    if c > PA_MAX_CLASSES or k > PA_MAX_CLASSES:
        raise _lib.GdaError(f"{what}: up to {PA_MAX_CLASSES} classes, got {max(c, k)}")


def _pa_cls(cls, n, k, dev, what):
    """``cls`` as a checked int64 device vector, or None where every row is class 0."""
    if cls is None:
        if k != 1:
            raise ValueError(f"{what}: classes are required for K = {k}")
        return None
    cls = cls.to(dev, torch.int64).contiguous()
    if cls.dim() != 1 or cls.numel() != n:
        raise ValueError(f"{what}: cls [N = {n}] expected, got {tuple(cls.shape)}")
    if n and (int(cls.min()) < 0 or int(cls.max()) >= k):
        raise ValueError(f"{what}: a class is outside [0, {k})")
    return cls


def _pa_items(counts, per_item):
    """``(slot, lo, hi)`` runs of at most ``per_item`` over consecutive per-slot counts, and the slot pointer."""
    items, ptr, at = [], [0], 0
    for slot, cnt in enumerate(counts):
        for lo in range(0, cnt, per_item):
            items.append((slot, at + lo, at + min(lo + per_item, cnt)))
        at += cnt
        ptr.append(len(items))
    return items, ptr


class PaEdgePlan:
    """The work lists of :func:`pa_edge_stats` for one graph (see PLANS in include/gda_hip.h): the unweighted CSR with
    rows = ``edge_index[0]`` (duplicates kept, no self loops added), its rows bucketed by class and cut into segments of
    at most ``PA_SEGMENT`` neighbours.  Built once per fit -- the labels never change -- with one small read-back.  The
    largest array beside the CSR itself is the segment list: one entry per non-empty row plus one per ``PA_SEGMENT``
    further neighbours of a hub row."""

    def __init__(self, edge_index, n, cls=None, K=1):
        dev = edge_index.device
        _pa_check_classes(1, K, "PaEdgePlan")
        self.n, self.K, self.cls = int(n), int(K), _pa_cls(cls, n, K, dev, "PaEdgePlan")
        self.num_edges = int(edge_index.size(1))
        g = build_csr(torch.stack([edge_index[1], edge_index[0]]), n, None, add_self_loops=False, normalize=False)
        self.rowptr, self.colidx = g.rowptr, g.colidx
        rp = g.rowptr.to(torch.int64)
        deg = rp[1:n + 1] - rp[:n]
        order = torch.arange(n, device=dev) if self.cls is None else torch.argsort(self.cls, stable=True)
        order = order[deg[order] > 0]
        nseg = (deg[order] + PA_SEGMENT - 1) // PA_SEGMENT
        row = torch.repeat_interleave(order, nseg)
        first = torch.cumsum(nseg, 0) - nseg
        k = torch.arange(row.numel(), device=dev) - torch.repeat_interleave(first, nseg)
        begin = rp[row] + k * PA_SEGMENT
        end = torch.minimum(begin + PA_SEGMENT, rp[row + 1])
        self.seg = torch.stack([row, begin, end], 1).to(torch.int32).contiguous()
        self.n_seg = int(row.numel())
        slot = torch.zeros_like(row) if self.cls is None else self.cls[row]
        counts = torch.bincount(slot, minlength=self.K).tolist()
        per_item = max(32, -(-self.n_seg // _PA_ITEMS))
        per_item = (per_item + 7) // 8 * 8
        items, ptr = _pa_items(counts, per_item)
        if len(items) > PA_MAX_ITEMS:
            raise _lib.GdaError(f"PaEdgePlan: {len(items)} work items, the kernel takes {PA_MAX_ITEMS}")
        self.n_items = len(items)
        self.items = torch.tensor(items if items else [(0, 0, 0)], dtype=torch.int32, device=dev)
        self.slot_ptr = torch.tensor(ptr, dtype=torch.int32, device=dev)


def _pa_edge_stats_host(z, edge_index, cls, K):
    """The same sums from the edge list by ``index_add_`` (float64)."""
    n, c = z.shape
    zd = z.detach().double()
    ci = torch.zeros(n, dtype=torch.int64, device=z.device) if cls is None else cls.long()
    i, j = edge_index[0], edge_index[1]
    outer = (zd[i].unsqueeze(2) * zd[j].unsqueeze(1)).reshape(-1, c * c)
    S = torch.zeros(K * K, c * c, dtype=torch.float64, device=z.device)
    S.index_add_(0, ci[i] * K + ci[j], outer)
    return S.view(K, K, c, c).permute(0, 2, 1, 3).contiguous()


def pa_edge_stats(z, plan):
    """``S[a, p, b, q] = sum over the edges (i, j) with cls_i = a, cls_j = b of z_i[p] z_j[q]`` (float64
    ``[K, C, K, C]``) for ``z [N, C]`` fp32 on the graph and classes of ``plan`` (:class:`PaEdgePlan`):
    gda_pa_edge_stats_f64.  No gradient; nothing of edge extent is allocated; two calls return the same bits."""
    z = _f32c(z.detach(), "z")
    if z.dim() != 2 or z.size(0) != plan.n:
        raise ValueError(f"z [N = {plan.n}, C] expected, got {tuple(z.shape)}")
    c, k = z.size(1), plan.K
    _pa_check_classes(c, k, "pa_edge_stats")
    out = torch.empty(k, c, k, c, dtype=torch.float64, device=z.device)
    ws, nbytes = _lib.scratch("gda_pa_edge_stats_workspace_bytes", z.device, "pa_edge", plan.n_items, c, k)
    _lib.call("gda_pa_edge_stats_f64", plan.colidx, z, plan.cls, plan.n, c, k, plan.seg, plan.n_seg, plan.items,
              plan.n_items, plan.slot_ptr, out, ws, nbytes, _lib.stream())
    return out


class PaSoftPlan:
    """The work lists of :func:`pa_softmax_sums` for a pair of domains: each domain's rows sorted by class, cut into
    runs of one class, the target's slots behind the source's."""

    def __init__(self, n0, cls0, K0, n1, cls1, K1, device):
        dev = torch.device(device)
        _pa_check_classes(1, max(K0, K1), "PaSoftPlan")
        self.n, self.K, self.order, items, ptr = (int(n0), int(n1)), (int(K0), int(K1)), [], [], [0]
        for dom, (n, cls, k) in enumerate(((n0, cls0, K0), (n1, cls1, K1))):
            cls = _pa_cls(cls, n, k, dev, "PaSoftPlan")
            self.order.append(None if cls is None else torch.argsort(cls, stable=True).to(torch.int32).contiguous())
            counts = [int(n)] if cls is None else torch.bincount(cls, minlength=k).tolist()
            per_item = max(1024, -(-int(n) // _PA_ITEMS))
            it, p = _pa_items(counts, per_item)
            base = len(ptr) - 1
            items += [(dom, base + s, lo, hi) for s, lo, hi in it]
            ptr += [ptr[base] + v for v in p[1:]]
        if len(items) > PA_MAX_ITEMS:
            raise _lib.GdaError(f"PaSoftPlan: {len(items)} work items, the kernel takes {PA_MAX_ITEMS}")
        self.n_items = len(items)
        self.items = torch.tensor(items if items else [(0, 0, 0, 0)], dtype=torch.int32, device=dev)
        self.slot_ptr = torch.tensor(ptr, dtype=torch.int32, device=dev)


def _pa_softmax_sums_host(z, cls, K):
    p = torch.softmax(z.detach(), dim=1).double()
    out = torch.zeros(K, z.size(1), dtype=torch.float64, device=z.device)
    return out.index_add_(0, torch.zeros(z.size(0), dtype=torch.int64, device=z.device) if cls is None else cls.long(), p)


def pa_softmax_sums(z0, z1, plan):
    """``(P0 [K0, C], P1 [K1, C])`` in float64 with ``P[a, p] = sum of softmax(z_i)[p] over the rows of class a``, both
    domains in one launch (gda_pa_softmax_sums_f64).  No gradient; deterministic."""
    z0, z1 = _f32c(z0.detach(), "z0"), _f32c(z1.detach(), "z1")
    c = z0.size(1)
    if z0.dim() != 2 or z1.dim() != 2 or z1.size(1) != c or (z0.size(0), z1.size(0)) != plan.n:
        raise ValueError(f"z0 [{plan.n[0]}, C] and z1 [{plan.n[1]}, C] expected, got {tuple(z0.shape)}, {tuple(z1.shape)}")
    _pa_check_classes(c, 1, "pa_softmax_sums")
    slots = plan.K[0] + plan.K[1]
    out = torch.empty(slots, c, dtype=torch.float64, device=z0.device)
    ws, nbytes = _lib.scratch("gda_pa_softmax_sums_workspace_bytes", z0.device, "pa_soft", plan.n_items, c)
    _lib.call("gda_pa_softmax_sums_f64", z0, z1, plan.order[0], plan.order[1], plan.n[0], plan.n[1], c, plan.items,
              plan.n_items, plan.slot_ptr, slots, out, ws, nbytes, _lib.stream())
    return out[:plan.K[0]], out[plan.K[0]:]


def _pa_ce_host(logits, labels, coef, sel):
    import torch.nn.functional as F
    if sel is not None:
        logits, labels = logits[sel], labels[sel]
    ce = F.cross_entropy(logits, labels, reduction="none")
    return torch.mean(coef.to(ce.dtype)[labels] * ce)


class _PaCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, coef, sel, stats):
        x = _f32c(logits, "logits")
        n, c = x.shape
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        ws, nbytes = _lib.scratch("gda_pa_ce_workspace_bytes", x.device, "pa_ce")
        ctx.n_sel = 0 if sel is None else int(sel.numel())
        _lib.call("gda_pa_ce_fwd_f32", x, labels, n, c, sel, ctx.n_sel, coef, loss, stats, ws, nbytes, _lib.stream())
        ctx.save_for_backward(x, labels, coef)
        ctx.sel = sel
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        x, labels, coef = ctx.saved_tensors
        n, c = x.shape
        gx = torch.empty_like(x)
        _lib.call("gda_pa_ce_bwd_f32", x, labels, n, c, ctx.sel, ctx.n_sel, coef,
                  gl.reshape(1).to(torch.float32).contiguous(), gx, _lib.stream())
        return gx, None, None, None, None


def pa_ce(logits, labels, coef, sel=None, stats=None):
    """``mean over the selected rows of coef[y_i] * cross_entropy(logits_i, y_i)``: ``sel`` an int64 list of distinct
    rows (a ``train_mask``'s ``nonzero``) or None for all rows, ``coef [C]`` fp32 read on the DEVICE when the kernel
    runs -- a captured call sees values written into it afterwards.  ``stats`` (float64 ``[2]``, optional) receives
    ``[loss, number of rows among ALL whose arg-max is their label]``.  Device: gda_pa_ce_{fwd,bwd}_f32 (the backward
    reads ``coef`` again: change it between steps, not between a forward and its backward); host tensors: torch."""
    if logits.dim() != 2 or labels.dim() != 1 or labels.numel() != logits.size(0) or coef.numel() != logits.size(1):
        raise ValueError(f"logits [N, C], labels [N] and coef [C] expected, got {tuple(logits.shape)}, "
                         f"{tuple(labels.shape)}, {tuple(coef.shape)}")
    if not logits.is_cuda:
        loss = _pa_ce_host(logits, labels, coef, sel)
        if stats is not None:
            stats[0] = float(loss)
            stats[1] = float((logits.detach().argmax(dim=1) == labels).sum())
        return loss
    _pa_check_classes(logits.size(1), 1, "pa_ce")
    _lib.require_gpu_tensor(labels, "labels", torch.int64)
    _lib.require_gpu_tensor(coef, "coef", torch.float32)
    if sel is not None:
        _lib.require_gpu_tensor(sel, "sel", torch.int64)
        if sel.dim() != 1 or sel.numel() < 1 or not sel.is_contiguous():
            raise ValueError("sel: a non-empty contiguous int64 vector of rows expected")
    if stats is not None and (stats.dtype != torch.float64 or stats.numel() != 2 or not stats.is_contiguous()):
        raise ValueError("stats: a contiguous float64 [2] expected")
    if not coef.is_contiguous():
        raise ValueError("coef is read in place by the kernel and must be contiguous")
    return _PaCE.apply(logits, labels.contiguous(), coef, sel, stats)


class PaGraph:
    """A re-weighted aggregation graph whose values are refreshed in place: ``graph`` (what ``propagate`` takes) with
    ``val = base * ((1 - lmda) + lmda * w)`` on both of its CSRs, ``base`` the values at ``w = 1`` -- the gcn
    normalisation and the mean's ``1 / count`` as nn.reweight_gnn._ReweightedGraphCache folds them, built once."""

    def __init__(self, edge_index, n, edge_weight, lmda, gcn_norm, mean):
        from .nn.reweight_gnn import _ReweightedGraphCache
        ones = torch.ones(edge_index.size(1), dtype=torch.float32, device=edge_index.device)
        g = self.graph = _ReweightedGraphCache().get(edge_index, ones, 0.0, n, gcn_norm, mean)     # lmda = 0: val = base
        self.base, self.t_base = g.val.clone(), g.t_val.clone()
        self.n, self.lmda = int(n), float(lmda)
        if edge_weight is not None and not bool((edge_weight == 1).all()):
            # weights the caller starts from: the same ingest on the same edge list lays the entries out the same way
            w = _ReweightedGraphCache().get(edge_index, edge_weight, lmda, n, gcn_norm, mean)
            if not (torch.equal(w.colidx, g.colidx) and torch.equal(w.t_colidx, g.t_colidx)):
                raise _lib.GdaError("PaGraph: two ingests of one edge list disagree on the entry order")
            g.val.copy_(w.val)
            g.t_val.copy_(w.t_val)
        else:
            mix = torch.tensor(float(1.0 - lmda), dtype=torch.float32) + torch.tensor(float(lmda), dtype=torch.float32)
            g.val.mul_(float(mix))
            g.t_val.mul_(float(mix))


def pa_refresh(pg, cls, rw):
    """``pg`` (:class:`PaGraph`) takes the class-pair table ``rw [C, C]`` (fp32, device): the entry of the edge
    ``(i, j)`` of ``edge_index`` becomes ``base * ((1 - lmda) + lmda * rw[cls_i, cls_j])`` in the forward CSR and in the
    transposed one that ``propagate``'s backward reads -- one gda_pa_refresh_values_f32 launch per side, no sort."""
    g, c = pg.graph, rw.size(0)
    _pa_check_classes(c, 1, "pa_refresh")
    _lib.require_gpu_tensor(rw, "rw", torch.float32)
    _lib.require_gpu_tensor(cls, "cls", torch.int64)
    if rw.shape != (c, c) or not rw.is_contiguous() or cls.numel() != pg.n or not cls.is_contiguous():
        raise ValueError(f"rw [C, C] and cls [N = {pg.n}], both contiguous, expected")
    keep = float(1.0 - pg.lmda)
    # rows of the forward CSR are edge_index[0]: (row, col) = (i, j); of the transposed one edge_index[1]: (j, i)
    _lib.call("gda_pa_refresh_values_f32", g.rowptr, g.colidx, pg.base, g.val, pg.n, g.nnz_cap, cls, rw, c, keep,
              pg.lmda, 0, _lib.stream())
    _lib.call("gda_pa_refresh_values_f32", g.t_rowptr, g.t_colidx, pg.t_base, g.t_val, pg.n, g.nnz_cap, cls, rw, c, keep,
              pg.lmda, 1, _lib.stream())


# ------------------------------------------------------------- svd_transform on the device (csrc/gda_svd.hip) --
SVD_SPLIT_THRESHOLD = 32          # rows of the Laplacian beyond twice this many entries are summed in chunks of it
SVD_MAX_WIDTH = 4096              # GDA_SVD_MAX_WIDTH


def svd_panel_ld(w):
    """Leading dimension of a ``[N, w]`` panel: rows start on 128-byte boundaries (110 -> 128, 1010 -> 1024)."""
    return (int(w) + 31) // 32 * 32


def svd_panel(n, w, device):
    """An uninitialised ``[n, w]`` fp32 view of a ``[n, svd_panel_ld(w)]`` block."""
    return torch.empty(n, svd_panel_ld(w), dtype=torch.float32, device=device)[:, :w]


def _panel(t, name):
    _lib.require_gpu_tensor(t, name, torch.float32)
    if t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)):
        raise ValueError(f"{name} must be a row-major [N, w] panel (a column view of a wider block is fine)")
    return t, (t.stride(0) if t.size(0) > 1 else max(t.size(1), 1))


class SvdLaplacian:
    """The combinatorial Laplacian ``D - A`` of pygda/utils/svd_transform.py:59-69 as an operator: self loops dropped,
    ``-1`` once per distinct directed pair, the diagonal the out-degree with duplicates counted.  Holds the
    de-duplicated, loop-free CSR pair (by source for ``L X``, by destination for ``L^T X``), the degree vector and the
    long-row layouts; no value array, no dense matrix."""

    def __init__(self, edge_index, num_nodes, threshold=SVD_SPLIT_THRESHOLD):
        from .graph import RowSplit, check_index_range
        _lib.require_gpu_tensor(edge_index, "edge_index", torch.int64)
        if edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise ValueError(f"edge_index must have shape [2, E], got {tuple(edge_index.shape)}")
        n, dev = int(num_nodes), edge_index.device
        if edge_index.size(1) > 0:
            check_index_range(edge_index, n)
        row, col = edge_index[0], edge_index[1]
        keep = row != col
        row, col = row[keep], col[keep]
        self.num_nodes, self.device, self.threshold = n, dev, int(threshold)
        self.diag = torch.bincount(row, minlength=n).to(torch.float32)
        pairs = torch.unique(row * n + col)                    # the "last writer wins" scatter: every pair once
        self.nnz = int(pairs.numel())
        if self.nnz:
            g = build_csr(torch.stack([pairs // n, pairs % n]), n, add_self_loops="drop", normalize=False, validate=False)
            # by-source rows hold the columns of L's rows; by-destination rows those of L^T
            self._csr = {False: (g.t_rowptr, g.t_colidx), True: (g.rowptr, g.colidx)}
            self._split = {t: RowSplit(rp, n, g.nnz_cap, threshold=self.threshold) for t, (rp, _) in self._csr.items()}
        else:
            rp = torch.zeros(n + 1, dtype=torch.int32, device=dev)
            ci = torch.zeros(1, dtype=torch.int32, device=dev)
            self._csr = {False: (rp, ci), True: (rp, ci)}
            self._split = {False: RowSplit.without_hubs(self.threshold), True: RowSplit.without_hubs(self.threshold)}

    def split_counts(self, transposed=False):
        """``(n_long, n_chunks)`` of the layout the kernels walk."""
        s = self._split[bool(transposed)]
        return s.n_long, s.n_chunks

    def _args(self, x, transposed, moments, tag):
        x, ldx = _panel(x, "x")
        if x.size(0) != self.num_nodes:
            raise ValueError(f"x has {x.size(0)} rows, the graph {self.num_nodes} nodes")
        if x.size(1) < 1 or x.size(1) > SVD_MAX_WIDTH:
            raise _lib.GdaError(f"panel widths 1 .. {SVD_MAX_WIDTH} are supported, got {x.size(1)}")
        s = self._split[bool(transposed)]
        sp = None
        if s.n_long:
            sp = _lib.RowSplitStruct(s.threshold, s.n_long, s.n_chunks, s.long_rows.data_ptr(), s.long_chunk_ptr.data_ptr(),
                                     s.chunk_long.data_ptr(), None, None)
        ws, nbytes = _lib.scratch("gda_svd_lap_workspace_bytes", x.device, tag, self.num_nodes, x.size(1), s.n_long,
                                  s.n_chunks, int(moments))
        return x, ldx, sp, ws, nbytes

    def apply(self, x, transposed=False, out=None):
        """``L x`` (``L^T x`` with ``transposed``) for a ``[N, w]`` panel; ``out`` (another panel) is filled and returned."""
        x, ldx, sp, ws, nbytes = self._args(x, transposed, False, "svd_lap")
        if out is None:
            out = svd_panel(self.num_nodes, x.size(1), x.device)
        y, ldy = _panel(out, "out")
        if y.shape != x.shape:
            raise ValueError("out must have the shape of x")
        rp, ci = self._csr[bool(transposed)]
        with profiler.region("svd_lap_apply", 1, 4 * (self.nnz + 2 * self.num_nodes) * x.size(1), 0):
            _lib.call("gda_svd_lap_apply_f32", rp, ci, self.diag, self.num_nodes, x.size(1), x, ldx, y, ldy,
                      ctypes.byref(sp) if sp is not None else None, ws if nbytes else None, nbytes, _lib.stream())
        return out

    def moments(self, x, transposed=False):
        """``[2, w]`` float64: the column sums and sums of squares of ``L x``, which is not written."""
        x, ldx, sp, ws, nbytes = self._args(x, transposed, True, "svd_lap")
        out = torch.empty(2, x.size(1), dtype=torch.float64, device=x.device)
        rp, ci = self._csr[bool(transposed)]
        with profiler.region("svd_lap_moments", 1, 4 * (self.nnz + self.num_nodes) * x.size(1), 0):
            _lib.call("gda_svd_lap_moments_f32", rp, ci, self.diag, self.num_nodes, x.size(1), x, ldx, out,
                      ctypes.byref(sp) if sp is not None else None, ws if nbytes else None, nbytes, _lib.stream())
        return out


def svd_gram(y, out=None):
    """``y^T y`` ([w, w] fp32, symmetric bit for bit) of a ``[N, w]`` panel on the fp32 matrix cores."""
    y, ldy = _panel(y, "y")
    n, w = y.shape
    if w < 1 or w > SVD_MAX_WIDTH:
        raise _lib.GdaError(f"panel widths 1 .. {SVD_MAX_WIDTH} are supported, got {w}")
    if out is None:
        out = torch.empty(w, w, dtype=torch.float32, device=y.device)
    ws, nbytes = _lib.scratch("gda_svd_gram_workspace_bytes", y.device, "svd_gram", n, w)
    with profiler.region("svd_gram", 1, 4 * (n * w + w * w), n * w * (w + 1)):
        _lib.call("gda_svd_gram_f32", y, ldy, n, w, out, out.stride(0), ws if nbytes else None, nbytes, _lib.stream())
    return out


def svd_panel_matmul(y, r, out):
    """``out [N, m] = y [N, w] @ r [w, m]`` on panels (gda_gemm_f32, NN); ``out`` must be another panel than ``y``."""
    y, ldy = _panel(y, "y")
    o, ldo = _panel(out, "out")
    r = _f32c(r, "r")
    if r.size(0) != y.size(1) or o.shape != (y.size(0), r.size(1)):
        raise ValueError(f"shapes do not chain: {tuple(y.shape)} @ {tuple(r.shape)} -> {tuple(o.shape)}")
    gemm_raw(GEMM_NN, y.size(0), r.size(1), y.size(1), y, ldy, r, r.size(1), o, ldo, name="svd_panel_matmul")
    return out


# ------------------------------------------- GMMClustering / Clustering on the device (csrc/gda_gmm.hip) --
GMM_MAX_DIM = 128                 # GDA_GMM_MAX_DIM
GMM_MAX_COMPONENTS = 32           # GDA_GMM_MAX_COMPONENTS
GMM_MAX_RUNS = 8                  # GDA_GMM_MAX_RUNS
KMEANS_COS, KMEANS_SQEUC, KMEANS_EUC_NORMALISED = 0, 1, 2


def gmm_check_limits(d, k, r=1):
    """GdaError, before any device work, for a mixture wider than the kernels take."""
    if not (1 <= d <= GMM_MAX_DIM and 1 <= k <= GMM_MAX_COMPONENTS and 1 <= r <= GMM_MAX_RUNS):
        raise _lib.GdaError(f"the mixture kernels take 1 .. {GMM_MAX_DIM} columns, 1 .. {GMM_MAX_COMPONENTS} components "
                            f"and 1 .. {GMM_MAX_RUNS} runs, got d={d}, components={k}, runs={r}")


def gmm_state(r, device):
    """``[r, 32]`` bytes of ``gda_gmm_state``: zero counters and flags, lower bound ``-inf``."""
    st = torch.zeros(r, 32, dtype=torch.uint8, device=device)
    st.view(torch.float64)[:, :2] = float("-inf")
    return st


def gmm_state_fields(state):
    """``(bounds [r, 2] float64: lower bound and its predecessor, ints [r, 4] int32: n_iter, converged, failed, 0)``:
    views of the state, nothing is read."""
    return state.view(torch.float64)[:, :2], state.view(torch.int32)[:, 4:8]


def _gmm_x(x):
    x, ldx = _panel(x, "x")
    n, d = x.shape
    if n < 1:
        raise ValueError("x has no rows")
    return x, ldx, n, d


def gmm_mstep(x, resp, reg_covar=1e-6, state=None, out=None):
    """``(weights [R, K], means [R, K, d], covariances [R, K, d, d])`` of sklearn's M-step from ``resp [R, N, K]``."""
    x, ldx, n, d = _gmm_x(x)
    resp = _f32c(resp, "resp")
    if resp.dim() != 3 or resp.size(1) != n:
        raise ValueError(f"resp must be [R, N={n}, K], got {tuple(resp.shape)}")
    r, _, k = resp.shape
    gmm_check_limits(d, k, r)
    f32 = dict(dtype=torch.float32, device=x.device)
    w, mu, cov = out if out is not None else (torch.empty(r, k, **f32), torch.empty(r, k, d, **f32),
                                              torch.empty(r, k, d, d, **f32))
    ws, nbytes = _lib.scratch("gda_gmm_mstep_workspace_bytes", x.device, "gmm_mstep", n, d, k, r)
    with profiler.region("gmm_mstep", 4, 4 * (n * d + r * n * k + r * k * d * d), r * k * n * d * (d + 1)):
        _lib.call("gda_gmm_mstep_f32", x, ldx, n, d, k, r, resp, float(reg_covar), w, mu, cov, state, ws, nbytes,
                  _lib.stream())
    return w, mu, cov


def gmm_factor(cov, state, out=None):
    """``(precisions_cholesky [R, K, d, d], log_det [R, K] float64)``; a covariance without a Cholesky factor sets the run's
    ``failed`` flag in ``state`` (read it when the host may wait)."""
    cov = _f32c(cov, "covariances")
    r, k, d, _ = cov.shape
    gmm_check_limits(d, k, r)
    f32 = dict(dtype=torch.float32, device=cov.device)
    prec, logdet = out if out is not None else (torch.empty(r, k, d, d, **f32),
                                                torch.empty(r, k, dtype=torch.float64, device=cov.device))
    with profiler.region("gmm_factor", 1, 8 * r * k * d * d, r * k * d * d * d):
        _lib.call("gda_gmm_factor_f32", cov, d, k, r, prec, logdet, state, _lib.stream())
    return prec, logdet


def gmm_estep(x, weights, means, prec, logdet, tol=1e-3, state=None, out=None):
    """``resp [R, N, K]`` of one E-step; with ``state`` the call also closes the iteration (lower bound, flags)."""
    x, ldx, n, d = _gmm_x(x)
    r, k = weights.shape
    gmm_check_limits(d, k, r)
    resp = out if out is not None else torch.empty(r, n, k, dtype=torch.float32, device=x.device)
    logdet = _lib.require_gpu_tensor(logdet, "log_det", torch.float64).contiguous()
    ws, nbytes = _lib.scratch("gda_gmm_estep_workspace_bytes", x.device, "gmm_estep", n, r)
    with profiler.region("gmm_estep", 2 if state is not None else 1, 4 * (n * d + r * n * k + r * k * d * d),
                         r * k * n * d * (d + 1)):
        _lib.call("gda_gmm_estep_f32", x, ldx, n, d, k, r, _f32c(weights, "weights"), _f32c(means, "means"),
                  _f32c(prec, "precisions_chol"), logdet, resp, float(tol), state, ws, nbytes, _lib.stream())
    return resp


def kmeans_step(x, centers, metric=KMEANS_COS, want_dist=True):
    """``(labels [N] int64, dist [N, K] or None, sums [K, d], counts [K])``: one assignment step against ``centers``."""
    x, ldx, n, d = _gmm_x(x)
    centers = _f32c(centers, "centers")
    k = centers.size(0)
    if centers.dim() != 2 or centers.size(1) != d:
        raise ValueError(f"centers must be [K, {d}], got {tuple(centers.shape)}")
    gmm_check_limits(d, k)
    f32 = dict(dtype=torch.float32, device=x.device)
    labels = torch.empty(n, dtype=torch.int64, device=x.device)
    dist = torch.empty(n, k, **f32) if want_dist else None
    sums, counts = torch.empty(k, d, **f32), torch.empty(k, **f32)
    ws, nbytes = _lib.scratch("gda_kmeans_step_workspace_bytes", x.device, "kmeans_step", n, d, k)
    with profiler.region("kmeans_step", 2, 4 * (n * d + n * k), 2 * n * d * k):
        _lib.call("gda_kmeans_step_f32", x, ldx, n, d, k, centers, int(metric), labels, dist, sums, counts, ws, nbytes,
                  _lib.stream())
    return labels, dist, sums, counts


def gmm_label_sums(x, labels, k, out=None):
    """``(sums [k, d], counts [k])``: the per-label sums of the rows of ``x`` and the label counts, ``labels [N]`` int64."""
    x, ldx, n, d = _gmm_x(x)
    gmm_check_limits(d, k)
    labels = _lib.require_gpu_tensor(labels, "labels", torch.int64).contiguous()
    if labels.shape != (n,):
        raise ValueError(f"labels must be [{n}], got {tuple(labels.shape)}")
    f32 = dict(dtype=torch.float32, device=x.device)
    sums, counts = out if out is not None else (torch.empty(k, d, **f32), torch.empty(k, **f32))
    ws, nbytes = _lib.scratch("gda_gmm_label_sums_workspace_bytes", x.device, "gmm_label_sums", n, d, k)
    with profiler.region("gmm_label_sums", 2, 4 * (n * d + k * d) + 8 * n, n * d):
        _lib.call("gda_gmm_label_sums_f32", x, ldx, n, d, k, labels, sums, counts, ws, nbytes, _lib.stream())
    return sums, counts


def _lsa_out(k, device, out):
    if out is not None:
        return out
    return (torch.empty(k, dtype=torch.int32, device=device), torch.empty(k, dtype=torch.int32, device=device))


def lsa_cos(tgt_centers, src_centers, state=None, out=None):
    """``(cluster2label [K], shuffle_idx [K])`` int32: the linear assignment of ``0.5 (1 - cos)`` between the rows of the
    two ``[K, d]`` centre matrices (float64 on the device, scipy's algorithm).  ``state``: one run's ``gda_gmm_state``; a
    non-finite cost gives the identity and sets its ``failed``."""
    tgt, src = _f32c(tgt_centers, "tgt_centers"), _f32c(src_centers, "src_centers")
    if tgt.dim() != 2 or tgt.shape != src.shape:
        raise ValueError(f"the centres must be two [K, d] matrices, got {tuple(tgt.shape)} and {tuple(src.shape)}")
    k, d = tgt.shape
    gmm_check_limits(d, k)
    c2l, shuf = _lsa_out(k, tgt.device, out)
    with profiler.region("lsa_cos", 1, 8 * k * d, 2 * k * k * d):
        _lib.call("gda_lsa_cos_f32", tgt, src, k, d, c2l, shuf, state, _lib.stream())
    return c2l, shuf


def lsa_cost(cost, state=None, out=None):
    """:func:`lsa_cos` for a ready ``[K, K]`` float64 cost matrix."""
    cost = _lib.require_gpu_tensor(cost, "cost", torch.float64).contiguous()
    if cost.dim() != 2 or cost.size(0) != cost.size(1):
        raise ValueError(f"cost must be [K, K], got {tuple(cost.shape)}")
    k = cost.size(0)
    gmm_check_limits(1, k)
    c2l, shuf = _lsa_out(k, cost.device, out)
    with profiler.region("lsa_cost", 1, 8 * k * k, k * k * k):
        _lib.call("gda_lsa_cost_f64", cost, k, c2l, shuf, state, _lib.stream())
    return c2l, shuf


def gmm_relabel(resp, cluster2label=None, shuffle_idx=None, fallback=None, state=None, want_prob=True, out=None):
    """``(prob [N, K] or None, labels [N] int64, onehot [N, K])`` of ``resp [N, K]``: the columns re-arranged by
    ``shuffle_idx``, ``cluster2label[argmax]`` (``fallback``'s label where ``state``'s ``failed`` is set) and its one-hot
    row.  Without the two permutations: the argmax of ``resp`` alone (no ``prob``)."""
    resp = _f32c(resp, "resp")
    if resp.dim() != 2:
        raise ValueError(f"resp must be [N, K], got {tuple(resp.shape)}")
    n, k = resp.shape
    gmm_check_limits(1, k)
    if fallback is not None:
        fallback = _lib.require_gpu_tensor(fallback, "fallback", torch.int64).contiguous()
    if cluster2label is None:
        want_prob = False
    if out is not None:
        prob, labels, hot = out
    else:
        prob = torch.empty(n, k, dtype=torch.float32, device=resp.device) if want_prob else None
        labels = torch.empty(n, dtype=torch.int64, device=resp.device)
        hot = torch.empty(n, k, dtype=torch.float32, device=resp.device)
    with profiler.region("gmm_relabel", 1, 12 * n * k + 8 * n, n * k):
        _lib.call("gda_gmm_relabel_f32", resp, n, k, cluster2label, shuffle_idx, fallback, state, prob, labels, hot,
                  _lib.stream())
    return prob, labels, hot
