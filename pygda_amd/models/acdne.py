"""``ACDNE`` trainer (pygda/models/acdne.py): Adversarial Deep Network Embedding for cross-network node classification.

``fit`` runs process_graph on both domains -- the K-step transition matrix, its PPMI and the PPMI-weighted neighbour
features -- on csrc/gda_acdne.hip, then ``epoch`` epochs of ``round(max(Ns, Nt) / (batch_size / 2))`` steps of
``h = int(batch_size / 2)`` source rows and h target rows each: the two encoders on the hand-written GEMMs, then the
proximity loss and the heads (classifier CE over the source half, GradReverse(alpha) -> 128 -> 128 -> 2 with the domain
CE) as two fused kernels that produce the step's loss and every gradient of the embedding and the heads.  The log line
is the float64 sum of the step losses and the source accuracy of ``predict(source, train=True)``.

What this port keeps from the reference, on purpose:
- the batch indices are drawn with ``np.random.permutation`` in the reference's exact order (its generators are lazy:
  source, then target, then one draw per wrap, :meth:`batch_index_stream`);
- after a wrap within an epoch the reference re-permutes the already shuffled rows but yields the NEW permutation as
  ``shuffle_index``: the step's rows are the composed permutation while ``batch_ppmi`` reads the PPMI entries at the
  new permutation's positions, i.e. of other nodes than the batch's own.  This is reproduced (the two index sets are
  shipped separately); fixing it is out of scope;
- dropout is always on (``F.dropout(x, p)`` in FE1 / FE2), in ``predict`` too;
- ``predict`` returns softmax probabilities of the fit-time stacked rows -- the first Ns with ``train=True``, the last
  Nt otherwise -- and ignores ``data`` except for its row count and labels;
- the classification loss covers the source half only; ``num_layers`` and edge weights are unused.
process_graph follows the float32 semantics the reference was written for (numpy 1.x; under numpy 2's NEP 50
``a_k / k`` would turn everything after it float64 and the reference's first ``predict`` then fails).  The adjacency is
sized by the node count, so an isolated last node has zero PPMI rows and columns where the reference crashes.

On the GPU the steps replay as hipGraphs, ``steps_per_graph`` (default 8) per replay: the epoch's index draws are
shipped once per epoch, each replay copies its slice into the captured step's buffer, alpha lives on the device and
the loss accumulates there.  Raised before any device work: data-parallel runs (NotImplementedError), ``batch_size <
2``, a domain with fewer than ``batch_size / 2`` nodes, more than 128 rows per domain on the GPU, and source labels
that do not span ``num_classes`` (ValueError)."""
import time

import numpy as np
import torch
import torch.nn.functional as F

from ..metrics import eval_micro_f1
from ..nn.acdne_base import ACDNEBase
from ..ops import ACDNE_MAX_HALF, acdne_heads, acdne_predict, acdne_process_graph, acdne_prox
from .base import BaseGDA


def batch_index_stream(n, half):
    """The reference's ``batch_generator(..., half, shuffle=True)`` reduced to indices: yields ``(rows, ppmi_index)``
    per batch -- the original row numbers the batch holds (the composed permutation) and the ``shuffle_index`` slice it
    yields (the latest permutation) -- drawing ``np.random.permutation(n)`` exactly when the reference does."""
    perm = np.random.permutation(n)
    order = perm
    count = 0
    while True:
        if count * half + half >= n:
            count = 0
            perm = np.random.permutation(n)
            order = order[perm]
        start = count * half
        count += 1
        yield order[start:start + half], perm[start:start + half]


def epoch_indices(ns, nt, half, num_batch):
    """One epoch's draws in the reference's order: int64 ``[num_batch, 2, 2 half]``, ``[:, 0]`` the rows of the stacked
    arrays (target rows offset by ``ns``), ``[:, 1]`` the PPMI indices within each domain."""
    gs, gt = batch_index_stream(ns, half), batch_index_stream(nt, half)
    out = np.empty((num_batch, 2, 2 * half), dtype=np.int64)
    for k in range(num_batch):
        rs, ps = next(gs)
        rt, pt = next(gt)
        out[k, 0, :half], out[k, 1, :half] = rs, ps
        out[k, 0, half:], out[k, 1, half:] = rt + ns, pt
    return out


class ACDNE(BaseGDA):
    _net_name = "acdne"          # the attribute that holds the network: the reference's name (DMGNN: ``dmgnn``)

    @property
    def _net(self):
        return getattr(self, self._net_name)

    def __init__(self, in_dim, hid_dim, num_classes, num_layers=0, n_emb=128, pair_weight=0.1, step=3, dropout=0.,
                 act=F.relu, weight_decay=0., lr=4e-3, epoch=100, device='cuda:0', batch_size=100, num_neigh=-1,
                 verbose=2, **kwargs):
        steps_per_graph = int(kwargs.pop("steps_per_graph", 8))
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers,
                         dropout=dropout, act=act, weight_decay=weight_decay, lr=lr, epoch=epoch, device=device,
                         batch_size=batch_size, num_neigh=num_neigh, verbose=verbose, **kwargs)
        self.n_emb, self.pair_weight, self.step = n_emb, pair_weight, step
        self.steps_per_graph = steps_per_graph

    def init_model(self, **kwargs):
        return ACDNEBase(n_input=self.in_dim, n_hidden=[self.hid_dim] * 2, n_emb=self.n_emb,
                         num_class=self.num_classes, drop=self.dropout, batch_size=self.batch_size,
                         **kwargs).to(self.device)

    def forward_model(self, **kwargs):
        pass

    def _check(self, source_data, target_data):
        from .own_epoch import refuse_data_parallel
        name = type(self).__name__
        refuse_data_parallel(self)
        b = self.batch_size
        if not isinstance(b, int) or b < 2:
            raise ValueError(f"{name}: batch_size must be an int >= 2 (got {b!r}): the reference divides by "
                             "batch_size // 2")
        half = int(b / 2)
        ns, nt = source_data.x.shape[0], target_data.x.shape[0]
        if ns < half or nt < half:
            raise ValueError(f"{name}: both domains need at least batch_size / 2 = {half} nodes (got {ns} and {nt})")
        if torch.device(self.device).type == "cuda" and half > ACDNE_MAX_HALF:
            raise ValueError(f"{name}: at most {ACDNE_MAX_HALF} rows per domain in a step on the GPU "
                             f"(batch_size <= {2 * ACDNE_MAX_HALF + 1}), got {half}")
        top = int(source_data.y.max()) + 1
        if top != self.num_classes:
            raise ValueError(f"{name}: the source labels span {top} classes but num_classes is {self.num_classes}: "
                             "the reference's one-hot rows would not match the logits")
        if self.step < 1:
            raise ValueError(f"{name}: step must be >= 1")

    def process_graph(self, data, out=None):
        """``(A_ppmi [N, N], X_nei [N, F])`` on ``self.device``."""
        x = data.x.to(self.device, torch.float32)
        ppmi, x_nei = acdne_process_graph(data.edge_index.to(self.device), x, x.size(0), self.step, out=out)
        if out is not None and x_nei is not out:
            out.copy_(x_nei)
        return ppmi, x_nei

    def fit(self, source_data, target_data):
        self._check(source_data, target_data)
        dev = torch.device(self.device)
        cuda = dev.type == "cuda"
        ns, nt = source_data.x.shape[0], target_data.x.shape[0]
        self.num_source_nodes, self.num_target_nodes = ns, nt
        xs = source_data.x.to(dev, torch.float32)
        xt = target_data.x.to(dev, torch.float32)
        self.whole_xs_xt_stt = torch.cat([xs, xt]).contiguous()
        self.whole_xs_xt_stt_nei = torch.empty_like(self.whole_xs_xt_stt)
        self.ppmi_s, _ = self.process_graph(source_data, out=self.whole_xs_xt_stt_nei[:ns])
        self.ppmi_t, _ = self.process_graph(target_data, out=self.whole_xs_xt_stt_nei[ns:])
        self.y_s = source_data.y.to(dev, torch.int64).contiguous()
        self._src_y = source_data.y

        setattr(self, self._net_name, self.init_model(**self.kwargs))
        if cuda:
            from ..optim import Adam
            self.optimizer = Adam(list(self._net.parameters()), lr=self.lr, weight_decay=self.weight_decay)
        else:
            self.optimizer = torch.optim.Adam(self._net.parameters(), lr=self.lr, weight_decay=self.weight_decay)
        self._heads = self._net.head_parameters()
        self._half = half = int(self.batch_size / 2)
        num_batch = round(max(ns / (self.batch_size / 2), nt / (self.batch_size / 2)))
        self._graph = None
        if cuda:
            self._alpha = torch.zeros((), dtype=torch.float32, device=dev)
            self._loss_acc = torch.zeros(1, dtype=torch.float64, device=dev)
            self._head_out = (torch.empty(2 * half, self.n_emb, dtype=torch.float32, device=dev),
                              [torch.empty_like(p) for p in self._heads])
            self._pinned = torch.empty(num_batch, 2, 2 * half, dtype=torch.int64).pin_memory()
            self._dev_idx = torch.empty(num_batch, 2, 2 * half, dtype=torch.int64, device=dev)
        start = time.time()
        for epoch in range(self.epoch):
            p = float(epoch) / self.epoch
            alpha = 2. / (1. + np.exp(-10. * p)) - 1
            idx = epoch_indices(ns, nt, half, num_batch)
            if cuda:
                epoch_loss = self._device_epoch(idx, float(alpha))
            else:
                epoch_loss = 0
                for k in range(num_batch):
                    t = torch.from_numpy(idx[k])
                    epoch_loss += self._step(t[0], t[1], alpha).item()
            probs, labels = self.predict(source_data, train=True)
            acc = eval_micro_f1(labels.to(probs.device), probs.argmax(dim=1))
            self._report(epoch, epoch_loss, acc, start)
        self._graph = None

    # -- one step ----------------------------------------------------------------------------------------------------
    def _step(self, rows, pidx, alpha, loss_acc=None, out=None):
        """Forward, loss, backward and the Adam update of one batch (eager, or recorded into a hipGraph)."""
        X, Xn = self.whole_xs_xt_stt, self.whole_xs_xt_stt_nei
        if X.is_cuda:
            from ..ops import dropout_state, gather_rows
            dropout_state.next_step(X.device)
            xb, xn = gather_rows(X, rows), gather_rows(Xn, rows)
        else:
            xb, xn = X.index_select(0, rows), Xn.index_select(0, rows)
        self._net.train()
        z = self._net.network_embedding.pre_embedding(xb, xn)
        loss, dz, grads = self._step_loss(z.detach(), rows, pidx, alpha, loss_acc, out)
        self.optimizer.zero_grad(set_to_none=True)
        z.backward(dz)
        for prm, g in zip(self._heads, grads):
            prm.grad = g
        self.optimizer.step()
        return loss

    def _step_loss(self, zd, rows, pidx, alpha, loss_acc, out):
        """``(loss, dz, head gradients)`` of one batch from the embedding before its ReLU: two fused calls."""
        prox, gprox = acdne_prox(self.ppmi_s, self.ppmi_t, pidx, zd, self._half, self.pair_weight)
        if zd.is_cuda:
            return acdne_heads(zd, gprox, self._heads, self.y_s, rows, alpha, prox, self.pair_weight,
                               loss_acc=loss_acc, out=out)
        return acdne_heads(zd, gprox, self._heads, self.y_s, rows, alpha, prox, self.pair_weight)

    def _device_epoch(self, idx, alpha):
        num_batch = idx.shape[0]
        self._pinned.numpy()[...] = idx
        self._dev_idx.copy_(self._pinned, non_blocking=True)
        self._alpha.fill_(alpha)
        self._loss_acc.zero_()
        U = self.steps_per_graph
        use_graph = self._want_hip_graph() and U >= 1 and num_batch >= U
        if use_graph and self._graph is None:
            self._capture(U)
        k = 0
        while k < num_batch:
            if use_graph and num_batch - k >= U:
                self._cur.copy_(self._dev_idx[k:k + U])
                self._graph.replay()
                k += U
            else:
                self._step(self._dev_idx[k, 0], self._dev_idx[k, 1], self._alpha, self._loss_acc, self._head_out)
                k += 1
        return float(self._loss_acc.item())

    def _capture(self, U):
        """U steps recorded into one hipGraph reading ``self._cur [U, 2, 2h]``.  The warm-up step is rolled back
        (parameters, Adam state, the epoch's loss sum), so the fit takes exactly the eager steps."""
        from ..epoch_graph import capture_rolled_back
        self._cur = self._dev_idx[:U].clone()
        self._graph = capture_rolled_back(
            lambda u: self._step(self._cur[u, 0], self._cur[u, 1], self._alpha, self._loss_acc, self._head_out),
            U, self._net.parameters(), [self.optimizer], also=[self._loss_acc])

    def predict(self, data, train=False):
        """Softmax probabilities of the fit-time stacked rows: the first ``len(data.x)`` with ``train=True``, the last
        ``len(data.x)`` otherwise (dropout stays on, as in the reference); ``data.y`` as the labels."""
        n, N = data.x.shape[0], self.whole_xs_xt_stt.size(0)
        lo, hi = (0, n) if train else (N - n, N)
        self._net.eval()
        with torch.no_grad():
            z = self._net.network_embedding.pre_embedding(self.whole_xs_xt_stt[lo:hi], self.whole_xs_xt_stt_nei[lo:hi])
            lay = self._net.node_classifier.layer
            probs = self._probabilities(z, lay.weight, lay.bias, train)
        return probs, data.y

    def _probabilities(self, z, weight, bias, train):
        return acdne_predict(z, weight, bias)
