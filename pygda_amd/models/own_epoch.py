"""``OwnEpochGDA``: what ASN, JHGDA, SEPA and SOGA share around the epoch each of them writes itself and drives through
``epoch_graph.run_epochs`` -- the data-parallel refusal and the edge-bounds check, one ``_dom`` per domain, the ``fit``
split into the project's Adam + ``_device_fit`` or torch's Adam + a host loop, the slot buffers of a replay and the
tail of a device epoch.  A trainer supplies ``_check`` (its own refusals around the two shared ones), ``_init_fit``
(build the model, reset the logs, return the trained parameters), ``_host_epoch`` and ``_device_fit``.
``SourceFreeGDA`` adds what SOGA, GTrans and GraphCTA share on top: the log that carries an accuracy only while the
source is trained on, the source-label range check and the reference's two empty hooks."""
import os
import time
from types import SimpleNamespace

import torch

from .base import BaseGDA


def refuse_data_parallel(trainer):
    from ..distributed import active
    if active():
        raise NotImplementedError(f"{type(trainer).__name__}: data-parallel training is not supported")


class OwnEpochGDA(BaseGDA):
    _unroll_env = None            # the environment variable behind ``epochs_per_graph``'s default, or None: a plain 4
    _host_dtype = None            # the features' dtype on the host, or None: as given

    def __init__(self, **kwargs):
        default = os.environ.get(self._unroll_env, "4") if self._unroll_env else 4
        self.epochs_per_graph = int(kwargs.pop("epochs_per_graph", default))
        super().__init__(**kwargs)

    def _check_edges(self, *datas, empty_ok=True):
        for d in datas:
            n, ei = d.x.shape[0], d.edge_index
            if (not empty_ok and ei.numel() == 0) or (ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= n)):
                raise ValueError(f"{type(self).__name__}: edge_index refers to nodes outside [0, {n})")

    def _check_labels(self, y):
        if y.numel() and (int(y.min()) < 0 or int(y.max()) >= self.num_classes):
            raise ValueError(f"{type(self).__name__}: a source label is outside [0, {self.num_classes})")

    def _dom(self, data, dev):
        """One domain on ``dev``: ``x`` (fp32 on the GPU), ``edge_index``, ``y`` and the node count ``n``."""
        x = data.x.to(dev, torch.float32 if dev.type == "cuda" else self._host_dtype or data.x.dtype).contiguous()
        return SimpleNamespace(x=x, edge_index=data.edge_index.to(dev), y=data.y.to(dev), n=x.size(0))

    def _device_args(self, s, t):
        """Further arguments of ``_device_fit(s, t, ...)``, built after the optimiser."""
        return ()

    def fit(self, source_data, target_data):
        self._check(source_data, target_data)
        dev = torch.device(self.device)
        s, t = self._dom(source_data, dev), self._dom(target_data, dev)
        params = list(self._init_fit(s, t))
        if dev.type == "cuda":
            from ..optim import Adam
            self.optimizer = Adam(params, lr=self.lr, weight_decay=self.weight_decay)
            self._device_fit(s, t, *self._device_args(s, t))
            return
        self._host_fit(s, t, torch.optim.Adam(params, lr=self.lr, weight_decay=self.weight_decay))

    def _host_fit(self, s, t, optimizer):
        self._host_epochs(optimizer, lambda epoch: self._host_epoch(s, t, epoch), time.time())

    def _host_epochs(self, optimizer, epoch_fn, start):
        """``self.epoch`` host epochs: ``epoch_fn(epoch)`` returns the loss and a callable that gives the log's
        accuracy once the step is taken."""
        for epoch in range(self.epoch):
            loss, accuracy = epoch_fn(epoch)
            epoch_loss = loss.item()
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            self._report(epoch, epoch_loss, accuracy(), start)

    def _slots(self, dtype=torch.float32, **tails):
        """The epochs per replay ``U``; per keyword a zeroed ``[U, *tail]`` device buffer ``self._<name>_buf``."""
        U = max(int(self.epochs_per_graph), 1)
        for name, tail in tails.items():
            setattr(self, f"_{name}_buf", torch.zeros(U, *tail, dtype=dtype, device=torch.device(self.device)))
        return U

    def _step(self, u, loss, **slots):
        """The tail of a device epoch: the loss, then ``slots``' values (a callable is computed now, behind the loss's
        copy), into slot ``u``; backward; the step."""
        self._loss_buf[u].copy_(loss.detach())
        for name, value in slots.items():
            getattr(self, f"_{name}_buf")[u].copy_(value() if callable(value) else value)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()


class SourceFreeGDA(OwnEpochGDA):
    """Pretraining on the source, then adaptation on the target alone: ``_phase`` is "source" until the trainer sets
    it to "target", and only a source epoch's log line carries an accuracy unless the trainer sets
    ``_target_accuracy``."""
    _unroll_env = "PYGDA_AMD_GRAPH_UNROLL"
    _phase = "source"
    _target_accuracy = False      # True: the adaptation epochs' log lines carry an accuracy as well (GraphATA)

    def forward_model(self, data, **kwargs):
        pass

    def process_graph(self, data):
        pass

    def _report(self, epoch, loss, acc, start):
        super()._report(epoch, loss, acc if self._phase == "source" or self._target_accuracy else None, start)
