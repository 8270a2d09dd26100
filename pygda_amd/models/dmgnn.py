"""``DMGNN`` trainer (pygda/models/dmgnn.py): domain-adaptive message passing on ACDNE's network.

DMGNN is ACDNE's sibling in the reference, line for line: ``ACDNEBase`` as the network, the same ``process_graph``
(K-step transition matrix, its PPMI, the PPMI-weighted neighbour features), the same batch generator with its wrap
quirk, both cross-entropies and the log line.  All of that is :class:`~pygda_amd.models.acdne.ACDNE`'s code, inherited
here -- the argument checks, :func:`~pygda_amd.models.acdne.epoch_indices`, the captured steps, the device-side
``alpha`` and the float64 loss accumulator.  What differs runs on csrc/gda_dmgnn.hip:

- the proximity loss is ``nei_prox_loss``: ``|E - A E|_F / h`` per domain, with ``A`` the row-normalised block of the
  PPMI at the batch's indices (:func:`~pygda_amd.ops.dmgnn_prox`);
- the classifier logits of each half get ``A @ logits`` added before the cross-entropy, so the classifier gradient
  returns through ``I + A_s^T`` (:func:`~pygda_amd.ops.dmgnn_heads`; the target half's propagated logits enter no loss
  and are not formed on the GPU);
- ``predict`` returns ``P + PPMI @ P`` with ``P`` the softmax probabilities of the fit-time stacked rows and ``PPMI``
  the domain's unnormalised dense PPMI (:func:`~pygda_amd.ops.dmgnn_predict`): not probabilities, and only their
  ``argmax`` is used by the log line.

Kept from the reference on purpose, beyond what ACDNE's docstring lists: after a wrap the block ``A`` is read at the
new permutation's positions, i.e. it is the proximity of other nodes than the batch's own rows, and that ``A`` also
propagates the logits; dropout stays on in ``predict``; ``num_neigh`` is ignored.  The network is ``self.dmgnn``."""
import torch.nn.functional as F

from ..ops import dmgnn_heads, dmgnn_predict, dmgnn_prox
from .acdne import ACDNE


class DMGNN(ACDNE):
    _net_name = "dmgnn"

    def __init__(self, in_dim, hid_dim, num_classes, num_layers=0, n_emb=128, pair_weight=0.1, step=3, dropout=0.,
                 act=F.relu, weight_decay=0., lr=4e-3, epoch=200, device='cuda:0', batch_size=100, num_neigh=-1,
                 verbose=2, **kwargs):
        super().__init__(in_dim=in_dim, hid_dim=hid_dim, num_classes=num_classes, num_layers=num_layers, n_emb=n_emb,
                         pair_weight=pair_weight, step=step, dropout=dropout, act=act, weight_decay=weight_decay,
                         lr=lr, epoch=epoch, device=device, batch_size=batch_size, num_neigh=num_neigh,
                         verbose=verbose, **kwargs)

    def _step_loss(self, zd, rows, pidx, alpha, loss_acc, out):
        prox, gprox, a_blocks = dmgnn_prox(self.ppmi_s, self.ppmi_t, pidx, zd, self._half, self.pair_weight)
        if zd.is_cuda:
            return dmgnn_heads(zd, gprox, a_blocks, self._heads, self.y_s, rows, alpha, prox, self.pair_weight,
                               loss_acc=loss_acc, out=out)
        return dmgnn_heads(zd, gprox, a_blocks, self._heads, self.y_s, rows, alpha, prox, self.pair_weight)

    def predict(self, data, train=False):
        """``P + PPMI @ P`` over the fit-time stacked rows: the first ``len(data.x)`` with the source PPMI when
        ``train=True``, the last ``len(data.x)`` with the target PPMI otherwise (dropout stays on, as in the
        reference); ``data.y`` as the labels."""
        return super().predict(data, train)

    def _probabilities(self, z, weight, bias, train):
        return dmgnn_predict(z, weight, bias, self.ppmi_s if train else self.ppmi_t)
