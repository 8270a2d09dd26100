"""``A2GNNBase`` (pygda/nn/a2gnn_base.py:11-203): L asymmetric-propagation conv layers
(act + dropout after each), a conv classifier with one propagation step, optional linear
domain discriminator behind gradient reversal."""
import torch.nn.functional as F
from torch import nn

from .prop_gcn_conv import PropGCNConv
from .reverse_layer import GradReverse
from .linear import DenseLinear


def global_mean_pool(x, batch, size=None):
    """PyG's ``global_mean_pool`` as a2gnn_base.py:141 calls it on a collated batch: per-graph mean of the node
    rows (``gda_segment_mean_fwd/bwd_f32``); ``size`` defaults to the loader's ``num_graphs`` when the batch
    vector carries it."""
    from ..ops import segment_mean
    if size is None:
        size = getattr(batch, "_gda_num_graphs", None)
    return segment_mean(x, batch, size)


class ActPair:
    """Layer 0's output ALREADY through ``dropout(relu(.))``, in two independent draws: ``draws[0]`` for the pass that is
    differentiated (the features the domain loss reads), ``draws[1]`` (may be None) for the trainer's second pass over the
    same layer-0 output.  What :meth:`A2GNNBase.first_conv` hands out when the aggregation's epilogue applied the
    activation (ops.propagate_act); :meth:`A2GNNBase.feat_bottleneck_from` continues from either form."""
    __slots__ = ("draws",)

    def __init__(self, a, b=None):
        self.draws = (a, b)

    def detach(self):
        return ActPair(self.draws[0].detach(), None if self.draws[1] is None else self.draws[1].detach())


class StackedAct:
    """Layer 0's output of the trainer's TWO source passes, already through ``dropout(relu(.))`` with independent draws and
    stacked ``[2n, h]`` (the projection's epilogue wrote it: ops.tall_linear_act mode 2)."""
    __slots__ = ("y",)

    def __init__(self, y):
        self.y = y


class A2GNNBase(nn.Module):
    def __init__(self, in_dim, hid_dim, num_classes, num_layers=1, adv=False, dropout=0.1,
                 act=F.relu, mode="node", **kwargs):
        super().__init__()
        self.in_dim, self.hid_dim, self.num_classes = in_dim, hid_dim, num_classes
        self.num_layers, self.adv, self.dropout, self.act, self.mode = num_layers, adv, dropout, act, mode
        widths = [in_dim] + [hid_dim] * num_layers
        self.convs = nn.ModuleList(PropGCNConv(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.cls = PropGCNConv(hid_dim, num_classes) if mode == "node" else DenseLinear(hid_dim, num_classes)
        if adv:
            self.domain_discriminator = DenseLinear(hid_dim, 2)

    def second_leaves(self, table):
        """Context manager: inside it the conv layers read their weight / bias through SECOND leaf tensors over the same
        storage, so the gradients of a second pass over the shared layers (the trainer's target branch) land in those
        leaves' ``.grad`` instead of being added onto the first pass's by autograd -- one elementwise launch per shared
        tensor (four at A2GNN's depth, the last two between the final gradient kernel and the optimiser update).
        ``table`` (``pygda_amd.optim.Adam.grad_aliases``: id(parameter) -> leaf) is kept current; the update kernel
        forms ``grad + leaf.grad``, the value the accumulation would have stored.  Not in the reference."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            swapped = []
            for conv in self.convs:
                for owner, name in ((conv.lin, "weight"), (conv, "bias")):
                    p = owner._parameters.get(name)
                    if p is None or not p.requires_grad:
                        continue
                    a = table.get(id(p))
                    if a is None or a.data_ptr() != p.data_ptr() or a.stride() != p.stride() or a.shape != p.shape:
                        a = table[id(p)] = nn.Parameter(p.detach())      # same storage (re-made if the weight was re-laid out)
                    owner._parameters[name] = a
                    swapped.append((owner, name, p))
            try:
                yield
            finally:
                for owner, name, p in swapped:
                    owner._parameters[name] = p
        return scope()

    def forward(self, data, prop_nums):
        batch = None if self.mode == "node" else data.batch
        h = self.feat_bottleneck(data.x, data.edge_index, batch, prop_nums=prop_nums)
        return self.feat_classifier(h, data.edge_index, batch, prop_nums=1)

    def feat_bottleneck(self, x, edge_index, batch, prop_nums=30):
        return self.feat_bottleneck_from(self.first_conv(x, edge_index, prop_nums), edge_index, batch, prop_nums)

    def first_conv(self, x, edge_index, prop_nums, draws=0):
        """Output of layer 0 BEFORE activation / dropout: a deterministic function of the inputs,
        so the two passes the trainer makes over the same graph (features and logits) can share
        it -- the reference recomputes it, projection and all ``prop_nums`` aggregations, per pass.
        ``draws`` (1 or 2; the trainers' sampled steps): the caller will continue with that many
        :meth:`feat_bottleneck_from` passes and accepts an :class:`ActPair` -- the activation applied by the
        aggregation's epilogue -- when this batch allows it."""
        conv = self.convs[0]
        if draws == "stacked":
            # the two source passes as one pass over stacked rows (feat_pair_from) on a sampled batch: projection, bias,
            # both dropout draws of the activation -- and the batch's feature gather -- in one launch
            hit = conv.forward_stacked(x, self.dropout, self.training, 2) \
                if (prop_nums <= 0 and self.act is F.relu and self.mode == "node" and self.hid_dim % 4 == 0) else None
            if hit is not None:
                return StackedAct(hit)
            draws = 0
        if draws and self.act is F.relu and self.mode == "node" and prop_nums > 0:
            hit = conv.forward_act(x, edge_index, prop_nums, self.dropout, self.training, pair=draws > 1)
            if hit is not None:
                return ActPair(*hit) if draws > 1 else ActPair(hit)
        return conv.forward_colmajor(x, edge_index, prop_nums) if self._fused_act(x) else conv(x, edge_index, prop_nums)

    def _fused_act(self, x):
        """ReLU on the device: the conv may hand its result over in the K-step kernel's column-major
        layout, which the fused activation kernel consumes directly (no transpose pass in between)."""
        return self.act is F.relu and x.is_cuda and self.mode == "node"

    def _act_dropout(self, x):
        from ..ops import ColMajor
        if isinstance(x, ColMajor) or (self.act is F.relu and x.is_cuda):   # fused kernel; other activations compose
            from ..ops import relu_dropout
            return relu_dropout(x, self.dropout, self.training)
        return F.dropout(self.act(x), p=self.dropout, training=self.training)

    def feat_bottleneck_from(self, h0, edge_index, batch, prop_nums=30, draw=0, preact_out=False):
        """``feat_bottleneck`` continued from a precomputed :meth:`first_conv` output (``draw``: which of an
        :class:`ActPair`'s two dropout draws this pass continues from).  A conv's column-major pre-activation goes
        straight to the next conv where that conv's projection can apply the activation itself
        (PropGCNConv.forward_from_preact); ``preact_out``: the LAST one is handed back as it is (a ``ColMajor``) for
        :meth:`feat_classifier` to do the same -- only for a pass that nothing else reads."""
        from ..ops import ColMajor
        pre = x = None                      # `pre`: a conv's output whose activation is still to be applied
        if isinstance(h0, ActPair):
            x = h0.draws[draw] if h0.draws[draw] is not None else h0.draws[0]
        else:
            pre = h0
        for conv in self.convs[1:]:
            if pre is not None:
                nxt = conv.forward_from_preact(pre, edge_index, prop_nums, self.dropout, self.training) \
                    if (isinstance(pre, ColMajor) and self.act is F.relu and self.mode == "node") else None
                if nxt is not None:
                    pre = nxt
                    continue
                x, pre = self._act_dropout(pre), None
            hit = conv.forward_act(x, edge_index, prop_nums, self.dropout, self.training) \
                if (self.act is F.relu and self.mode == "node" and prop_nums > 0) else None
            if hit is not None:
                x = hit
                continue
            pre = conv.forward_colmajor(x, edge_index, prop_nums) if self._fused_act(x) else conv(x, edge_index, prop_nums)
        if pre is not None:
            if preact_out and isinstance(pre, ColMajor) and self.mode == "node":
                return pre
            x = self._act_dropout(pre)
        if self.mode == "graph":
            x = global_mean_pool(x, batch)
        return x

    def feat_pair_from(self, h0, edge_index, batch, prop_nums=30):
        """TWO ``feat_bottleneck_from`` passes over the same ``h0`` (independent dropout draws) -- the trainer's
        feature pass and logits pass over one domain.  With ``prop_nums = 0`` every layer acts row by row, so
        the two passes run as ONE pass over the stacked rows ``[2n, h]``: half the launches each way, one weight
        gradient GEMM per layer instead of two plus an accumulation, the gradient of ``h0`` summed inside the
        activation's backward kernel.  Otherwise: two passes, the first result first."""
        from ..ops import relu_dropout_pair, relu_dropout_pair_ok, split_halves
        stacked = isinstance(h0, StackedAct)
        if not stacked and not (prop_nums <= 0 and self.mode == "node" and self.act is F.relu and relu_dropout_pair_ok(h0)
                                and self.hid_dim % 4 == 0):
            return (self.feat_bottleneck_from(h0, edge_index, batch, prop_nums),
                    self.feat_bottleneck_from(h0, edge_index, batch, prop_nums))
        x = h0.y if stacked else relu_dropout_pair(h0, self.dropout, self.training)
        rest = list(self.convs[1:])
        for conv in rest[:-1]:
            hit = conv.forward_stacked(x, self.dropout, self.training, 1) if stacked else None
            x = hit if hit is not None else self._act_dropout(conv(x, edge_index, prop_nums))
        if rest:            # the last activation hands out the two halves itself: its backward stacks and masks in one pass
            from ..ops import relu_dropout_split
            hit = rest[-1].forward_stacked(x, self.dropout, self.training, 3) if stacked else None
            if hit is not None:
                return hit
            return relu_dropout_split(rest[-1](x, edge_index, prop_nums), self.dropout, self.training)
        return split_halves(x)

    def feat_classifier(self, x, edge_index, batch, prop_nums=1):
        from ..ops import ColMajor
        if isinstance(x, ColMajor):         # feat_bottleneck_from(preact_out=True): the activation is still to be applied
            hit = self.cls.forward_logits_from_preact(x, edge_index, prop_nums, self.dropout, self.training) \
                if self.mode == "node" else None
            if hit is not None:
                return hit
            x = self._act_dropout(x)
        return self.cls(x, edge_index, prop_nums) if self.mode == "node" else self.cls(x)

    def domain_classifier(self, x, alpha):
        return self.domain_discriminator(GradReverse.apply(x, alpha))
