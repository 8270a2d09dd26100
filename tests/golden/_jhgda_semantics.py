"""JHGDA fixture support: the two shims the reference's ``jhgda_base.py`` needs beyond ``_pyg_stub``, and the driver
that runs the reference's own ``jhgda.py`` / ``jhgda_base.py`` / ``gmm_clustering.py`` (build container only, via
``make_golden_jhgda``).

SHIMS (stated as the issue asks):
- ``torch_sparse.spmm(index, value, m, n, matrix)`` (torch_sparse/spmm.py): ``out[row] += value * matrix[col]`` into an
  ``[m, matrix.size(1)]`` zero matrix, duplicate entries summed (index_add in entry order);
- ``torch_geometric.utils.degree(index, num_nodes, dtype)``: the count of each node in ``index``.  Only the import of
  ``gmm_clustering.py`` needs it: the GMMClustering object jhgda_base builds is never used."""
import numpy as np
import torch

from . import _pyg_stub


def spmm(index, value, m, n, matrix):
    row, col = index[0], index[1]
    out = torch.zeros(m, matrix.size(1), dtype=matrix.dtype)
    return out.index_add_(0, row, value.to(matrix.dtype)[:, None] * matrix[col])


def degree(index, num_nodes=None, dtype=None):
    n = _pyg_stub.maybe_num_nodes(index, num_nodes)
    return torch.zeros(n, dtype=dtype or torch.float32).index_add_(0, index, torch.ones(index.numel(),
                                                                                         dtype=dtype or torch.float32))


def load_jhgda(ref):
    import sys
    from . import _ref_loader
    sys.modules["torch_sparse"].spmm = spmm
    sys.modules["torch_geometric.utils"].degree = degree
    _ref_loader._load("pygda.nn.gmm_clustering", "pygda/nn/gmm_clustering.py")
    jb = _ref_loader._load("pygda.nn.jhgda_base", "pygda/nn/jhgda_base.py")
    sys.modules["pygda.nn"].JHGDABase = jb.JHGDABase
    jm = _ref_loader._load("pygda.models.jhgda", "pygda/models/jhgda.py")
    ref.JHGDABase, ref.JHGDA, ref.GCNPooling = jb.JHGDABase, jm.JHGDA, jb.GCNPooling
    return ref


def run_fit(ref, s, t, kw, epochs, init_seed, dtype=torch.float32):
    """The reference's ``JHGDA.fit`` and both ``predict``s.  ``dtype`` float64 runs the same lines under
    ``torch.set_default_dtype(torch.float64)`` with float64 features, from the same float32 initial state."""
    import pygda.models.jhgda as jmod
    m = ref.JHGDA(device="cpu", epoch=epochs, verbose=0, **kw)
    rec, log = {}, []
    init = m.init_model

    def init_rec(**k):
        old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float32)
        try:
            net = init(**k)
        finally:
            torch.set_default_dtype(old)
        rec["init"] = {k2: v.detach().numpy().copy() for k2, v in net.state_dict().items()}
        return net.to(dtype)

    m.init_model = init_rec
    lms = []
    fwd = m.forward_model

    def forward_rec(sd, td):                    # the epoch's label_matching sum: an argmax count inside the loss
        out = fwd(sd, td)
        lms.append(float(sum(float(x['lm']) for x in m.jhgda.pooling_loss)))
        return out

    m.forward_model = forward_rec
    old_log = jmod.logger
    jmod.logger = lambda **k: log.append((k["loss"], k["source_train_acc"]))
    old_dtype = torch.get_default_dtype()
    if dtype == torch.float64:
        s = _pyg_stub.Data(x=s.x.double(), edge_index=s.edge_index, y=s.y)
        t = _pyg_stub.Data(x=t.x.double(), edge_index=t.edge_index, y=t.y)
    try:
        torch.set_default_dtype(dtype)
        torch.manual_seed(init_seed)
        m.fit(s, t)
        src_logits, _ = m.predict(s)
        tgt_logits, _ = m.predict(t)
    finally:
        jmod.logger = old_log
        torch.set_default_dtype(old_dtype)
    final = {k: v.detach().double().numpy().copy() for k, v in m.jhgda.state_dict().items()}
    return dict(init=rec["init"], final=final, losses=np.array([l for l, _ in log], dtype=np.float64),
                lm=np.array(lms, dtype=np.float64),
                accs=np.array([a for _, a in log], dtype=np.float64), src_logits=src_logits.detach().double().numpy(),
                tgt_logits=tgt_logits.detach().double().numpy())
