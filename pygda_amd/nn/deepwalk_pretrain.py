"""``DWPretrain`` (pygda/nn/deepwalk_pretrain.py): DeepWalk embeddings for DGDA -- PyG's ``Node2Vec`` with ``p = q = 1``,
sparse gradients and ``SparseAdam(lr=0.01)``, 128 start nodes per batch, the reference's signature and defaults.

The walks come from a HIP kernel (ops.dgda_walks, csrc/gda_dgda.hip: one lane per walk, uniform neighbours from the
project's Philox, a node without out-edges stays put) on the device and from the same rule in torch on the host.  The
skip-gram step is composed of torch operators: windows of ``context_size`` over each walk of ``walk_length`` nodes
(``walk_length - context_size + 1`` windows per walk; the first node of a window is the centre), negatives that are
uniformly random nodes behind the same start nodes, ``-log(sigmoid + 1e-15)`` for the positive pairs and
``-log(1 - sigmoid + 1e-15)`` for the negative ones, a row-sparse Adam.

NO PARITY TEST AGAINST PyG: the project's fixtures run the reference on a stub of torch_geometric that has neither
``Node2Vec`` nor torch_cluster's walks, so the windowing above is PyG's ``Node2Vec`` restated and not checked against
it, and the walks and negatives come from another generator.
The update scatters sparse gradients whose accumulation order the device does not fix, so the pretraining is NOT
bit-reproducible; DGDA's parity tests inject embeddings (``pretrained_emb``) instead."""
import torch

EPS = 1e-15


def walk_csr(edge_index, n):
    """``(rowptr, col)`` int64: the out-edges of every node in edge order, duplicates kept."""
    row, col = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    order = torch.argsort(row, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=row.device)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    return rowptr, col[order].contiguous()


def _host_walks(rowptr, col, start, length):
    if col.numel() == 0:
        return start.view(-1, 1).repeat(1, length + 1)
    cur, out = start, [start]
    for _ in range(length):
        b, d = rowptr[cur], rowptr[cur + 1] - rowptr[cur]
        r = torch.minimum((torch.rand(cur.numel()) * d).to(torch.int64), (d - 1).clamp(min=0))
        cur = torch.where(d > 0, col[(b + r).clamp(max=col.numel() - 1)], cur)
        out.append(cur)
    return torch.stack(out, 1)


class DWPretrain(torch.nn.Module):
    def __init__(self, data, epoch=200, embedding_dim=128, walk_length=20, context_size=10, walks_per_node=10,
                 num_negative_samples=1, verbose=True):
        super().__init__()
        if walk_length < context_size:
            raise ValueError("DWPretrain: walk_length must be at least context_size")
        self.data = data
        self.device = data.edge_index.device
        self.epoch, self.embedding_dim = epoch, embedding_dim
        self.walk_length, self.context_size = walk_length, context_size
        self.walks_per_node, self.num_negative_samples = walks_per_node, num_negative_samples
        self.verbose = verbose
        self.num_nodes = int(data.x.shape[0])
        if data.edge_index.numel() and (int(data.edge_index.min()) < 0 or int(data.edge_index.max()) >= self.num_nodes):
            raise ValueError(f"DWPretrain: edge_index refers to nodes outside [0, {self.num_nodes})")
        self.rowptr, self.col = walk_csr(data.edge_index, self.num_nodes)
        self.embedding = torch.nn.Embedding(self.num_nodes, embedding_dim, sparse=True).to(self.device)
        self.batch_size = 128
        self.optimizer = torch.optim.SparseAdam(list(self.embedding.parameters()), lr=0.01)

    def walks(self, start):
        """``[len(start), walk_length]``: every walk's start node and its ``walk_length - 1`` steps."""
        if start.is_cuda:
            from ..ops import dgda_walks
            return dgda_walks(self.rowptr, self.col, start, self.walk_length - 1)
        return _host_walks(self.rowptr, self.col, start, self.walk_length - 1)

    def _windows(self, rw):
        k = rw.size(1) - self.context_size + 1
        return torch.cat([rw[:, j:j + self.context_size] for j in range(k)], 0)

    def sample(self, batch):
        pos = self._windows(self.walks(batch.repeat(self.walks_per_node)))
        start = batch.repeat(self.walks_per_node * self.num_negative_samples)
        rnd = torch.randint(self.num_nodes, (start.numel(), self.walk_length - 1), device=start.device)
        return pos, self._windows(torch.cat([start.view(-1, 1), rnd], -1))

    def _pair_scores(self, rw):
        h0 = self.embedding(rw[:, 0]).unsqueeze(1)
        h = self.embedding(rw[:, 1:].reshape(-1)).view(rw.size(0), -1, self.embedding_dim)
        return (h0 * h).sum(-1).view(-1)

    def loss(self, pos_rw, neg_rw):
        pos = -torch.log(torch.sigmoid(self._pair_scores(pos_rw)) + EPS).mean()
        neg = -torch.log(1 - torch.sigmoid(self._pair_scores(neg_rw)) + EPS).mean()
        return pos + neg

    def train(self):
        """One epoch over the shuffled nodes; the mean batch loss."""
        if self.device.type == "cuda":
            from ..ops import dropout_state
            dropout_state.next_step(self.device)
        perm = torch.randperm(self.num_nodes, device=self.device)
        total, batches = torch.zeros((), device=self.device), 0
        for batch in perm.split(self.batch_size):
            self.optimizer.zero_grad()
            loss = self.loss(*self.sample(batch))
            loss.backward()
            self.optimizer.step()
            total += loss.detach()
            batches += 1
        return float(total) / max(batches, 1)

    def fit(self):
        for epoch in range(self.epoch):
            loss = self.train()
            if self.verbose:
                print(f'Epoch: {epoch:03d}, pretrain loss: {loss:.4f}')

    def get_embedding(self):
        return self.embedding.weight
