"""Minimal graph container and loaders with the PyG names pygda's trainers use
(``Data``; ``NeighborLoader(data, num_neighbors, batch_size=...)``;
pygda/models/a2gnn.py:254-286).  Full-batch loading hands out the graph itself (cached on
the device after the first ``.to``); fan-out sampling is done by the native host sampler
(pygda_amd/sampler.py)."""
import collections.abc
import weakref

import torch
import torch.utils.data


class Data:
    """Any object with ``x [N,F] fp32``, ``edge_index [2,E] int64`` (row 0 = source, row 1 =
    destination), ``y [N] int64`` and ``.to(device)`` satisfies the trainers; this is one."""

    def __init__(self, x=None, edge_index=None, y=None, **kwargs):
        self.x, self.edge_index, self.y = x, edge_index, y
        for k, v in kwargs.items():
            setattr(self, k, v)
        self._device_copies = {}

    # -- container protocol -------------------------------------------------------
    def keys(self):
        return [k for k, v in self.__dict__.items() if not k.startswith("_") and v is not None]

    def __contains__(self, key):
        return key in self.keys()

    def __getitem__(self, key):
        return getattr(self, key)

    @property
    def num_nodes(self):
        if self.x is not None:
            return self.x.size(0)
        return int(self.edge_index.max()) + 1 if self.edge_index is not None and self.edge_index.numel() else 0

    @property
    def num_edges(self):
        return 0 if self.edge_index is None else self.edge_index.size(1)

    @property
    def num_node_features(self):
        return 0 if self.x is None else self.x.size(1)

    def is_undirected(self):
        ei = self.edge_index
        n = self.num_nodes
        a = torch.unique(ei[0] * n + ei[1])
        b = torch.unique(ei[1] * n + ei[0])
        return a.numel() == b.numel() and bool((a == b).all())

    def to(self, device, non_blocking=False):
        """Device copy, made once per device and then reused -- so per-step
        ``batch.to(device)`` (a2gnn.py:311-312) costs nothing after the first call and the
        graph cache sees the same edge tensor every step."""
        device = torch.device(device)
        probe = self.x if self.x is not None else self.edge_index
        if probe is not None and probe.device == device:
            return self
        key = str(device)
        hit = self._device_copies.get(key)
        if hit is None:
            hit = Data(**{k: (v.to(device, non_blocking=non_blocking) if torch.is_tensor(v) else v)
                          for k, v in self.__dict__.items() if not k.startswith("_")})
            self._device_copies[key] = hit
            if device.type == "cuda" and hit.x is not None:
                from . import sparse_features          # bag-of-words inputs: CSR once, SpMM projection
                sparse_features.maybe_register(hit.x)
        if getattr(self, "_static_graph", False) and hit.edge_index is not None:
            hit.edge_index._gda_static = True
        return hit

    def cpu(self):
        return self.to("cpu")

    def __repr__(self):
        info = ", ".join(f"{k}={list(v.shape) if torch.is_tensor(v) else v}" for k, v in self.__dict__.items()
                         if not k.startswith("_") and v is not None)
        return f"Data({info})"


def degree_order(edge_index, num_nodes):
    """``new_id [N]``: the relabelling that numbers the nodes by decreasing in-degree (ties in id order).  On a power-law
    graph the rows most rows gather then share cache lines and pages: the full-graph aggregation of an R-MAT 2^22 graph
    runs 6.8 -> 5.2 ms with it (profiles/HISTORY.md 5, `roofline_hbm_regime.rmat_2^22`); a uniform graph has nothing to gain."""
    deg = torch.bincount(edge_index[1], minlength=num_nodes)
    order = torch.argsort(deg, descending=True, stable=True)          # order[k] = old id of the k-th node
    new_id = torch.empty_like(order)
    new_id[order] = torch.arange(num_nodes, device=order.device)
    return new_id


def relabel(data, new_id):
    """The same graph with node ``i`` renamed ``new_id[i]`` (features, labels, every per-node attribute and the edge
    list follow): an isomorphic ``Data``, so training on it is training on the original; ``out[new_id]`` maps a
    per-node result of the relabelled graph back to the original numbering."""
    n = data.num_nodes
    e = data.num_edges
    inv = torch.empty_like(new_id)
    inv[new_id] = torch.arange(n, device=new_id.device)
    out, private = {}, {}
    for k, v in data.__dict__.items():
        if v is None:
            continue
        if k.startswith("_"):
            # private flags travel (`_static_graph`: the K-step kernel's eligibility); the device-copy cache does not --
            # it holds copies of the OLD numbering
            if k != "_device_copies":
                private[k] = v
        elif k == "edge_index":
            out[k] = new_id[v]
        elif torch.is_tensor(v) and v.dim() >= 1 and v.size(0) == n and not _edge_level(k, v, n, e):
            out[k] = v[inv]
        else:
            out[k] = v                                  # per-edge attributes keep their order: the edges did not move
    res = Data(**out)
    for k, v in private.items():
        setattr(res, k, v)
    return res


def _edge_level(key, v, n, e):
    """Is ``v`` (first dimension n) a per-EDGE attribute?  Only ambiguous when the graph has as many edges as nodes:
    then the PyG naming convention decides (``edge_attr``, ``edge_weight``, ``edge_*`` are per edge; ``x``, ``y``,
    ``batch``, ``pos``, ``*_mask`` per node), and anything else is refused rather than guessed."""
    if e != n:
        return False
    if key.startswith("edge"):
        return True
    if key in ("x", "y", "batch", "pos") or key.endswith("_mask") or key.startswith("node"):
        return False
    raise ValueError(f"relabel: attribute {key!r} has {n} rows and the graph has {n} nodes AND {e} edges -- "
                     "name it edge_* or node_* so that it is permuted (or not) on purpose")


AUTO_REORDER = True             # tests/test_gpu_configs.py turns it off for its reference
AUTO_REORDER_MIN_NODES = 1 << 20
AUTO_REORDER_SKEW = 64.0
SAMPLER_PRIORITY = 0            # of the device sampler's stream


def auto_reorder(data):
    """``(data', new_id)``: the degree-ordered relabelling of a STATIC full-batch graph when it pays -- at least
    ``AUTO_REORDER_MIN_NODES`` nodes (2^20: below that the feature matrix sits in the Infinity Cache anyway) and a
    largest in-degree of at least ``AUTO_REORDER_SKEW`` x the mean (a uniform graph has nothing to reorder: 9.03 ms
    either way at 5 M nodes) -- else ``(data, None)``.  One bincount + one sort + one row permutation per fit()."""
    ei = data.edge_index
    n = data.num_nodes
    if (not AUTO_REORDER or ei is None or data.x is None or n < AUTO_REORDER_MIN_NODES or ei.numel() == 0
            or getattr(data, "batch", None) is not None):
        return data, None
    deg = torch.bincount(ei[1], minlength=n)
    if float(deg.max()) < AUTO_REORDER_SKEW * max(float(ei.size(1)) / n, 1.0):
        return data, None
    order = torch.argsort(deg, descending=True, stable=True)
    new_id = torch.empty_like(order)
    new_id[order] = torch.arange(n, device=order.device)
    return relabel(data, new_id), new_id


def to_undirected(edge_index, num_nodes=None):
    """Symmetrise and de-duplicate an edge list (what benchmark/node/a2gnn.py:92-97 applies)."""
    n = int(edge_index.max()) + 1 if num_nodes is None else num_nodes
    both = torch.cat([edge_index, edge_index.flip(0)], dim=1)
    key = torch.unique(both[0] * n + both[1])
    return torch.stack([key // n, key % n])


class NeighborLoader:
    """``NeighborLoader(data, num_neighbors, batch_size)`` as the trainers build it.

    ``num_neighbors`` all -1 with ``batch_size >= N``: one batch, the whole graph (every
    benchmark setting of the reference).  Otherwise seeds are taken ``batch_size`` at a time
    (in order unless ``shuffle``) and each batch is the union of their sampled L-hop
    in-neighbourhoods, seeds first, exactly ``batch.batch_size`` of them."""

    def __init__(self, data, num_neighbors, batch_size=1, shuffle=False, input_nodes=None,
                 rank=0, world_size=1, seed=0, device=None, prefetch=2, full_batch=None, auto_reorder=False, recycle=False,
                 **kwargs):
        self.prefetch = int(prefetch)
        # sampled batches in a ring of prefetch + 4 blocks written round and round (sampler._Ring: one foreign call per batch
        # in the producer thread).  Only for consumers that are done with a batch when they take the next one
        self.recycle = bool(recycle)
        self._ring = None
        self.num_neighbors = list(num_neighbors)
        self.batch_size, self.shuffle = int(batch_size), shuffle
        self.rank, self.world_size, self.seed = rank, world_size, seed
        n = data.num_nodes
        # ``full_batch=False`` sends a whole-graph request (fan-out -1, one batch) through the sampler
        # anyway: the sampled-batch code path on an input whose result is known (tests)
        full = (all(k == -1 for k in self.num_neighbors) and self.batch_size >= n
                and input_nodes is None and world_size == 1 and full_batch is not False)
        # sampled mode keeps the feature matrix resident on the training device: batches are
        # assembled there by the row-gather kernel, only node / edge ids cross PCIe
        self.data = data.to(device) if (device is not None and not full) else data
        # full batch on a large power-law graph: train on the degree-ordered relabelling (hubs first: the rows most
        # rows gather share cache lines and pages -- 7.85 -> 5.16 ms per aggregation on R-MAT 2^22, profiles/HISTORY.md 5); node i
        # of the caller's numbering is row new_id[i] of every batch, predict() maps results back
        # (``auto_reorder=True``: the trainers whose step reads nothing but the loader's batches ask for it -- a caller
        # that indexes a batch with structures of its own built from the original numbering must not)
        self.new_id = None
        if full and auto_reorder:
            self.data, self.new_id = globals()["auto_reorder"](data)
        self.input_nodes = torch.arange(n) if input_nodes is None else torch.as_tensor(input_nodes).long().cpu()
        self.full_batch = full
        self._sampler = None
        self._epoch = 0

    def _batches(self, epoch=None):
        seeds = self.input_nodes
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + (self._epoch if epoch is None else epoch))
            seeds = seeds[torch.randperm(seeds.numel(), generator=g)]
        chunks = list(torch.split(seeds, self.batch_size))
        # data-parallel shard of the seed batches; every rank gets the same count (short ranks
        # wrap around) so that the per-step gradient all-reduce never waits for a missing peer
        per_rank = -(-len(chunks) // self.world_size)
        return [chunks[(self.rank + i * self.world_size) % len(chunks)] for i in range(per_rank)]

    def __len__(self):
        return 1 if self.full_batch else len(self._batches())

    def sampler_description(self):
        """Which sampler assembles the batches (bench.py: config.sampler)."""
        if self.full_batch:
            return "none (full batch)"
        if self._sampler is None:
            return "not started"
        return self._sampler.description()

    def __iter__(self):
        if self.full_batch:
            self.data._static_graph = True        # the same graph every step: operators derived from it
            if self.data.edge_index is not None:  # (A*A for K-step propagation) may be cached
                self.data.edge_index._gda_static = True
            yield self.data
            return
        from .sampler import NeighborSampler, DeviceNeighborSampler
        if self._sampler is None:
            self._sampler = self._make_sampler()
        # the epoch counter advances when iteration STARTS: ``zip(source_loader, target_loader)`` never
        # resumes the second generator after the first one is exhausted, so a bump after the last yield
        # would leave the target loader on epoch 0 (same neighbourhoods and shuffle every epoch)
        epoch = self._epoch
        self._epoch += 1
        batches = self._batches(epoch)
        seeds_of = lambda b: hash((self.seed, epoch, b, self.rank)) & 0x7FFFFFFF
        if isinstance(self._sampler, DeviceNeighborSampler):
            yield from self._device_batches(batches, seeds_of)
        elif self.prefetch <= 0:
            for b, seeds in enumerate(batches):
                yield self._sampler.sample_batch(self.data, seeds, self.num_neighbors, seed=seeds_of(b))
        else:
            # host sampling of the next batches runs in a background thread (the native sampler
            # releases the GIL) while the device works on the current one; device-side assembly
            # (row gather on the training stream) stays in the consumer thread
            import queue
            import threading
            q, stop = queue.Queue(maxsize=self.prefetch), threading.Event()

            def producer():
                try:
                    for b, seeds in enumerate(batches):
                        if stop.is_set():
                            return
                        q.put((seeds, self._sampler.sample(seeds, self.num_neighbors, seed=seeds_of(b),
                                                           csr=self._sampler.emit_csr(self.data))))
                    q.put(None)
                except BaseException as exc:        # surface sampler errors in the consumer
                    q.put(exc)

            th = threading.Thread(target=producer, daemon=True)
            th.start()
            try:
                while True:
                    item = q.get()
                    if item is None:
                        break
                    if isinstance(item, BaseException):
                        raise item
                    seeds, parts = item
                    yield self._sampler.assemble(self.data, seeds, *parts)
            finally:
                stop.set()
                while th.is_alive():                 # unblock a producer waiting on a full queue
                    try:
                        q.get_nowait()
                    except queue.Empty:
                        th.join(timeout=0.01)


    def iter_raw(self):
        """The batches of :meth:`__iter__` WITHOUT their consumer-side assembly: ``(slot, (n, e, nnz, n_interior))`` per
        batch, ``slot`` = the ring block the device sampler filled (sampler._Slot: node ids, edge list, CSR pair, interior
        K-step plans, all capacity-sized; its ``done`` event orders a consumer behind the sampler's stream).  For the
        captured sampled step (pygda_amd/sampled_graph.py), which copies the block into its static buffers and gathers
        the feature rows inside the graph.  Device sampler + recycling ring only (None otherwise)."""
        from .sampler import DeviceNeighborSampler
        if self.full_batch or not self.recycle or self.prefetch <= 0:
            return None
        if self._sampler is None:
            self._sampler = self._make_sampler()
        if not isinstance(self._sampler, DeviceNeighborSampler):
            return None
        epoch = self._epoch
        self._epoch += 1
        batches = self._batches(epoch)
        seeds_of = lambda b: hash((self.seed, epoch, b, self.rank)) & 0x7FFFFFFF
        return self._device_batches(batches, seeds_of, raw=True)

    def _make_sampler(self):
        """The device sampler when the graph and the features live on the GPU and the fan-outs allow it (1..64, or
        -1 within its workspace budget); the native host sampler otherwise (``PYGDA_AMD_DEVICE_SAMPLER=0`` forces it)."""
        import os
        from .sampler import NeighborSampler, DeviceNeighborSampler
        ei = self.data.edge_index
        if (ei.is_cuda and self.data.x is not None and self.data.x.is_cuda
                and os.environ.get("PYGDA_AMD_DEVICE_SAMPLER", "1") == "1"):
            ds = DeviceNeighborSampler(ei, self.data.num_nodes)
            if ds.supports(self.batch_size, self.num_neighbors):
                return ds
        return NeighborSampler(ei, self.data.num_nodes)

    def _device_batches(self, batches, seeds_of, raw=False):
        """Batches from the device sampler.  With prefetching, a producer thread enqueues batch b+1.. on a side
        stream and waits for their sizes there, so the training stream never waits for a size read-back; the
        consumer orders itself behind the side stream with an event and gathers the feature rows."""
        S = self._sampler
        if self.prefetch <= 0:
            for b, seeds in enumerate(batches):
                yield S.assemble(self.data, S.enqueue(seeds, self.num_neighbors, seed=seeds_of(b)))
            return
        import queue
        import threading
        import time
        self.producer_cpu_s, self.producer_batches, self.producer_enqueue_cpu_s = 0.0, 0, 0.0
        dev = self.data.x.device
        if getattr(self, "_samp_stream", None) is None:
            # the sampler's ~45 small dependent launches per batch sit beside chip-filling training kernels: at the
            # default priority each of them queues behind whatever the training streams have in flight
            self._samp_stream = torch.cuda.Stream(device=dev, priority=SAMPLER_PRIORITY)
        side = self._samp_stream
        side.wait_stream(torch.cuda.current_stream())       # the graph / features may have just been produced
        ring = None
        if self.recycle and not getattr(self, "_ring_busy", False):     # (a second live iterator over this loader allocates)
            if self._ring is None:
                self._ring = S.new_ring(self.prefetch + 4, getattr(self, "static_interior", 0))
            ring = self._ring
            ring.reset()          # (the wait above also puts the last pass's batches behind the sampler's stream)
            self._ring_busy = True
        q, stop = queue.Queue(maxsize=self.prefetch), threading.Event()

        def producer():
            try:
                torch.cuda.set_device(dev)
                with torch.cuda.stream(side):
                    for b, seeds in enumerate(batches):
                        if stop.is_set():
                            return
                        c0 = time.thread_time()
                        p = S.enqueue(seeds, self.num_neighbors, seed=seeds_of(b), ring=ring)
                        self.producer_enqueue_cpu_s += time.thread_time() - c0
                        sizes = p.wait()
                        # on-core time of this thread per batch: what the training thread may have to wait for when it
                        # wants the interpreter lock back (bench.py: config.producer_cpu_ms_per_batch)
                        self.producer_cpu_s += time.thread_time() - c0
                        self.producer_batches += 1
                        q.put((p, sizes))
                q.put(None)
            except BaseException as exc:
                q.put(exc)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                yield item if raw else S.assemble(self.data, *item)
        finally:
            stop.set()
            while th.is_alive():
                try:
                    q.get_nowait()
                except queue.Empty:
                    th.join(timeout=0.01)
            if ring is not None:
                self._ring_busy = False


def collate_graphs(graphs):
    """PyG's ``Batch.from_data_list`` for what pygda's graph mode reads: ``x`` / ``y`` concatenated in list order,
    ``edge_index`` with every graph's node ids shifted by the nodes before it, ``batch`` = graph index per node
    (sorted by construction), ``num_graphs``."""
    counts = torch.tensor([g.x.size(0) for g in graphs], dtype=torch.long)
    offs = (torch.cumsum(counts, 0) - counts).tolist()
    ei = [g.edge_index + o for g, o in zip(graphs, offs)]
    b = Data(x=torch.cat([g.x for g in graphs], dim=0),
             edge_index=torch.cat(ei, dim=1) if ei else torch.empty(2, 0, dtype=torch.long),
             y=torch.cat([g.y.reshape(-1) for g in graphs], dim=0),
             batch=torch.repeat_interleave(torch.arange(len(graphs)), counts), num_graphs=len(graphs))
    return b


class _GraphBatch(Data):
    """A collated batch: ``.to(device)`` tags the device copy of ``batch`` as sorted and with its graph count, so
    the readout needs no device check and no read-back."""

    def to(self, device, non_blocking=False):
        hit = super().to(device, non_blocking)
        if hit.batch is not None:
            hit.batch._gda_sorted = True
            hit.batch._gda_num_graphs = self.num_graphs
        return hit


def _collate(graphs):
    b = collate_graphs(graphs)
    out = _GraphBatch(**{k: getattr(b, k) for k in ("x", "edge_index", "y", "batch", "num_graphs")})
    out.batch._gda_sorted = True
    out.batch._gda_num_graphs = out.num_graphs
    return out


def _variant_key(improved, add_self_loops, normalize, degree_side):
    return (bool(improved), add_self_loops if add_self_loops == "drop" else bool(add_self_loops), bool(normalize),
            degree_side)


class _StoreVariant:
    """One normalisation variant of a store: the CSR pair of the dataset-order block-diagonal graph (device) and the
    stored entries per graph (host)."""

    def __init__(self, store, key):
        from .graph import SPLIT_THRESHOLD, build_csr
        improved, add_self_loops, normalize, degree_side = key
        # (the edges were range-checked at construction: no second look, no host sync for it)
        self.csr = build_csr(store._global_edges(), store.num_nodes, None, improved, add_self_loops, normalize,
                             degree_side, validate=False)
        rowptr, t_rowptr = (r.cpu().to(torch.long) for r in (self.csr.rowptr, self.csr.t_rowptr))   # this variant's one read-back
        self.nnz = rowptr[store._node_ptr_host[1:]] - rowptr[store._node_ptr_host[:-1]]
        # a batch's rows are rows of this graph: where it has no row beyond the long-row layout's limit, no batch has one
        self.hubs = tuple(bool(r.numel() > 1 and int((r[1:] - r[:-1]).max()) > 2 * SPLIT_THRESHOLD) for r in (rowptr, t_rowptr))


class _StorePPMI:
    """The random-walk PPMI pairs of a store for one ``PPMIConv`` layer: the walks drawn ONCE over the dataset-order
    block-diagonal graph (csrc/gda_ppmi_dev.hip, ``gda_ppmi_build_ratio``) and cut per graph.  A walk never leaves its
    graph, so a pair's ``p / colsum`` does not depend on which batch the graph is drawn into; what does -- the batch's
    number of visited nodes -- is a sum of the per-graph counts kept here on the host.  Per pair, graph after graph,
    sorted by (src, dst): graph-local ids (int32) and the ratio (double).  One read-back, here."""

    def __init__(self, store, path_len, passes):
        from . import _lib
        from .graph import SPLIT_THRESHOLD
        from .nn.ppmi_conv import draw_seed
        self.path_len, self.passes = int(path_len), int(passes)
        self.seed = draw_seed()                       # as ppmi_edges(seed=None) draws it: np.random.seed governs the walks
        E, N, G, dev = store.num_edges, store.num_nodes, len(store), store.device
        need = _lib.lib().gda_ppmi_workspace_bytes(E, N, self.path_len, self.passes)
        if need == 0:
            raise ValueError(f"GraphStore(ppmi='per_graph'): {N} nodes x {self.passes} walks x path_len {self.path_len} "
                             f"visits or 2 x {E} edges are beyond the device PPMI builder's 32-bit limits (2^31 - 1); "
                             "use ppmi='per_batch'")
        i64 = dict(dtype=torch.long, device=dev)
        zeros = torch.zeros(G, dtype=torch.long)
        self.pair_counts, self.target_counts, self.loop_counts = zeros, zeros.clone(), zeros.clone()
        self.pair_ptr = torch.zeros(G + 1, **i64)
        self.local_src = self.local_dst = torch.empty(0, dtype=torch.int32, device=dev)
        self.ratio = torch.empty(0, dtype=torch.float64, device=dev)
        self.num_pairs, self.hubs = 0, (False, False)
        if E == 0 or N == 0:
            self._structure(store, torch.empty(0, **i64), torch.empty(0, **i64))
            return
        cap = N * self.passes * self.path_len
        src, dst, count = torch.empty(cap, **i64), torch.empty(cap, **i64), torch.zeros(1, **i64)
        ratio = torch.empty(cap, dtype=torch.float64, device=dev)
        ei = store._global_edges()
        with torch.cuda.device(dev):
            ws = torch.empty(need, dtype=torch.uint8, device=dev)      # one-off, as in ppmi_edges_device: not cached
            _lib.call("gda_ppmi_build_ratio", ei[0].contiguous(), ei[1].contiguous(), E, N, self.path_len, self.passes,
                      self.seed & (2 ** 64 - 1), src, dst, ratio, count, ws, ws.numel(), _lib.stream())
        del ws
        # per-graph counts without a second look at the device: everything below is sized by `cap`, the slots beyond
        # the pair count parked on node N (the pairs are sorted by source, so the parked ones stay last)
        valid = torch.arange(cap, device=dev) < count
        a, b = torch.where(valid, src, N), torch.where(valid, dst, N)
        nodes = torch.arange(N + 1, device=dev)
        out_ptr = torch.searchsorted(a, nodes)                                       # pairs by source node
        in_ptr = torch.searchsorted(torch.sort(b).values, nodes)                     # ... by visited node
        pair_ptr = out_ptr[store.node_ptr]
        cum = lambda flags: torch.cat([torch.zeros(1, **i64), torch.cumsum(flags.to(torch.long), 0)])
        loops, targets = cum(valid & (a == b)), cum(in_ptr[1:] > in_ptr[:-1])
        stats = torch.cat([count, pair_ptr[1:] - pair_ptr[:-1], loops[pair_ptr[1:]] - loops[pair_ptr[:-1]],
                           targets[store.node_ptr[1:]] - targets[store.node_ptr[:-1]],
                           (in_ptr[1:] - in_ptr[:-1]).max().reshape(1), (out_ptr[1:] - out_ptr[:-1]).max().reshape(1)]).cpu()
        m = self.num_pairs = int(stats[0])
        self.pair_counts, self.loop_counts, self.target_counts = stats[1:1 + G], stats[1 + G:1 + 2 * G], stats[1 + 2 * G:1 + 3 * G]
        # rows of the batch graphs are rows of this one; the forward CSR's rows are the visited nodes.  A row holds its
        # pairs and the node's self loop: none beyond the long-row layout's limit here, none in any batch
        self.hubs = tuple(int(v) + 1 > 2 * SPLIT_THRESHOLD for v in stats[1 + 3 * G:])
        first = store.node_ptr[torch.bucketize(src[:m], store.node_ptr[1:], right=True)]     # of the pair's graph
        self.pair_ptr = pair_ptr
        self.local_src, self.local_dst = (src[:m] - first).to(torch.int32), (dst[:m] - first).to(torch.int32)
        self.ratio = ratio[:m].clone()
        self._structure(store, src[:m], dst[:m])

    def _structure(self, store, src, dst):
        """The structure of the normalised graph the ingestion makes of any batch's pair list, in dataset order -- it
        keeps every pair whatever its weight, sorts stably and closes each row with the node's loop, so nothing of it
        depends on a batch: both CSRs (``rowptr`` / ``colidx``, ``t_rowptr`` / ``t_colidx``), per stored entry the pair
        whose ratio weighs it (``pair_of`` / ``t_pair_of``; -1: a loop no pair ``(a, a)`` stands behind, filled with
        the constant) and the entries per graph (host).  ``src`` / ``dst``: the pairs, store-global ids, sorted by
        (src, dst).  One ingestion, once; ``gda_collate_ppmi_csr_f32`` gathers a batch's graph out of it."""
        from .graph import build_csr
        N, dev, m = store.num_nodes, store.device, src.numel()
        self.entry_counts = self.pair_counts - self.loop_counts + store.node_counts
        nnz = self.num_entries = int(self.entry_counts.sum())
        with torch.cuda.device(dev):
            g = build_csr(torch.stack([src, dst]), N, None, False, True, False, "row", validate=False)
        self.rowptr, self.t_rowptr = g.rowptr, g.t_rowptr
        self.colidx, self.t_colidx = g.colidx[:max(nnz, 1)].clone(), g.t_colidx[:max(nnz, 1)].clone()
        k = torch.arange(m, device=dev)
        loop = src == dst
        # by source the non-loop pairs keep their order: before pair k stand the non-loop pairs before it and the loops
        # of the rows before its own; by destination they stand in the stable order of their destinations
        by_src = k - (torch.cumsum(loop.long(), 0) - loop.long()) + src
        rank = torch.empty_like(k)
        rank[torch.sort(torch.where(loop, N, dst), stable=True).indices] = k
        by_dst = rank + dst
        maps = []
        for pos, rp in ((by_dst, g.rowptr), (by_src, g.t_rowptr)):
            last = rp.long()[src + 1] - 1                          # (a loop pair: its node's closing entry)
            pair_of = torch.full((max(nnz, 1),), -1, dtype=torch.int32, device=dev)
            pair_of[torch.where(loop, last, pos)] = k.to(torch.int32)
            maps.append(pair_of)
        self.pair_of, self.t_pair_of = maps


class _StoreBatchHandle:
    """What ``graph.as_graph`` finds on the ``edge_index`` of a store batch: enough to assemble the batch's normalised
    graph of any variant from the store's own (csrc/gda_collate.hip), one graph per (batch, variant)."""

    def __init__(self, store, ids_host, ids, seg_ptr, batch, num_nodes):
        self.store, self.ids_host, self.ids, self.seg_ptr, self.batch = store, ids_host, ids, seg_ptr, batch
        self.num_nodes = num_nodes
        self._graphs, self._ppmi_graphs = {}, {}

    def graph(self, improved, add_self_loops, normalize, degree_side):
        from . import _lib
        from .graph import CSRGraph, RowSplit
        key = _variant_key(improved, add_self_loops, normalize, degree_side)
        g = self._graphs.get(key)
        if g is not None:
            return g
        st, var = self.store, self.store.variant(key)
        B, n = self.ids.numel(), self.num_nodes
        nnz = int(var.nnz[self.ids_host].sum())
        dev = st.device
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        nnz_off = torch.empty(B + 1, dtype=torch.long, device=dev)
        out = (torch.empty(n + 1, **i32), torch.empty(max(nnz, 1), **i32), torch.empty(max(nnz, 1), **f32),
               torch.empty(n + 1, **i32), torch.empty(max(nnz, 1), **i32), torch.empty(max(nnz, 1), **f32))
        c = var.csr
        _lib.call("gda_collate_csr_offsets", self.ids, B, len(st), st.node_ptr, c.rowptr, nnz_off, _lib.stream())
        _lib.call("gda_collate_csr_f32", self.ids, B, len(st), st.node_ptr, self.seg_ptr, self.batch, n, nnz_off, nnz,
                  c.rowptr, c.colidx, c.val, c.t_rowptr, c.t_colidx, c.t_val, *out, _lib.stream())
        # neither `static` nor `transient`: the flags of the graph the host path builds from a collated edge list
        g = CSRGraph(n, nnz, *out)
        g._nnz = nnz                                   # known from the host counts: `nnz` never asks the device
        if not var.hubs[0]:                            # what RowSplit would find out with a read-back per batch
            g._split = RowSplit.without_hubs()
        if not var.hubs[1]:
            g._t_split = RowSplit.without_hubs()
        self._graphs[key] = g
        return g

    def ppmi_graph(self, conv):
        """The batch's normalised PPMI graph for the layer ``conv`` out of a ``ppmi="per_graph"`` store -- what the
        ingestion ``PPMIConv._ppmi_graph`` runs makes of the batch's pair list, bit for bit, without running it: the
        structure is gathered out of the store's own (``_StorePPMI._structure``), the values are the pairs' weights
        with the batch's target count (the pair gather ``gda_collate_ppmi_f32``, as before), normalised by the
        ingestion's arithmetic (``gda_collate_ppmi_csr_f32``: three launches after the entry scan).  Sizes come from
        the host counts: no walk, no sort, no read-back.  One graph per (batch, layer)."""
        from . import _lib
        from .graph import CSRGraph, RowSplit
        g = self._ppmi_graphs.get(conv)
        if g is not None:
            return g
        st, p = self.store, self.store.ppmi_pairs(conv)
        B, n, dev = self.ids.numel(), self.num_nodes, self.store.device
        m, targets, nnz = (int(c[self.ids_host].sum()) for c in (p.pair_counts, p.target_counts, p.entry_counts))
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        # the temporaries as two blocks: the three scans and the pair ids; the pair weights and the rows' deg^-1/2
        longs, floats = torch.empty(3 * (B + 1) + 2 * m, dtype=torch.long, device=dev), torch.empty(m + max(n, 1), **f32)
        ent_off, seg_ptr, pair_off, dis = longs[:B + 1], longs[B + 1:2 * B + 2], longs[2 * B + 2:3 * B + 3], floats[m:]
        out = (torch.empty(n + 1, **i32), torch.empty(max(nnz, 1), **i32), torch.empty(max(nnz, 1), **f32),
               torch.empty(n + 1, **i32), torch.empty(max(nnz, 1), **i32), torch.empty(max(nnz, 1), **f32))
        with torch.cuda.device(dev):
            s = _lib.stream()
            w = None
            if m:                                  # the batch's pair weights: one double log per pair, none without a pair
                pairs, w = longs[3 * B + 3:], floats[:m]
                _lib.call("gda_collate_offsets", self.ids, B, len(st), st.node_ptr, p.pair_ptr, seg_ptr, pair_off, s)
                _lib.call("gda_collate_ppmi_f32", self.ids, B, len(st), p.pair_ptr, pair_off, self.seg_ptr, p.local_src,
                          p.local_dst, p.ratio, p.num_pairs, targets, p.path_len, m, pairs, w, s)
            _lib.call("gda_collate_csr_offsets", self.ids, B, len(st), st.node_ptr, p.rowptr, ent_off, s)
            _lib.call("gda_collate_ppmi_csr_f32", self.ids, B, len(st), st.node_ptr, self.seg_ptr, self.batch, n, ent_off,
                      nnz, p.rowptr, p.colidx, p.pair_of, p.t_rowptr, p.t_colidx, p.t_pair_of, p.num_entries,
                      p.pair_ptr if m else None, pair_off if m else None, w, m, 2.0 if conv.improved else 1.0, *out, dis, s)
        # neither `static` nor `transient`: the flags of the graph the ingestion builds from a pair list
        g = CSRGraph(n, nnz, *out)
        g._nnz = nnz                                   # pairs - loop pairs + nodes: a pair (a, a) becomes a's self loop
        if not p.hubs[0]:
            g._split = RowSplit.without_hubs()
        if not p.hubs[1]:
            g._t_split = RowSplit.without_hubs()
        self._ppmi_graphs[conv] = g
        return g


class _StoreBatch(_GraphBatch):
    """A batch collated on the device: already where the trainer wants it."""

    def to(self, device, non_blocking=False):
        device = torch.device(device)
        if device.type == self.x.device.type and device.index in (None, self.x.device.index):
            return self
        return super().to(device, non_blocking)


class GraphStore(collections.abc.Sequence):
    """A graph-mode dataset kept on ``device``: the features of all graphs as one ``[N_total, F]`` array, per-graph node
    and edge pointers, all edges (graph-local ids), one label per graph -- uploaded once.  ``batch(ids)`` collates the
    graphs ``ids`` there (csrc/gda_collate.hip), bit for bit what ``_collate([graphs[i] for i in ids]).to(device)``
    gives, from nothing but the id list; the batch's normalised graphs are gathered out of the store's own, which are
    built once per variant (``graph.as_graph``).  Graph-mode trainers take a store wherever they take a list of graphs;
    as a ``Sequence`` it yields the graphs it was built from.  On ``device='cpu'`` batches are the host collation of
    the kept graphs.

    ``ppmi``: how ``PPMIConv`` layers get a batch's random-walk PPMI graph.  ``"per_batch"`` (default): from the
    collated edge list, every batch -- fresh walks per batch, what a list of graphs gives.  ``"per_graph"``: every
    layer's walks are drawn once, at its first batch, over the whole dataset in dataset order (the seed from
    ``np.random``, as for a list) and kept per graph for as long as the layer lives; a batch's PPMI graph is gathered
    out of them on the device with no walk and no host wait.  The walks of a graph then no longer change from batch to
    batch -- as in node mode, where a domain's walks are drawn once per layer."""

    PPMI_MODES = ("per_batch", "per_graph")

    def __init__(self, graphs, device, ppmi="per_batch"):
        self.graphs = list(graphs)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if ppmi not in self.PPMI_MODES:
            raise ValueError(f"ppmi must be one of {self.PPMI_MODES}, got {ppmi!r}")
        if ppmi == "per_graph" and self.device.type != "cuda":
            raise ValueError(f"ppmi='per_graph' keeps the walks on a GPU: the store's device is {self.device}")
        self.ppmi = ppmi
        self._ppmi_pairs = weakref.WeakKeyDictionary()        # PPMIConv layer -> _StorePPMI: gone with the layer
        width = None
        for i, g in enumerate(self.graphs):
            x, ei, y = getattr(g, "x", None), getattr(g, "edge_index", None), getattr(g, "y", None)
            if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32:
                raise ValueError(f"graph {i}: x must be a 2-D float32 tensor")
            width = x.size(1) if width is None else width
            if x.size(1) != width:
                raise ValueError(f"graph {i}: x has {x.size(1)} features, the graphs before it {width}")
            if not torch.is_tensor(y) or y.dtype != torch.long or y.numel() != 1:
                raise ValueError(f"graph {i}: y must be one int64 label per graph")
            if not torch.is_tensor(ei) or ei.dim() != 2 or ei.size(0) != 2 or ei.dtype != torch.long:
                raise ValueError(f"graph {i}: edge_index must be an int64 tensor of shape [2, E]")
            if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= x.size(0)):
                raise ValueError(f"graph {i}: edge_index values must lie in [0, {x.size(0)}), found "
                                 f"[{int(ei.min())}, {int(ei.max())}]")
        self.num_features = 0 if width is None else width
        self.node_counts = torch.tensor([g.x.size(0) for g in self.graphs], dtype=torch.long)
        self.edge_counts = torch.tensor([g.edge_index.size(1) for g in self.graphs], dtype=torch.long)
        self._node_ptr_host = torch.zeros(len(self.graphs) + 1, dtype=torch.long)
        self._node_ptr_host[1:] = torch.cumsum(self.node_counts, 0)
        self.num_nodes, self.num_edges = int(self.node_counts.sum()), int(self.edge_counts.sum())
        self._variants = {}
        if self.device.type != "cuda":
            return
        dev = self.device
        gs = self.graphs
        self.x = torch.cat([g.x.cpu() for g in gs] or [torch.empty(0, 0)]).to(dev)
        self.edges = torch.cat([g.edge_index.cpu() for g in gs] or [torch.empty(2, 0, dtype=torch.long)], dim=1).to(dev)
        self.y = torch.cat([g.y.cpu().reshape(-1) for g in gs] or [torch.empty(0, dtype=torch.long)]).to(dev)
        self.node_ptr = self._node_ptr_host.to(dev)
        edge_ptr = torch.zeros(len(self.graphs) + 1, dtype=torch.long)
        edge_ptr[1:] = torch.cumsum(self.edge_counts, 0)
        self.edge_ptr = edge_ptr.to(dev)

    # -- Sequence: the graphs the store was built from ---------------------------------
    def __len__(self):
        return len(self.graphs)

    def __getitem__(self, i):
        return self.graphs[i]

    def _global_edges(self):
        """The edge list of the dataset-order block-diagonal graph (store-global node ids)."""
        return self.edges + torch.repeat_interleave(self._node_ptr_host[:-1], self.edge_counts).to(self.device)

    def variant(self, key):
        """The store's own normalised graph for ``key = (improved, add_self_loops, normalize, degree_side)``, built on
        first use with ``graph.build_csr`` and kept."""
        hit = self._variants.get(key)
        if hit is None:
            hit = self._variants[key] = _StoreVariant(self, key)
        return hit

    def ppmi_pairs(self, conv):
        """The stored PPMI pairs for the layer ``conv`` (``ppmi="per_graph"``), drawn at first use -- the one time this
        (store, layer) pair takes a seed from ``np.random`` and reads anything back -- and kept while the layer lives."""
        if self.ppmi != "per_graph":
            raise ValueError("this store builds PPMI graphs per batch (ppmi='per_batch')")
        from .nn.ppmi_conv import PASSES
        hit = self._ppmi_pairs.get(conv)
        if hit is None or hit.path_len != int(conv.path_len):
            hit = self._ppmi_pairs[conv] = _StorePPMI(self, conv.path_len, PASSES)
        return hit

    def nnz_counts(self, improved=False, add_self_loops=True, normalize=True, degree_side="col"):
        """Stored entries per graph under that normalisation variant (host int64)."""
        return self.variant(_variant_key(improved, add_self_loops, normalize, degree_side)).nnz

    def batch(self, ids):
        """The collated batch of the graphs ``ids`` (a list of ints), in that order, on the store's device."""
        ids = [int(i) for i in ids]
        if not ids:
            raise ValueError("a batch needs at least one graph")
        if self.device.type != "cuda":
            return _collate([self.graphs[i] for i in ids])
        from . import _lib
        B, G, dev = len(ids), len(self.graphs), self.device
        if any(i < -G or i >= G for i in ids):
            raise IndexError(f"graph ids must lie in [{-G}, {G})")
        ids_host = torch.tensor([i % G for i in ids] if G else [], dtype=torch.long)
        n, e = int(self.node_counts[ids_host].sum()), int(self.edge_counts[ids_host].sum())   # host counts: no device query
        stage = torch.empty(B, dtype=torch.long, pin_memory=True)       # (the caching host allocator hands a block out
        stage.copy_(ids_host)                                           # again only once the copy below has run)
        ids_dev = torch.empty(B, dtype=torch.long, device=dev)
        ids_dev.copy_(stage, non_blocking=True)
        return self._collate_on_device(ids_host, ids_dev, n, e)

    def whole_batch(self, ids_dev):
        """The collated batch of ALL graphs in the order the device buffer ``ids_dev`` (int64 ``[len(store)]``, a
        permutation of the ids) holds WHEN THE KERNELS RUN: the fixed-shape form of :meth:`batch` for a captured epoch
        (``hipgraph.GraphedStoreStep``).  Every size of the batch and of its normalised graphs is a sum over all graphs
        and so the same for any permutation; nothing is read from ``ids_dev`` on the host, nothing is staged."""
        G = len(self.graphs)
        if self.device.type != "cuda" or not G or ids_dev.device != self.device or ids_dev.dtype != torch.long \
                or ids_dev.numel() != G:
            raise ValueError("whole_batch needs a device store and its int64 id buffer of len(store) entries")
        return self._collate_on_device(torch.arange(G), ids_dev, self.num_nodes, self.num_edges)

    def _collate_on_device(self, ids_host, ids_dev, n, e):
        """``ids_host`` serves the host COUNTS of the batch and of its graphs only (sums over the chosen graphs)."""
        from . import _lib
        B, G, dev = ids_dev.numel(), len(self.graphs), self.device
        i64 = dict(dtype=torch.long, device=dev)
        x = torch.empty(n, self.num_features, dtype=torch.float32, device=dev)
        edge_index, y, batch = torch.empty(2, e, **i64), torch.empty(B, **i64), torch.empty(n, **i64)
        seg_ptr, edge_off = torch.empty(B + 1, **i64), torch.empty(B + 1, **i64)
        with torch.cuda.device(dev):
            s = _lib.stream()
            _lib.call("gda_collate_offsets", ids_dev, B, G, self.node_ptr, self.edge_ptr, seg_ptr, edge_off, s)
            _lib.call("gda_collate_nodes_f32", ids_dev, B, G, self.node_ptr, seg_ptr, self.x, self.num_features, self.y,
                      n, x, batch, y, s)
            _lib.call("gda_collate_edges", ids_dev, B, G, self.edge_ptr, edge_off, seg_ptr, self.edges, self.num_edges,
                      e, edge_index, s)
        out = _StoreBatch(x=x, edge_index=edge_index, y=y, batch=batch, num_graphs=B)
        batch._gda_sorted, batch._gda_num_graphs, batch._gda_seg_ptr = True, B, seg_ptr
        edge_index._gda_store_batch = _StoreBatchHandle(self, ids_host, ids_dev, seg_ptr, batch, n)
        return out


class StoreLoader(torch.utils.data.DataLoader):
    """``DataLoader(store, batch_size, shuffle)`` whose batches the store collates on its device: torch's own loader
    over ``range(len(store))`` with a collation that returns the id list, so the default CPU generator is consumed
    exactly as by ``DataLoader`` over the list of graphs -- same draws, same batches."""

    def __init__(self, store, batch_size=1, shuffle=False, **kwargs):
        kwargs.pop("collate_fn", None)
        super().__init__(range(len(store)), batch_size=batch_size, shuffle=shuffle, collate_fn=list, **kwargs)
        self.store = store

    def id_batches(self):
        """One epoch's batches as lists of graph ids (the draws happen here, as in ``iter(DataLoader)``)."""
        return super().__iter__()

    def __iter__(self):
        return map(self.store.batch, self.id_batches())


class DataLoader(torch.utils.data.DataLoader):
    """``torch_geometric.loader.DataLoader(dataset, batch_size, shuffle)`` as a2gnn.py:278-286 builds it: torch's own
    loader (its shuffling draws -- the iterator's base seed, then the sampler's seed -- come from the default CPU
    generator exactly as with PyG, whose DataLoader is the same class) with the collation above.  ``dataset``: any
    sequence of ``Data``-like graphs (``x``, ``edge_index``, ``y`` with one label per graph)."""

    def __init__(self, dataset, batch_size=1, shuffle=False, **kwargs):
        kwargs.pop("collate_fn", None)
        super().__init__(dataset, batch_size=batch_size, shuffle=shuffle, collate_fn=_collate, **kwargs)
