"""Captured epochs for the trainers that write their own epoch (ASN, JHGDA, SEPA; ACDNE for its steps).

A trainer supplies ``epoch_fn(u)``: one whole epoch (forward, loss, backward, optimiser step) that leaves its loss in
``trainer._loss_buf[u]`` and its count of correct source predictions in ``trainer._hit_buf[u]``.  :func:`run_epochs`
records ``slots`` such epochs into one hipGraph and replays it, reads the two buffers once per replay, and runs what
does not fill a replay (or every epoch, with the graph off) eagerly through slot 0, so eager and captured fits take
the same kernels on the same values.  Nothing here knows a trainer: what one needs around a group it passes in as a
callable."""
import time

import torch


def rollback(params, saved, optimizers):
    """Undo warm-up steps: ``saved`` copied back into ``params``, every tensor of every optimiser's state zeroed (a
    fresh optimiser: step counts and moments start from zero)."""
    with torch.no_grad():
        for p, v in zip(params, saved):
            p.copy_(v)
        for o in optimizers:
            for st in o.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()


def capture_rolled_back(call, U, params, optimizers, also=()):
    """``call(0) .. call(U - 1)`` recorded into one hipGraph, which is returned.  ``call(0)`` first runs once on a side
    stream (allocations, lazy initialisation); that warm-up and whatever the recording itself ran are rolled back --
    ``params``, the optimisers' state and every tensor in ``also`` (counters, accumulators) -- so a fit takes exactly
    the eager steps."""
    params = list(params)
    saved = [p.detach().clone() for p in params]
    kept = [t.clone() for t in also]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for u in range(U):
            call(u)
    rollback(params, saved, optimizers)
    with torch.no_grad():
        for t, v in zip(also, kept):
            t.copy_(v)
    return graph


def replay_groups(total, U, use_graph):
    """``(first_epoch, k)`` over ``total`` epochs: groups of ``k == U`` while replays are wanted, the fit has at least
    ``U`` epochs and ``U`` remain; single epochs otherwise."""
    epoch = 0
    while epoch < total:
        k = U if use_graph and total >= U and total - epoch >= U else 1
        yield epoch, k
        epoch += k


def run_epochs(trainer, epoch_fn, n_source, slots, use_graph, before_group=None, after_group=None, also=()):
    """``trainer.epoch`` epochs of ``epoch_fn``, ``slots`` per replay when ``use_graph``, with one log line per epoch
    (loss, hits / ``n_source``).  ``before_group(first_epoch, k)`` runs ahead of each group (schedules that the epochs
    read from the device), ``after_group(k)`` after its read-back (a trainer's further slot buffers); ``also`` as in
    :func:`capture_rolled_back`.  Of ``trainer`` it uses ``device``, ``epoch``, ``optimizer`` (the one optimiser over
    every trained parameter: its ``param_groups`` are what the capture rolls back) and ``_report``, and it sets
    ``_loss_buf`` / ``_hit_buf``, which ``epoch_fn`` fills."""
    dev = torch.device(trainer.device)
    trainer._loss_buf = torch.zeros(slots, dtype=torch.float32, device=dev)
    trainer._hit_buf = torch.zeros(slots, dtype=torch.int64, device=dev)
    graph = None
    start = time.time()
    for epoch, k in replay_groups(trainer.epoch, slots, use_graph):
        if before_group is not None:
            before_group(epoch, k)
        if use_graph and k == slots:
            if graph is None:
                params = [p for g in trainer.optimizer.param_groups for p in g["params"]]
                graph = capture_rolled_back(epoch_fn, slots, params, [trainer.optimizer], also)
            graph.replay()
        else:
            epoch_fn(0)
        losses, hits = trainer._loss_buf[:k].tolist(), trainer._hit_buf[:k].tolist()
        if after_group is not None:
            after_group(k)
        for u in range(k):
            trainer._report(epoch + u, losses[u], hits[u] / n_source, start)
