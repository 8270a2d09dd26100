"""Graph-mode epochs from lists of graphs against the same epochs from device-resident stores (data.GraphStore), on
seeded stand-ins of the order of the three graph-classification sheets' domains, and the collation kernels' rate.

    python tools/graph_store_bench.py fit --out fit.jsonl            # A2GNN epochs, list and store input alternated
    python tools/graph_store_bench.py fit --lists-only --out p.jsonl # the same tool in a checkout without the store
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python tools/graph_store_bench.py collate --shape frankenstein --batch-size 0 --out DIR/collate.json
    python tools/graph_store_bench.py merge --fit fit.jsonl --parent p.jsonl --collate DIR... --out profiles/graph_store_bench.jsonl

    python tools/graph_store_bench.py ppmi --out ppmi.jsonl          # UDAGCN(ppmi=True): list, store per batch, store per graph
    python tools/graph_store_bench.py ppmi --kinds store --out p.jsonl   # the same tool in a checkout without ppmi="per_graph"
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python tools/graph_store_bench.py collate --ppmi --shape proteins --batch-size 64 --out DIR/collate.json
    python tools/graph_store_bench.py merge-ppmi --fit ppmi.jsonl --parent p.jsonl --collate DIR... --out profiles/graph_store_ppmi_bench.jsonl

    python tools/graph_store_bench.py capture --out c.jsonl          # store epochs eager and captured, alternated
    python tools/graph_store_bench.py capture --modes eager --out p.jsonl   # this file copied into a checkout of the parent
    python tools/graph_store_bench.py order --out o.jsonl            # an eager epoch before and after captured fits
    python tools/graph_store_bench.py merge-capture --fit c.jsonl --parent p.jsonl --collate DIR... --out profiles/graph_store_capture_bench.jsonl

``fit`` (and ``ppmi``, the same loop around UDAGCN with its PPMI encoder) times whole epochs on a host clock behind a device synchronise (the epoch hook), after warm-up epochs, over
windows of about ``--window`` seconds.  ``collate`` only draws batches and their default-variant graphs: it is the run
the kernel times come from.  ``merge`` (no device) joins them: bytes moved per batch from shapes, over the kernels'
time per batch, over the HBM peak.  The sizes are stand-ins: only their order of magnitude is meant."""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools._trainer_bench import collector, write_jsonl  # noqa: E402

# one domain (half a dataset) each
SHAPES = {"mutagenicity": dict(graphs=2170, nodes=30, edges=62, F=14),
          "proteins": dict(graphs=560, nodes=39, edges=146, F=4),
          "frankenstein": dict(graphs=2170, nodes=17, edges=36, F=780)}
HBM_PEAK = 6.29e12            # bytes/s, the measured float4 copy of MI355X_MICROARCH.md (8.0e12 by specification)
DEV = "cuda:0"


def domain(graphs, nodes, edges, F, seed):
    """``graphs`` random undirected graphs of ``nodes`` +- 50 % nodes, ``edges`` directed edges at the mean size."""
    from pygda_amd.data import Data
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(max(nodes // 2, 1), nodes + nodes // 2 + 1, (graphs,), generator=g).tolist()
    out = []
    for n in sizes:
        half = int(round(edges / 2 * n / nodes))
        s, d = torch.randint(0, n, (half,), generator=g), torch.randint(0, n, (half,), generator=g)
        out.append(Data(x=torch.randn(n, F, generator=g), edge_index=torch.stack([torch.cat([s, d]), torch.cat([d, s])]),
                        y=torch.randint(0, 2, (1,), generator=g)))
    return out


def batch_bytes(n, e, B, F, nnz):
    """Bytes the collation kernels read plus write for one batch of ``B`` graphs, ``n`` nodes, ``e`` edges (features,
    edge list, labels, graph index) and for its normalised graph of ``nnz`` stored entries (both orientations)."""
    collate = 2 * n * F * 4 + 2 * (2 * e * 8) + 2 * B * 8 + n * 8
    graph = 2 * (2 * (n + 1) * 4 + 2 * nnz * 8)
    return collate, graph


def epoch_ms(src, tgt, F, batch_size, epochs, warm, trainer="a2gnn", split=False, **kw):
    """``(ms per epoch, last loss)`` of one graph-mode fit at the sheets' settings: A2GNN, or UDAGCN with PPMI."""
    import numpy as np
    from pygda_amd.models import A2GNN, UDAGCN
    from pygda_amd.ops import dropout_state
    common = dict(mode='graph', device=DEV, epoch=warm + epochs, verbose=0, batch_size=batch_size, **kw)
    if trainer == "a2gnn":
        m = A2GNN(F, 128, 2, num_layers=2, dropout=0.5, s_pnums=0, t_pnums=10, weight=10, lr=0.01, weight_decay=0.005,
                  **common)
    else:
        m = UDAGCN(F, 128, 2, num_layers=3, dropout=0.1, ppmi=True, adv_dim=40, lr=0.001, weight_decay=0.005, **common)
    np.random.seed(0)                                 # the PPMI walks' seeds
    stamps, losses = [], []

    cpu = []

    def hook(e, loss, acc, secs):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        cpu.append(time.thread_time())                # on-core time of the training thread so far
        losses.append(float(loss))

    m.epoch_hook = hook
    torch.manual_seed(0)
    for counter in dropout_state.step.values():       # the masks' step counter outlives a fit: the same masks every time
        counter.zero_()
    m.fit(src, tgt)
    if split:      # (ms per epoch, of which the training thread was on a core)
        return (stamps[-1] - stamps[warm - 1]) / epochs * 1e3, (cpu[-1] - cpu[warm - 1]) / epochs * 1e3
    return (stamps[-1] - stamps[warm - 1]) / epochs * 1e3, losses[-1]


def run_fit(a):
    emit, lines = collector()
    for name in a.shapes:
        sh = SHAPES[name]
        src, tgt = domain(seed=1, **sh), domain(seed=2, **sh)
        inputs = {"list": (src, tgt)} if "list" in a.kinds else {}
        upload_ms = None
        if "store" in a.kinds:
            from pygda_amd.data import GraphStore
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inputs["store"] = (GraphStore(src, DEV), GraphStore(tgt, DEV))
            torch.cuda.synchronize()
            upload_ms = round((time.perf_counter() - t0) * 1e3, 1)
        if "per_graph" in a.kinds:
            from pygda_amd.data import GraphStore
            inputs["per_graph"] = (GraphStore(src, DEV, ppmi="per_graph"), GraphStore(tgt, DEV, ppmi="per_graph"))
        for bs in a.batch_sizes:
            line = dict(shape=name, **sh, batch_size=bs, batches_per_epoch=math.ceil(sh["graphs"] / (bs or sh["graphs"])),
                        upload_ms_once=upload_ms, trainer=a.trainer)
            if "per_graph" in inputs and bs == a.batch_sizes[0]:
                line["walks_ms_once_per_store_and_layer"] = walks_ms(inputs["per_graph"][0])
            plan, pilot_loss = {}, {}
            for kind, (s, t) in inputs.items():           # a short fit: warms every shape, sizes the window
                pilot, pilot_loss[kind] = epoch_ms(s, t, sh["F"], bs, 2, 1, a.trainer)
                plan[kind] = max(3, min(a.max_epochs, math.ceil(a.window * 1e3 / pilot)))
            times, last = {k: [] for k in inputs}, {}
            if "store" in inputs and "list" in inputs:    # three epochs each from the same seeds: the same number
                line["pilot_losses_equal"] = pilot_loss["store"] == pilot_loss["list"]
                line["pilot_loss"] = pilot_loss["store"]
            for _ in range(a.repeats):                    # alternated, so that drift hits both alike
                for kind, (s, t) in inputs.items():
                    ms, last[kind] = epoch_ms(s, t, sh["F"], bs, plan[kind], 2, a.trainer)
                    times[kind].append(round(ms, 3))
            for kind in inputs:
                line[f"{kind}_ms_per_epoch"] = times[kind]
                line[f"{kind}_epochs_per_window"] = plan[kind]
                line[f"{kind}_last_loss"] = last[kind]       # (windows differ in length: not comparable across kinds)
            emit(line)
    write_jsonl(a.out, lines)


# (trainer, batch size, store kind): the two captured shapes of a sheet, and the eager mini-batch epoch that isolates the
# sort-free PPMI assembly
CAPTURE_CASES = [("a2gnn", 0, "store"), ("udagcn-ppmi", 0, "per_graph"), ("udagcn-ppmi", 64, "per_graph")]


def run_capture(a):
    """Store epochs with the hipGraph switch off and on (one batch per domain: the captured epoch), alternated."""
    from pygda_amd.data import GraphStore
    emit, lines = collector()
    for name in a.shapes:
        sh = SHAPES[name]
        src, tgt = domain(seed=1, **sh), domain(seed=2, **sh)
        stores = {"store": (GraphStore(src, DEV), GraphStore(tgt, DEV)),
                  "per_graph": (GraphStore(src, DEV, ppmi="per_graph"), GraphStore(tgt, DEV, ppmi="per_graph"))}
        for trainer, bs, kind in CAPTURE_CASES:
            s, t = stores[kind]
            modes = [m for m in a.modes if bs == 0 or m == "eager"]
            run = lambda mode, epochs, warm: epoch_ms(s, t, sh["F"], bs, epochs, warm, trainer,      # noqa: E731
                                                      use_hip_graph=mode == "captured")
            line = dict(shape=name, **sh, batch_size=bs, trainer=trainer, store=kind,
                        batches_per_epoch=math.ceil(sh["graphs"] / (bs or sh["graphs"])))
            plan, pilot_loss = {}, {}
            for mode in modes:                            # a short fit: warms every shape, sizes the window
                pilot, pilot_loss[mode] = run(mode, 2, 1)
                plan[mode] = max(3, min(a.max_epochs, math.ceil(a.window * 1e3 / pilot)))
            if len(modes) == 2:                           # three epochs each from the same seeds: the same number
                line["pilot_losses_equal"] = pilot_loss["eager"] == pilot_loss["captured"]
            times = {m: [] for m in modes}
            for _ in range(a.repeats):
                for mode in modes:
                    times[mode].append(round(run(mode, plan[mode], 2)[0], 3))
            for mode in modes:
                line[f"{mode}_ms_per_epoch"] = times[mode]
                line[f"{mode}_epochs_per_window"] = plan[mode]
            emit(line)
    write_jsonl(a.out, lines)


def run_order(a):
    """One process: an eager mini-batch UDAGCN fit on fresh stores, then captured one-batch fits, then the same eager
    fit again -- ms per epoch, of which the training thread was on a core, the time the cyclic collector took, the
    objects it tracks and what the allocator holds: does an eager epoch that follows captured fits cost more, and where?"""
    import gc
    spent = [0.0, 0.0]

    def on_gc(phase, info):
        if phase == "start":
            spent[1] = time.perf_counter()
        else:
            spent[0] += time.perf_counter() - spent[1]

    gc.callbacks.append(on_gc)
    from pygda_amd.data import GraphStore
    emit, lines = collector()
    sh = SHAPES[a.shape]
    src, tgt = domain(seed=1, **sh), domain(seed=2, **sh)
    plain = (GraphStore(src, DEV), GraphStore(tgt, DEV))
    pg = (GraphStore(src, DEV, ppmi="per_graph"), GraphStore(tgt, DEV, ppmi="per_graph"))

    def eager(phase):
        epoch_ms(*pg, sh["F"], a.batch_size, 2, 1, "udagcn-ppmi", use_hip_graph=False)          # warms the shapes
        for rep in range(a.repeats):
            spent[0] = 0.0
            ms, on_core = epoch_ms(*pg, sh["F"], a.batch_size, a.epochs, 2, "udagcn-ppmi", split=True, use_hip_graph=False)
            emit(dict(shape=a.shape, batch_size=a.batch_size, phase=phase, window=rep, ms_per_epoch=round(ms, 3),
                      thread_on_core_ms_per_epoch=round(on_core, 3),
                      collector_ms_per_fit=round(spent[0] * 1e3, 2), tracked_objects=len(gc.get_objects()),
                      reserved_mb=round(torch.cuda.memory_reserved() / 2 ** 20, 1),
                      allocated_mb=round(torch.cuda.memory_allocated() / 2 ** 20, 1)))

    eager("before any captured fit")
    for _ in range(a.captured_fits):
        epoch_ms(*plain, sh["F"], 0, 20, 2, "a2gnn", use_hip_graph=True)
        epoch_ms(*pg, sh["F"], 0, 20, 2, "udagcn-ppmi", use_hip_graph=True)
    eager(f"after {2 * a.captured_fits} captured fits")
    write_jsonl(a.out, lines)


def run_merge_capture(a):
    med = statistics.median
    parent = {}
    for l in (open(a.parent) if a.parent else ()):
        d = json.loads(l)
        parent[d["shape"], d["trainer"], d["batch_size"]] = d["eager_ms_per_epoch"]
    kern = {}
    for d in a.collate:
        meta = json.load(open(os.path.join(d, "collate.json")))
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
        rows = list(csv.DictReader(open(stats)))
        us = lambda word: round(sum(float(r["TotalDurationNs"]) for r in rows if word in r["Name"]) / meta["batches"] / 1e3, 2)
        kern[meta["shape"], meta["batch_size"]] = dict(
            entries_per_batch=round(meta["entries_per_batch"]),
            ppmi_pair_gather_us_per_batch=us("k_collate_ppmi"), ppmi_csr_gather_us_per_batch=us("k_ppmi_csr_gather"), ppmi_csr_degree_us_per_batch=us("k_ppmi_csr_degree"),
            ppmi_csr_scale_us_per_batch=us("k_ppmi_csr_scale"), all_scans_us_per_batch=us("k_collate_scan"),
            kernel_time_source="rocprofv3 --kernel-trace --stats, a run of its own")
    lines = []
    for l in open(a.fit):
        d = json.loads(l)
        key = (d["shape"], d["trainer"], d["batch_size"])
        if key in parent:
            d["parent_eager_ms_per_epoch"] = parent[key]
        if "captured_ms_per_epoch" in d:
            d["captured_over_eager"] = round(med(d["captured_ms_per_epoch"]) / med(d["eager_ms_per_epoch"]), 4)
            d["captured_not_slower"] = med(d["captured_ms_per_epoch"]) <= med(d["eager_ms_per_epoch"])
        elif key in parent:
            spread = max(d["eager_ms_per_epoch"]) - min(d["eager_ms_per_epoch"])
            d["eager_over_parent"] = round(med(d["eager_ms_per_epoch"]) / med(parent[key]), 4)
            d["not_slower_than_parent_by_more_than_the_spread"] = med(d["eager_ms_per_epoch"]) - med(parent[key]) <= spread
        if d["trainer"] == "udagcn-ppmi":
            d.update(kern.get((d["shape"], d["batch_size"]), {}))
        lines.append(d)
        print(json.dumps(d))
    write_jsonl(a.out, lines, stamp=False)


def walks_ms(store):
    """ms of the one-off walk build of a ``per_graph`` store for one layer (second of two: the first warms)."""
    from pygda_amd.nn.ppmi_conv import PPMIConv
    for _ in range(2):
        conv = PPMIConv(store.num_features, 128)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store.ppmi_pairs(conv)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    return round(ms, 2)


def run_collate_ppmi(a):
    """Only draws batches and one layer's PPMI graph of each from a ``per_graph`` store."""
    from pygda_amd.data import GraphStore, StoreLoader
    from pygda_amd.nn.ppmi_conv import PPMIConv
    sh = SHAPES[a.shape]
    store = GraphStore(domain(seed=1, **sh), DEV, ppmi="per_graph")
    conv = PPMIConv(sh["F"], 128)
    loader = StoreLoader(store, batch_size=a.batch_size or len(store), shuffle=True)
    torch.manual_seed(0)
    batches = pairs = nodes = entries = 0
    for _ in range(a.epochs):
        for b in loader:
            g = b.edge_index._gda_store_batch.ppmi_graph(conv)
            h = b.edge_index._gda_store_batch
            pairs += int(store.ppmi_pairs(conv).pair_counts[h.ids_host].sum())     # (host counts, pairs (a, a) included)
            entries += g.nnz
            nodes += b.x.size(0)
            batches += 1
    torch.cuda.synchronize()
    with open(a.out, "w") as fh:
        # per pair: two int32 ids and a double in, two int64 ids and a float out
        json.dump(dict(shape=a.shape, batch_size=a.batch_size, batches=batches, pairs_per_batch=pairs / batches,
                       nodes_per_batch=nodes / batches, entries_per_batch=entries / batches,
                       ppmi_bytes_per_batch=pairs / batches * (16 + 20)), fh)


def run_merge_ppmi(a):
    parent = {}
    for l in (open(a.parent) if a.parent else ()):
        d = json.loads(l)
        parent[d["shape"], d["batch_size"]] = d
    kern = {}
    for d in a.collate:
        meta = json.load(open(os.path.join(d, "collate.json")))
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
        rows = list(csv.DictReader(open(stats)))
        ns = lambda word: sum(float(r["TotalDurationNs"]) for r in rows if word in r["Name"]) / meta["batches"]
        kern[meta["shape"], meta["batch_size"]] = dict(
            pairs_per_batch=round(meta["pairs_per_batch"]), ppmi_bytes_per_batch=round(meta["ppmi_bytes_per_batch"]),
            ppmi_gather_us_per_batch=round(ns("k_collate_ppmi") / 1e3, 2),
            ppmi_gather_bytes_per_s=round(meta["ppmi_bytes_per_batch"] / (ns("k_collate_ppmi") * 1e-9)),
            all_scans_us_per_batch=round(ns("k_collate_scan") / 1e3, 2),
            kernel_time_source="rocprofv3 --kernel-trace --stats, a run of its own")
    lines = []
    med = statistics.median
    for l in open(a.fit):
        d = json.loads(l)
        key = (d["shape"], d["batch_size"])
        if key in parent:
            d["parent_store_ms_per_epoch"] = parent[key]["store_ms_per_epoch"]
        d["per_graph_over_per_batch"] = round(med(d["per_graph_ms_per_epoch"]) / med(d["store_ms_per_epoch"]), 4)
        d["per_graph_not_slower"] = med(d["per_graph_ms_per_epoch"]) <= med(d["store_ms_per_epoch"])
        d.update(kern.get(key, {}))
        lines.append(d)
        print(json.dumps(d))
    write_jsonl(a.out, lines, stamp=False)


def run_collate(a):
    if a.ppmi:
        return run_collate_ppmi(a)
    from pygda_amd.data import GraphStore, StoreLoader
    from pygda_amd.graph import as_graph
    sh = SHAPES[a.shape]
    graphs = domain(seed=1, **sh)
    store = GraphStore(graphs, DEV)
    bs = a.batch_size or len(store)
    loader = StoreLoader(store, batch_size=bs, shuffle=True)
    torch.manual_seed(0)
    batches, tot = 0, [0, 0, 0]
    for _ in range(a.epochs):
        for b in loader:
            g = as_graph(b.edge_index, b.x.size(0))
            c, gr = batch_bytes(b.x.size(0), b.edge_index.size(1), b.num_graphs, sh["F"], g.nnz)
            tot[0] += c
            tot[1] += gr
            tot[2] += 2 * b.x.numel() * 4
            batches += 1
    torch.cuda.synchronize()
    with open(a.out, "w") as fh:
        json.dump(dict(shape=a.shape, batch_size=a.batch_size, batches=batches, collate_bytes_per_batch=tot[0] / batches,
                       graph_bytes_per_batch=tot[1] / batches, feature_bytes_per_batch=tot[2] / batches), fh)


def run_merge(a):
    parent = {}
    for l in (open(a.parent) if a.parent else ()):
        d = json.loads(l)
        parent[d["shape"], d["batch_size"]] = d
    kern = {}
    for d in a.collate:
        meta = json.load(open(os.path.join(d, "collate.json")))
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
        rows = [r for r in csv.DictReader(open(stats)) if "k_collate" in r["Name"]]
        ns = lambda pick: sum(float(r["TotalDurationNs"]) for r in rows if pick(r["Name"])) / meta["batches"]
        graph_ns = ns(lambda k: "rowptr" in k or "entries" in k)
        scan_ns = ns(lambda k: "scan" in k)
        copy_ns = ns(lambda k: "scan" not in k and "rowptr" not in k and "entries" not in k)
        moved = meta["collate_bytes_per_batch"] + meta["graph_bytes_per_batch"]
        rate = moved / ((graph_ns + scan_ns + copy_ns) * 1e-9)
        rows_ns = ns(lambda k: "k_collate_rows" in k)               # the feature gather: nearly all of the bytes at a wide F
        rows_rate = meta["feature_bytes_per_batch"] / (rows_ns * 1e-9)
        kern[meta["shape"], meta["batch_size"]] = dict(
            feature_gather_us_per_batch=round(rows_ns / 1e3, 2), feature_gather_bytes_per_s=round(rows_rate),
            feature_gather_share_of_hbm_peak=round(rows_rate / HBM_PEAK, 4),
            collate_bytes_per_batch=round(meta["collate_bytes_per_batch"]), graph_bytes_per_batch=round(meta["graph_bytes_per_batch"]),
            collate_kernels_us_per_batch=round((graph_ns + scan_ns + copy_ns) / 1e3, 2),
            of_which_scans_us=round(scan_ns / 1e3, 2), of_which_graph_gather_us=round(graph_ns / 1e3, 2),
            collate_bytes_per_s=round(rate), share_of_hbm_peak=round(rate / HBM_PEAK, 4), hbm_peak_bytes_per_s=HBM_PEAK,
            kernel_time_source="rocprofv3 --kernel-trace --stats, a run of its own")
    lines = []
    for l in open(a.fit):
        d = json.loads(l)
        key = (d["shape"], d["batch_size"])
        if key in parent:
            d["parent_list_ms_per_epoch"] = parent[key]["list_ms_per_epoch"]
            d["store_over_parent_list"] = round(statistics.median(d["store_ms_per_epoch"])
                                                / statistics.median(parent[key]["list_ms_per_epoch"]), 4)
        d.update(kern.get(key, {}))
        lines.append(d)
        print(json.dumps(d))
    write_jsonl(a.out, lines, stamp=False)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    for cmd in ("fit", "ppmi"):
        f = sub.add_parser(cmd)
        f.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
        f.add_argument("--batch-sizes", nargs="+", type=int, default=[0, 64])
        f.add_argument("--repeats", type=int, default=3)
        f.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
        f.add_argument("--max-epochs", type=int, default=300)
        f.add_argument("--out", default=None)
        if cmd == "fit":
            f.add_argument("--lists-only", action="store_true", help="for a checkout that has no GraphStore (the baseline)")
        else:
            f.add_argument("--kinds", nargs="+", default=["list", "store", "per_graph"], choices=["list", "store", "per_graph"],
                           help="'store' is the default store (PPMI graphs per batch); a checkout without "
                                "ppmi='per_graph' runs --kinds store")
    cp = sub.add_parser("capture")
    cp.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    cp.add_argument("--modes", nargs="+", default=["eager", "captured"], choices=["eager", "captured"],
                    help="a checkout without captured store epochs runs --modes eager")
    cp.add_argument("--repeats", type=int, default=3)
    cp.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    cp.add_argument("--max-epochs", type=int, default=300)
    cp.add_argument("--out", default=None)
    od = sub.add_parser("order")
    od.add_argument("--shape", default="proteins", choices=list(SHAPES))
    od.add_argument("--batch-size", type=int, default=64)
    od.add_argument("--epochs", type=int, default=20)
    od.add_argument("--repeats", type=int, default=3)
    od.add_argument("--captured-fits", type=int, default=3)
    od.add_argument("--out", default=None)
    mc = sub.add_parser("merge-capture")
    mc.add_argument("--fit", required=True)
    mc.add_argument("--parent", default=None, help="the parent commit's `capture --modes eager` lines")
    mc.add_argument("--collate", nargs="*", default=[], help="directories of the `collate --ppmi` runs")
    mc.add_argument("--out", required=True)
    c = sub.add_parser("collate")
    c.add_argument("--shape", required=True, choices=list(SHAPES))
    c.add_argument("--batch-size", type=int, default=0)
    c.add_argument("--epochs", type=int, default=20)
    c.add_argument("--ppmi", action="store_true", help="a per_graph store's batches and one layer's PPMI graphs")
    c.add_argument("--out", required=True)
    m = sub.add_parser("merge")
    m.add_argument("--fit", required=True)
    m.add_argument("--parent", default=None)
    m.add_argument("--collate", nargs="*", default=[], help="directories of the collate runs (collate.json + the trace)")
    m.add_argument("--out", required=True)
    mp = sub.add_parser("merge-ppmi")
    mp.add_argument("--fit", required=True)
    mp.add_argument("--parent", default=None, help="the parent commit's `ppmi --kinds store` lines")
    mp.add_argument("--collate", nargs="*", default=[], help="directories of the `collate --ppmi` runs")
    mp.add_argument("--out", required=True)
    a = p.parse_args()
    if not a.cmd.startswith("merge") and not torch.cuda.is_available():
        raise SystemExit("graph_store_bench: no GPU (timings are taken on the device or not at all)")
    if a.cmd == "fit":
        a.trainer, a.kinds = "a2gnn", ["list"] if a.lists_only else ["list", "store"]
    elif a.cmd == "ppmi":
        a.trainer = "udagcn-ppmi"
    {"fit": run_fit, "ppmi": run_fit, "collate": run_collate, "merge": run_merge, "merge-ppmi": run_merge_ppmi,
     "capture": run_capture, "merge-capture": run_merge_capture, "order": run_order}[a.cmd](a)


if __name__ == "__main__":
    main()
