#!/usr/bin/env python
"""``svd_transform`` on the device against the host path, on synthetic stand-ins (distinct uniform random undirected
pairs, mean degree 10, symmetrised: the graphs of bench.make_cfg_a without features):

- seconds of ``svd_transform(data, device=...)`` at N = 2,048 / 9,360 (ACMv9's node count) / 100,000 (k = 1000, panels
  1010 wide), the second of two calls, with the split over its device operations from the profiler's regions of a
  third call (operator applications, Gram matrices, panel products, column moments; the rest is the host's float64
  factorisations of the (k + 10)^2 matrices and the copies around them);
- seconds of the host path (``device=None``: sklearn's TruncatedSVD on the dense [N, N] Laplacian) at the first two
  sizes -- it is not run at 100,000 nodes, where the dense matrix alone is 40 GB.

One JSON line per size, also written to ``--out``.

    python tools/svd_transform_bench.py [--sizes 2048 9360 100000] [--host-up-to 9360] [--out profiles/svd_transform_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pygda_amd import profiler  # noqa: E402
from pygda_amd.data import Data  # noqa: E402
from pygda_amd.utils import svd_transform  # noqa: E402
from _trainer_bench import write_jsonl  # noqa: E402

DEV = "cuda:0"
REGIONS = ("svd_lap_apply", "svd_gram", "svd_panel_matmul", "svd_lap_moments")


def stand_in(n, mean_degree=10, seed=200):
    g = torch.Generator().manual_seed(seed)
    e = n * mean_degree // 2
    a, b = torch.randint(0, n, (2 * e,), generator=g), torch.randint(0, n, (2 * e,), generator=g)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    keys = torch.unique((lo * n + hi)[lo != hi])
    keys = keys[torch.randperm(keys.numel(), generator=g)[:e]]
    lo, hi = keys // n, keys % n
    ei = torch.stack([torch.cat([lo, hi]), torch.cat([hi, lo])])
    return Data(x=torch.zeros(n, 1), edge_index=ei, y=torch.zeros(n, dtype=torch.int64))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 9360, 100000])
    ap.add_argument("--host-up-to", type=int, default=9360)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_transform_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    for n in args.sizes:
        d = stand_in(n)
        first, _ = timed(lambda: svd_transform(d, device=DEV))
        secs, out = timed(lambda: svd_transform(d, device=DEV))
        profiler.start()
        svd_transform(d, device=DEV)
        torch.cuda.synchronize()
        profiler.stop()
        summ = profiler.summary()
        split = {r: round(summ[r]["ms"] / 1e3, 4) for r in REGIONS if r in summ}
        line = {"bench": "svd_transform", "nodes": n, "directed_edges": int(d.edge_index.size(1)),
                "k": int(out.eival.numel()), "device_s": round(secs, 4), "device_first_call_s": round(first, 4),
                "device_split_s": split, "device_other_s": round(secs - sum(split.values()), 4)}
        if n <= args.host_up_to:
            t = time.perf_counter()
            h = svd_transform(stand_in(n))
            line["host_s"] = round(time.perf_counter() - t, 4)
            line["speedup"] = round(line["host_s"] / secs, 2)
            line["eival_max_rel_diff"] = float(((out.eival.cpu() - h.eival).abs() / h.eival).max())
        else:
            line["host_s"] = None
            line["note"] = "host path not run: the dense Laplacian alone is %.0f GB" % (4.0 * n * n / 1e9)
        print(json.dumps(line), flush=True)
        lines.append(line)
    write_jsonl(args.out, lines)


if __name__ == "__main__":
    main()
