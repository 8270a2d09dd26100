#!/usr/bin/env python
"""The device fit of ``pygda.nn.GMMClustering`` against sklearn's own fit on the host, on synthetic embeddings (K
anisotropic Gaussians, centres 4 sigma apart) at the citation shapes (N, d, K, n_init) = (7410, 128, 6, 5) and
(5578, 64, 5, 5):

- seconds of ``init_resp`` (the seeded k-means of the five starts) and of ``fit_em`` (EM for the five runs at once) on
  the device, the second of two calls, with the split over the kernels from the profiler's regions of a third call;
- seconds of ``sklearn.mixture.GaussianMixture(K, n_init=5).fit`` on the same array on ``--threads`` host threads (16 by
  default: the quota of a job, not the machine's core count).

sklearn draws its own starts, so iteration counts differ; both are reported.  One JSON line per case, ``data:
synthetic``, also written to ``--out``.

    python tools/gmm_bench.py [--threads 16] [--out profiles/gmm_bench.jsonl] [--case N,d,K,n_init] [--skip-host]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((7410, 128, 6, 5), (5578, 64, 5, 5))
REGIONS = ("gmm_estep", "gmm_mstep", "gmm_factor", "kmeans_step")
DEV = "cuda:0"


def embeddings(n, d, k, seed=300):
    import numpy as np
    rng = np.random.RandomState(seed)
    cen = rng.normal(size=(k, d)) * 4.0 / np.sqrt(2 * d)
    lab = rng.randint(0, k, n)
    mix = [np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d) for _ in range(k)]
    return np.stack([cen[c] + mix[c] @ rng.normal(size=d) for c in lab]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm_bench.jsonl"))
    ap.add_argument("--case", default=None, help="N,d,K,n_init instead of the two citation shapes")
    ap.add_argument("--skip-host", action="store_true", help="leave sklearn's fit out")
    args = ap.parse_args()
    cases = (tuple(int(v) for v in args.case.split(",")),) if args.case else CASES
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[var] = str(args.threads)                      # before numpy loads its BLAS
    import torch
    from sklearn.mixture import GaussianMixture
    from pygda_amd import profiler
    from pygda_amd.nn.gmm_clustering import GMMClustering
    from _trainer_bench import write_jsonl

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    lines = []
    for n, d, k, n_init in cases:
        x_host = embeddings(n, d, k)
        x = torch.from_numpy(x_host).to(DEV)
        c = GMMClustering(k, DEV, n_init=n_init, seed=0)
        timed(lambda: c.fit_em(x, c.init_resp(x)))                                   # first call: workspaces, attributes
        init_s, resp0 = timed(lambda: c.init_resp(x))
        fit_s, model = timed(lambda: c.fit_em(x, resp0))
        profiler.start()
        c.fit_em(x, c.init_resp(x))
        torch.cuda.synchronize()
        profiler.stop()
        summ = profiler.summary()
        split = {r: round(summ[r]["ms"] / 1e3, 5) for r in REGIONS if r in summ}
        line = {"bench": "gmm_fit", "data": "synthetic", "n": n, "d": d, "components": k, "n_init": n_init,
                "device_init_s": round(init_s, 4), "device_fit_s": round(fit_s, 4), "device_split_s": split,
                "device_n_iter_kept_run": model.n_iter_, "device_lower_bound": round(model.lower_bound_, 4)}
        if not args.skip_host:
            t = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = GaussianMixture(k, n_init=n_init, random_state=0).fit(x_host)
            host_s = time.perf_counter() - t
            line.update({"host_threads": args.threads, "host_fit_s": round(host_s, 4),
                         "host_n_iter_kept_run": int(ref.n_iter_), "host_lower_bound": round(float(ref.lower_bound_), 4),
                         "host_over_device": round(host_s / (init_s + fit_s), 2)})
        print(json.dumps(line), flush=True)
        lines.append(line)
    write_jsonl(args.out, lines)


if __name__ == "__main__":
    main()
