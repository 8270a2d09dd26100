"""Regenerate ``gmm_clustering.npz`` by RUNNING THE REFERENCE's ``pygda/nn/gmm_clustering.py`` on the PyG stub with the
shims of ``_jhgda_semantics`` (build container only, needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_golden_gmm [--out DIR]

Recorded: ``Clustering.feature_clustering`` from given initial centres for both metrics, with and without a cluster that
goes empty (inputs of ``tests.test_gmm_host.clustering_inputs``): labels, ``dist2center``, the aligned centres and
``center_change``; and ``GMMClustering.forward(smooth=False)`` on separated embeddings
(``tests.test_gmm_host.separated``) with ``np.random.seed(7)`` -- sklearn's ``random_state=None`` draws its starts from
numpy's global state --: labels, ``dist2center`` and the kept mixture's lower bound.  One CPU thread."""
import argparse
import contextlib
import io
import os

import numpy as np
import torch

from . import _jhgda_semantics, _ref_loader
from .make_golden import HERE, np_

PERM = [2, 0, 3, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    torch.set_num_threads(1)
    from tests.test_gmm_host import clustering_inputs, separated
    ref = _jhgda_semantics.load_jhgda(_ref_loader.load_reference())
    import sys
    G = sys.modules["pygda.nn.gmm_clustering"]
    out = {}
    for dist_type, eps in (("cos", 1e-6), ("euc", 1e-3)):
        for empty in (False, True):
            feat, init = clustering_inputs(empty)
            c = G.Clustering(eps, "cpu", max_len=64, dist_type=dist_type)
            c.set_init_centers(init)
            with contextlib.redirect_stdout(io.StringIO()):
                c.feature_clustering(feat, torch.zeros(len(feat), dtype=torch.int64))
            key = f"clustering/{dist_type}/{int(empty)}/"
            out.update({key + "label": np_(c.samples["label"]), key + "dist2center": np_(c.samples["dist2center"]),
                        key + "centers": np_(c.centers), key + "center_change": np_(c.center_change)})
    cen, lab, x = separated()
    emb = torch.tensor(x, dtype=torch.float32)
    np.random.seed(7)
    g = G.GMMClustering(len(cen), "cpu")
    s = g.forward(torch.tensor(cen[PERM], dtype=torch.float32), emb, torch.tensor(lab), None, None, False, 0.5)
    out.update({"gmm/label": np_(s["label"]), "gmm/dist2center": np_(s["dist2center"]),
                "gmm/lower_bound": np.float64(g.gmm.lower_bound_), "gmm/perm": np.array(PERM)})
    path = os.path.join(args.out, "gmm_clustering.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
