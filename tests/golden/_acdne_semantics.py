"""ACDNE restated in float64, independent of the reference's files: the arbiter of the fixtures' fp32 numbers.

Everything the reference computes is computed here in float64 -- process_graph, the batch PPMI blocks, the network,
the three losses and torch's Adam -- from the same initial parameters and the same ``np.random`` index draws
(pygda_amd.models.acdne.epoch_indices, which the host tests check against the reference's generator).  Dropout is 0.
"""
import numpy as np
import torch
import torch.nn.functional as F


def process_graph(edge_index, x, n, step):
    """(A_ppmi, X_nei) in float64; the adjacency sized by n (duplicates summed)."""
    adj = np.zeros((n, n))
    np.add.at(adj, (edge_index[0], edge_index[1]), 1.0)

    def scale(w):
        s = w.sum(1)
        r = np.where(s + 1e-12 > 0, 1.0 / (s + 1e-12), 0.0)
        return r[:, None] * w

    g = scale(adj)
    a_k, a = g, g.copy()
    for k in range(2, step + 1):
        a_k = a_k @ g
        a = a + a_k / k
    np.fill_diagonal(a, 0)
    a = scale(a)
    col = a.sum(0)
    col[col == 0] = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        ppmi = np.log(n * a / col[None, :] + 1e-12)
    ppmi[np.isnan(ppmi)] = 0
    ppmi[ppmi < 0] = 0
    return ppmi, scale(ppmi) @ np.asarray(x, dtype=np.float64)


def batch_block(ppmi, idx):
    a = ppmi[np.ix_(idx, idx)].copy()
    np.fill_diagonal(a, 0)
    s = a.sum(1)
    return (1.0 / (s + 1e-12))[:, None] * a


def fit(src, tgt, init_state, hid, n_emb, num_classes, step, pair_weight, lr, weight_decay, epochs, batch_size,
        np_seed):
    """``src`` / ``tgt``: dicts of numpy arrays x, ei, y.  Returns per-epoch losses, the final state and the two
    predict outputs (softmax probabilities)."""
    from pygda_amd.models.acdne import epoch_indices
    ns, nt = len(src["x"]), len(tgt["x"])
    ps, xns = process_graph(src["ei"], src["x"], ns, step)
    pt, xnt = process_graph(tgt["ei"], tgt["x"], nt, step)
    X = torch.tensor(np.concatenate([src["x"], tgt["x"]]), dtype=torch.float64)
    Xn = torch.tensor(np.concatenate([xns, xnt]), dtype=torch.float64)
    ys = torch.tensor(src["y"], dtype=torch.int64)
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in init_state.items()}
    names = list(P)
    opt = torch.optim.Adam([P[k] for k in names], lr=lr, weight_decay=weight_decay, foreach=False)
    lin = lambda x, n: F.linear(x, P[n + ".weight"], P[n + ".bias"])        # noqa: E731

    def embed(x, xn):
        h1 = F.relu(lin(F.relu(lin(x, "network_embedding.fe1.h1_self")), "network_embedding.fe1.h2_self"))
        h2 = F.relu(lin(F.relu(lin(xn, "network_embedding.fe2.h1_nei")), "network_embedding.fe2.h2_nei"))
        return F.relu(lin(torch.cat([h1, h2], 1), "network_embedding.emb"))

    def predict(lo, hi):
        with torch.no_grad():
            return F.softmax(lin(embed(X[lo:hi], Xn[lo:hi]), "node_classifier.layer"), dim=1)

    half = int(batch_size / 2)
    num_batch = round(max(ns / (batch_size / 2), nt / (batch_size / 2)))
    np.random.seed(np_seed)
    losses, accs = [], []
    for epoch in range(epochs):
        p = float(epoch) / epochs
        alpha = 2. / (1. + np.exp(-10. * p)) - 1
        idx = epoch_indices(ns, nt, half, num_batch)
        total_epoch = 0.0
        for k in range(num_batch):
            rows, pidx = torch.tensor(idx[k, 0]), idx[k, 1]
            emb = embed(X[rows], Xn[rows])
            logit = lin(emb, "node_classifier.layer")
            er = emb * 1.0
            er.register_hook(lambda g, a=alpha: -a * g)
            d = lin(F.relu(lin(F.relu(lin(er, "domain_discriminator.h_dann_1")), "domain_discriminator.h_dann_2")),
                    "domain_discriminator.output_layer")
            clf = F.cross_entropy(logit[:half], ys[rows[:half]])
            dom = F.cross_entropy(d, torch.cat([torch.zeros(half), torch.ones(half)]).long())
            net = 0.0
            for dom_i, ppmi in enumerate((ps, pt)):
                a = torch.tensor(batch_block(ppmi, pidx[dom_i * half:(dom_i + 1) * half]))
                e = emb[dom_i * half:(dom_i + 1) * half]
                r = torch.sum(e * e, 1).reshape(-1, 1)
                net = net + torch.mean(torch.sum(a * (r - 2 * e @ e.T + r.T), 1))
            total = clf + dom + pair_weight * net
            opt.zero_grad()
            total.backward()
            opt.step()
            total_epoch += total.item()
        losses.append(total_epoch)
        pr = predict(0, ns)
        accs.append(float((pr.argmax(1) == ys).double().mean()))
    out = dict(losses=np.array(losses), accs=np.array(accs), src_prob=predict(0, ns).numpy(),
               tgt_prob=predict(ns, ns + nt).numpy(), ppmi_s=ps, ppmi_t=pt, xnei_s=xns, xnei_t=xnt)
    out.update({"final/" + k: v.detach().numpy() for k, v in P.items()})
    return out
