"""The one convex program PairAlign solves (pygda/models/pa.py: ``LS_optimization`` and ``calc_label_rw``):

    min_x  |A x - m|^2 + lam |x - 1|^2     subject to   mu . x = 1,   x >= 0,     lam > 0.

The objective is strictly convex, so the solution is unique; ``x = 1 / sum(mu)`` is feasible whenever ``mu`` is
non-negative with a positive sum (``x = 1`` for a distribution).  The reference hands the program to cvxpy / SCS, which
stops at about 1e-4 relative accuracy; :func:`solve_simplex_ls` returns the optimum itself, to rounding, by a primal
active-set method in float64 numpy.  Host code on purpose: at most ``PA_MAX_CLASSES ** 2`` variables, once every
``ew_freq`` / ``lw_freq`` epochs."""
import numpy as np


def solve_simplex_ls(A, m, mu, lam, max_iter=None):
    """The minimiser ``x [n]`` (float64) for ``A [r, n]``, ``m [r]``, ``mu [n]`` (non-negative, positive sum) and
    ``lam > 0``.  Each iteration solves the equality-constrained program on the free coordinates (one symmetric
    solve), walks to it or to the first bound on the way, and releases the bound coordinate with the most negative
    multiplier once the walk has arrived.  Raises ``RuntimeError`` after ``max_iter`` (default ``10 n``) iterations
    instead of looping."""
    A = np.asarray(A, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    n = mu.size
    if A.ndim != 2 or A.shape != (m.size, n):
        raise ValueError(f"A [r, n], m [r] and mu [n] expected, got {A.shape}, {m.shape}, {mu.shape}")
    if not lam > 0:
        raise ValueError("lam must be positive: it is what makes the program strictly convex")
    if np.any(mu < 0) or not mu.sum() > 0 or not (np.all(np.isfinite(A)) and np.all(np.isfinite(m))):
        raise ValueError("mu must be non-negative with a positive sum, A and m finite")
    H = 2.0 * (A.T @ A + lam * np.eye(n))
    g = -2.0 * (A.T @ m + lam)
    x = np.full(n, 1.0 / mu.sum())
    free = np.ones(n, dtype=bool)
    scale = max(1.0, float(np.abs(g).max()))
    cap = 10 * n if max_iter is None else int(max_iter)
    for _ in range(cap):
        F = np.flatnonzero(free)
        k = F.size
        KKT = np.zeros((k + 1, k + 1))
        KKT[:k, :k] = H[np.ix_(F, F)]
        KKT[:k, k] = KKT[k, :k] = mu[F]
        sol = np.linalg.solve(KKT, np.concatenate([-g[F], [1.0]]))
        p, nu = sol[:k] - x[F], sol[k]
        if np.abs(p).max() <= 1e-13 * max(1.0, float(np.abs(x).max())):
            x[F] = sol[:k]
            red = H @ x + g + nu * mu                  # the bound multipliers where x is held at 0
            held = np.flatnonzero(~free)
            if held.size == 0 or red[held].min() >= -1e-12 * scale:
                x[~free] = 0.0
                return x
            free[held[np.argmin(red[held])]] = True
            continue
        neg = p < 0
        steps = np.where(neg, -x[F] / np.where(neg, p, -1.0), np.inf)
        j = int(np.argmin(steps))
        if steps[j] < 1.0:
            x[F] = x[F] + steps[j] * p
            x[F[j]] = 0.0
            free[F[j]] = False
        else:
            x[F] = sol[:k]
    raise RuntimeError(f"solve_simplex_ls: no optimum within {cap} iterations (n = {n})")
