"""``torch.optim.Adam``'s update (amsgrad off, maximize off) as include/gda_hip.h documents it for
``gda_adam_multi_f32``, restated in numpy so that the optimiser kernel (pygda_amd/csrc/gda_optim.hip, the rule in
gda_adam_rule.h) has a float64 reference that needs neither a device nor a torch optimiser.  tests/test_optim_host.py
ties :func:`adam_step64` to ``torch.optim.Adam`` in float64 once; the GPU tests (tests/test_gpu_optim.py) compare the
kernel with it inside :func:`adam_tolerances`.

 A1  The kernel receives ``lr, beta1, beta2, eps, weight_decay`` as C floats: the reference rounds them to float32
     first and computes in float64 from there.
 A2  ``t`` is the step counter AFTER its increment (the first update has t = 1).
 A3  ``G = g + wd * p`` (L2 weight decay folded into the gradient; ``G = g`` when ``wd == 0``).
 A4  ``M' = m + (G - m) * (1 - beta1)``            (``exp_avg.lerp_(grad, 1 - beta1)``)
 A5  ``V' = beta2 * v + (1 - beta2) * G * G``      (``exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)``)
 A6  ``bc1 = 1 - beta1 ** t``, ``bc2 = 1 - beta2 ** t``; ``0 ** t = 0`` for t >= 1, so a zero beta has bc = 1.
 A7  ``D = (lr / bc1) * M' / (sqrt(V') / sqrt(bc2) + eps)``, ``P' = p - D``.

Tolerances (:func:`adam_tolerances`), with ``u = 2**-24`` the fp32 unit roundoff, computed from the float64 quantities
only -- never from what the code under test returned:

 T1  ``tol_m = 8u * max(|G|, |m|)``: G carries 2 roundings when wd != 0, the lerp 3 more, each at most u times the
     larger operand.
 T2  ``tol_v = 16u * V'``: both terms of A5 are non-negative, so V' bounds each; G*G doubles G's relative error.
 T3  ``tol_p = (32u + 4u/bc1 + 2u/bc2) * |D| + 2u * max(|p|, |P'|) + (lr/bc1) * tol_m / (sqrt(V')/sqrt(bc2) + eps)``.
     ``1 - powf(beta, t)`` is rounded at the magnitude of 1, an ABSOLUTE error of a few u in bc, i.e. a RELATIVE one of
     a few u / bc (6e-5 in bc2 at t = 2, beta2 = 0.999): 4u/bc1 enters D through lr/bc1, 2u/bc2 through the square root
     (which halves a relative error).  32u covers the remaining roundings of D (sqrt, two divisions, the sum with eps,
     the product) and V's error through the root.  2u * max|p| is the final subtraction.  The third term carries the
     first moment's ABSOLUTE error (which may be large relative to a cancelled M') through the quotient.
 T4  Each tolerance has a floor of one fp32 denormal (2**-149), so that exact zeros and underflowed squares compare.

T1-T3 assume that forming G loses nothing to cancellation (|G| = |g| + wd |p|): wherever ``wd != 0`` the tests that
use these bounds draw ``g`` with the sign of ``p``.  Random signs are the business of the trajectory test in
tests/test_gpu_parity.py, at its own tolerance.

:func:`adam_step32_emulated` performs A3-A7 in numpy float32 in the kernel's order of operations; the host test uses
it to show that the bounds hold, with a factor of two to spare, for a correct fp32 implementation.
"""
import numpy as np

U = 2.0 ** -24
DENORM = 2.0 ** -149


def _f32_hyper(lr, b1, b2, eps, wd):
    return [float(np.float32(x)) for x in (lr, b1, b2, eps, wd)]                      # A1


def adam_step64(p, g, m, v, t, lr, b1, b2, eps, wd):
    """One update in float64.  ``p, g, m, v``: arrays (any float dtype, converted); ``t``: the counter after the
    increment, a number or an array broadcastable against ``p``.  Returns a dict with the new ``p``, ``m``, ``v`` and
    the intermediates ``G``, ``D``, ``bc1``, ``bc2`` (and the rounded ``lr``, ``eps`` the tolerances use)."""
    lr, b1, b2, eps, wd = _f32_hyper(lr, b1, b2, eps, wd)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    t = np.asarray(t, dtype=np.float64)
    assert np.all(t >= 1)
    G = g + wd * p if wd != 0 else g.copy()                                           # A3
    M = m + (G - m) * (1.0 - b1)                                                      # A4
    V = b2 * v + (1.0 - b2) * G * G                                                   # A5
    bc1 = 1.0 - np.power(b1, t)                                                       # A6
    bc2 = 1.0 - np.power(b2, t)
    D = (lr / bc1) * M / (np.sqrt(V) / np.sqrt(bc2) + eps)                            # A7
    return dict(p=p - D, m=M, v=V, G=G, D=D, bc1=bc1, bc2=bc2, p0=p, m0=m, lr=lr, eps=eps)


def adam_tolerances(ref):
    """``(tol_p, tol_m, tol_v)`` (T1-T4) for the result ``ref`` of :func:`adam_step64`."""
    G, D, bc1, bc2, V = ref["G"], ref["D"], ref["bc1"], ref["bc2"], ref["v"]
    tol_m = 8 * U * np.maximum(np.abs(G), np.abs(ref["m0"]))
    tol_v = 16 * U * V
    denom = np.sqrt(V) / np.sqrt(bc2) + ref["eps"]
    with np.errstate(divide="ignore", invalid="ignore"):
        carried = np.where(tol_m > 0, (ref["lr"] / bc1) * tol_m / denom, 0.0)         # 0 / 0 (eps = 0, V' = 0): nothing to carry
    tol_p = ((32 * U + 4 * U / bc1 + 2 * U / bc2) * np.abs(D) + 2 * U * np.maximum(np.abs(ref["p0"]), np.abs(ref["p"]))
             + carried)
    return tuple(np.maximum(x, DENORM) for x in (tol_p, tol_m, tol_v))


def adam_step32_emulated(p, g, m, v, t, lr, b1, b2, eps, wd):
    """The same update with every operation rounded to float32, in the order of gda_adam_rule.h.  Returns
    ``(p, m, v)`` as float32 arrays."""
    f = np.float32
    lr, b1, b2, eps, wd = (f(x) for x in (lr, b1, b2, eps, wd))
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    one = f(1.0)
    with np.errstate(under="ignore"):
        bc1 = one - np.power(b1, f(t), dtype=f)
        bc2 = one - np.power(b2, f(t), dtype=f)
        step_size, bc2_sqrt = lr / bc1, np.sqrt(bc2)
        G = g + wd * p if wd != 0 else g
        M = m + (G - m) * (one - b1)
        V = v * b2 + (one - b2) * G * G
        denom = np.sqrt(V) / bc2_sqrt + eps
        P = p - step_size * (M / denom)
    assert P.dtype == f and M.dtype == f and V.dtype == f
    return P, M, V


def draw_case(rng, n, t, scale, wd):
    """Inputs of one comparison: ``p ~ N(0, 1)``; ``g ~ scale * N(0, 1)``, with the sign of ``p`` when ``wd != 0``
    (see the module docstring); for ``t > 1`` moments ``m ~ 0.3 * scale * N(0, 1)``, ``v ~ scale^2 * U(0, 1)``, zero at
    the first step.  float32 arrays."""
    p = rng.standard_normal(n).astype(np.float32)
    g = (scale * rng.standard_normal(n)).astype(np.float32)
    if wd != 0:
        g = np.copysign(g, p)
    if t > 1:
        m = (0.3 * scale * rng.standard_normal(n)).astype(np.float32)
        v = (scale * scale * rng.random(n)).astype(np.float32)
    else:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    return p, g, m, v


# the grid of the single-step comparisons, shared by the host and the device test
GRID_T = (1, 2, 3, 10, 1000, 100000)
GRID_LR = (1e-3, 0.05)
GRID_BETAS = ((0.9, 0.999), (0.5, 0.9), (0.0, 0.999), (0.9, 0.0))
GRID_EPS = (1e-8, 1e-3)
GRID_WD = (0.0, 0.005)
GRID_SCALE = (1.0, 1e-4, 1e3)
GRID_N = 4099


def grid():
    return [(t, lr, betas, eps, wd, scale) for t in GRID_T for lr in GRID_LR for betas in GRID_BETAS
            for eps in GRID_EPS for wd in GRID_WD for scale in GRID_SCALE]
