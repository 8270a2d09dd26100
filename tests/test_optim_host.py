"""CPU: the float64 restatement of the Adam update (tests/golden/_adam_semantics.py) against ``torch.optim.Adam``, and
the tolerances the device tests use against a float32 emulation of the kernel's rule.

Measured worst ratios |emulation - float64| / tolerance over the whole grid (1152 cases of 4099 elements, seeded per
case as below): 0.408 for ``exp_avg`` (t = 3, betas (0, 0.999), weight decay 0.005, gradient scale 1e-4), 0.338 for
``exp_avg_sq`` (t = 100000, weight decay 0.005, scale 1e-4) and 0.497 for the parameter (t = 100000, betas
(0, 0.999), eps 1e-3, scale 1e-4: the update is far below the parameter's ulp there, and the half ulp of the final
subtraction against its 2u bound is the whole ratio) -- ``test_fp32_emulation_stays_within_half_of_every_tolerance``
prints them.
"""
import zlib

import numpy as np
import pytest
import torch

from tests.golden import _adam_semantics as A


@pytest.mark.parametrize("t", [1, 7, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.005])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
def test_adam_step64_is_torch_adam_in_float64(t, wd, betas):
    """One ``torch.optim.Adam`` step in float64 on the CPU from a preset state (counter t - 1, nonzero moments) gives
    the parameter and both moments of ``adam_step64`` to 1e-14 relative.  Hyper-parameters are the float32-rounded
    values (A1), handed to torch as Python floats."""
    rng = np.random.default_rng(1000 * t + int(wd * 1e4) + int(betas[0] * 10))
    n = 513
    p, g, m, v = A.draw_case(rng, n, 2, 1.0, wd)                  # nonzero moments at every t: state is preset anyway
    # a RELATIVE bound needs results that are not cancelled: the first moment has the sign of the gradient here, so
    # lerp(m, G) lies between two numbers of one sign (torch evaluates the lerp in a slightly different form)
    m = np.copysign(m, g)
    lr, eps = 0.01, 1e-8
    lr32, b1, b2, eps32, wd32 = A._f32_hyper(lr, betas[0], betas[1], eps, wd)
    param = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    param.grad = torch.from_numpy(g.astype(np.float64))
    opt = torch.optim.Adam([param], lr=lr32, betas=(b1, b2), eps=eps32, weight_decay=wd32)
    opt.state[param] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.astype(np.float64)),
                        "exp_avg_sq": torch.from_numpy(v.astype(np.float64))}
    opt.step()
    ref = A.adam_step64(p, g, m, v, t, lr, betas[0], betas[1], eps, wd)
    assert float(opt.state[param]["step"]) == t
    np.testing.assert_allclose(opt.state[param]["exp_avg"].numpy(), ref["m"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(opt.state[param]["exp_avg_sq"].numpy(), ref["v"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(param.detach().numpy(), ref["p"], rtol=1e-14, atol=0)


def test_fp32_emulation_stays_within_half_of_every_tolerance():
    """The reference rounded to fp32 -- the rule in the kernel's order of operations, numpy float32 -- stays within HALF
    of ``adam_tolerances`` at every element of every grid case; the other half is the device's ``powf``, ``sqrtf`` and
    division differing from numpy's by an ulp.  Measured worst ratios: 0.408 (exp_avg), 0.338 (exp_avg_sq), 0.497
    (parameter); the cases are named in the module docstring."""
    worst = {"p": (0.0, None), "m": (0.0, None), "v": (0.0, None)}
    for case in A.grid():
        t, lr, (b1, b2), eps, wd, scale = case
        rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
        p, g, m, v = A.draw_case(rng, A.GRID_N, t, scale, wd)
        ref = A.adam_step64(p, g, m, v, t, lr, b1, b2, eps, wd)
        tol = dict(zip("pmv", A.adam_tolerances(ref)))
        got = dict(zip("pmv", A.adam_step32_emulated(p, g, m, v, t, lr, b1, b2, eps, wd)))
        for key in "pmv":
            assert np.all(np.isfinite(got[key]))
            ratio = float(np.max(np.abs(got[key].astype(np.float64) - ref[key]) / tol[key]))
            if ratio > worst[key][0]:
                worst[key] = (ratio, case)
    print("worst emulation / tolerance ratios:", worst)
    for key in "pmv":
        assert worst[key][0] <= 0.5, (key, worst[key])


def test_tolerances_have_a_denormal_floor_and_nothing_else_at_zero():
    """All-zero inputs: every tolerance is exactly one fp32 denormal, so a kernel that leaves zeros alone compares and
    one that writes anything else does not."""
    z = np.zeros(5, np.float32)
    ref = A.adam_step64(z, z, z, z, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    for key in "pmv":
        assert np.all(ref[key] == 0)
    for tol in A.adam_tolerances(ref):
        assert np.all(tol == A.DENORM)
