"""GPU: ``pygda_amd.optim.Adam`` (one ``gda_adam_multi_sum_f32`` launch per table of up to 48 tensors,
pygda_amd/csrc/gda_optim.hip; the per-element rule in gda_adam_rule.h) against the float64 restatement of the update in
tests/golden/_adam_semantics.py, inside the tolerances derived there (fp32 roundings of the rule, worked out from the
float64 quantities; tests/test_optim_host.py ties the restatement to ``torch.optim.Adam`` and shows that a correct fp32
implementation uses at most half of each bound).

Every comparison covers every element of the parameter and of both moments.  Parameters, gradients and moments are
views at ODD element offsets (4-byte, not 16-byte aligned) into flat buffers whose gaps hold a sentinel: a write past a
tensor's end, or a work item routed to the neighbouring tensor, changes a gap or an element that is compared.  State is
preset through ``opt.state[p]`` (``Adam._state`` returns an existing entry): a float32 device scalar ``step`` holding
t - 1 and moment views into the flat buffers.

Measured on an MI355X over the grid and a 97-tensor table, worst |device - float64| / tolerance: 0.497 for the
parameter, 0.401 for exp_avg, 0.331 for exp_avg_sq -- the figures of the fp32 emulation on the host.

Known and not asserted either way: a zero-element tensor is skipped by the launch, so its step counter is not
incremented; torch would increment it.
"""
import copy
import zlib

import numpy as np
import pytest
import torch

from pygda_amd.optim import MAX_TENSORS, Adam
from tests.golden import _adam_semantics as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
SENTINEL = np.float32(-123456.789)
SENTINEL_BITS = int(np.array([SENTINEL]).view(np.int32)[0])
SIZES = (1, 3, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6144, 10000)
HYPER = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.005)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def exact(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


def within(got, ref, tol, what):
    """Every element: NaN exactly where the reference is NaN, |got - ref| <= tol everywhere else."""
    got = got.astype(np.float64)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN pattern")
    err = np.where(nan, 0.0, np.abs(got - np.where(nan, 0.0, ref)))
    bad = ~(err <= np.where(nan, 1.0, tol))
    if bad.any():
        i = int(np.argmax(np.where(bad, err / tol, 0)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the tolerance; worst at {i}: "
                             f"got {got.flat[i]!r}, want {ref.flat[i]!r}, |err| {err.flat[i]:.3e} > tol {tol.flat[i]:.3e}")


class Flat:
    """1-D arrays laid into one device buffer: at least GUARD sentinel elements before, between and after them, every
    array at an odd element offset."""

    def __init__(self, arrays):
        self.spans, cursor = [], 0
        for a in arrays:
            cursor += GUARD
            cursor += 1 - cursor % 2
            self.spans.append((cursor, cursor + a.size))
            cursor += a.size
        host = np.full(cursor + GUARD, SENTINEL, np.float32)
        self.gap = np.ones(host.size, bool)
        for (lo, hi), a in zip(self.spans, arrays):
            host[lo:hi] = a.reshape(-1)
            self.gap[lo:hi] = False
        self.dev = torch.from_numpy(host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.views = [self.dev[lo:hi] for lo, hi in self.spans]
        assert all(v.data_ptr() % 8 == 4 for v in self.views if v.numel())

    def host(self, k=None):
        h = self.dev.cpu().numpy()
        return h if k is None else h[self.spans[k][0]:self.spans[k][1]]

    def assert_guards_intact(self, what):
        hit = np.flatnonzero(self.gap & (bits(self.host()) != SENTINEL_BITS))
        assert hit.size == 0, f"{what}: {hit.size} guard elements were overwritten, the first at flat index {hit[:8]}"


def draw(rng, n, t, scale=1.0, wd=HYPER["weight_decay"], hyper=None):
    p, g, m, v = A.draw_case(rng, n, t, scale, wd)
    return dict(p=p, g=g, m=m, v=v, t=t, hyper=hyper or HYPER)


class Table:
    """The tensors of ``cases`` (dicts of float32 arrays ``p, g, m, v``, the counter ``t`` AFTER the step and the
    ``hyper`` of their param group) in four guarded flat buffers, as Parameters with gradients."""

    def __init__(self, cases, preset=True):
        self.cases = cases
        self.P, self.G, self.M, self.V = (Flat([c[key] for c in cases]) for key in "pgmv")
        self.params = [torch.nn.Parameter(v) for v in self.P.views]
        for p, v, g in zip(self.params, self.P.views, self.G.views):
            assert p.data_ptr() == v.data_ptr()
            p.grad = g
        self.preset = preset

    def optimiser(self, params=None):
        groups, last = [], None
        for p, c in zip(self.params, self.cases):
            if c["hyper"] is not last:
                groups.append(dict(params=[], **c["hyper"]))
                last = c["hyper"]
            groups[-1]["params"].append(p)
        opt = Adam(groups if params is None else params, **({} if params is None else self.cases[0]["hyper"]))
        if self.preset:
            for p, c, m, v in zip(self.params, self.cases, self.M.views, self.V.views):
                opt.state[p] = {"step": torch.tensor(float(c["t"] - 1), dtype=torch.float32, device=DEV),
                                "exp_avg": m, "exp_avg_sq": v}
        self.opt = opt
        return opt

    def set_grads(self, grads):
        for view, g in zip(self.G.views, grads):
            view.copy_(torch.from_numpy(g))

    def assert_guards_intact(self):
        for name, flat in (("parameter", self.P), ("gradient", self.G), ("exp_avg", self.M), ("exp_avg_sq", self.V)):
            flat.assert_guards_intact(name)

    def snapshot(self):
        """The device's p, m, v and counters now, as cases for the NEXT step (gradients to be filled in)."""
        return [dict(p=self.P.host(k).copy(), m=self.M.host(k).copy(), v=self.V.host(k).copy(),
                     t=int(float(self.opt.state[p]["step"])) + 1, hyper=c["hyper"])
                for k, (p, c) in enumerate(zip(self.params, self.cases))]

    def check(self, cases=None, steps=1):
        """Every tensor against ``steps`` successive float64 updates of ``cases`` (the inputs this table was built
        from by default) with the same gradient, tolerances summed; counters exact; guards intact."""
        for k, c in enumerate(self.cases if cases is None else cases):
            if c["p"].size == 0:
                continue                                       # its counter: see the module docstring
            h = c["hyper"]
            p, m, v = c["p"], c["m"], c["v"]
            tol = [0.0, 0.0, 0.0]
            for s in range(steps):
                ref = A.adam_step64(p, c["g"], m, v, c["t"] + s, h["lr"], h["betas"][0], h["betas"][1], h["eps"],
                                    h["weight_decay"])
                tol = [a + b for a, b in zip(tol, A.adam_tolerances(ref))]
                p, m, v = ref["p"], ref["m"], ref["v"]
            what = f"tensor {k} (numel {c['p'].size}, t {c['t']})"
            within(self.P.host(k), p, tol[0], what + " parameter")
            within(self.M.host(k), m, tol[1], what + " exp_avg")
            within(self.V.host(k), v, tol[2], what + " exp_avg_sq")
            step = self.opt.state[self.params[k]]["step"]
            assert step.dtype == torch.float32 and step.is_cuda and step.dim() == 0
            assert float(step) == c["t"] + steps - 1, what
        self.assert_guards_intact()

    def assert_same_bits(self, other):
        for a, b in ((self.P, other.P), (self.M, other.M), (self.V, other.V)):
            exact(a.dev, b.dev)
        for p, q in zip(self.params, other.params):
            if p.numel():
                exact(self.opt.state[p]["step"], other.opt.state[q]["step"])


def table_cases(n, seed, empties=()):
    """``n`` non-empty tensors, numel cycling through SIZES, tensor k at step t_k = 1 + 37 k; zero-element tensors
    inserted before the positions in ``empties``."""
    rng = np.random.default_rng(seed)
    cases = [draw(rng, SIZES[k % len(SIZES)], 1 + 37 * k) for k in range(n)]
    for at in sorted(empties, reverse=True):
        cases.insert(at, draw(rng, 0, 1))
    return cases


# ---------------------------------------------------------------- one step, the grid --
@pytest.mark.parametrize("t", A.GRID_T)
@pytest.mark.parametrize("betas", A.GRID_BETAS, ids=lambda b: f"b{b[0]}-{b[1]}")
def test_single_step_vs_float64_over_the_grid(t, betas):
    """The grid of tests/test_optim_host.py (every lr, eps, weight decay and gradient scale at this t and these
    betas): one 4099-element tensor at counter t - 1, one step; parameter and both moments inside the tolerances, the
    counter exactly t."""
    for case in A.grid():
        if case[0] != t or case[2] != betas:
            continue
        _, lr, _, eps, wd, scale = case
        rng = np.random.default_rng(zlib.crc32(repr(case).encode()) + 1)
        hyper = dict(lr=lr, betas=betas, eps=eps, weight_decay=wd)
        tab = Table([draw(rng, A.GRID_N, t, scale, wd, hyper)])
        tab.optimiser().step()
        tab.check()


# ------------------------------------------------------------------------- the table --
@pytest.mark.parametrize("n,empties", [(MAX_TENSORS, ()), (MAX_TENSORS, (0, 24, 48)), (MAX_TENSORS - 3, (0, 24, 45)),
                                       (50, ()), (97, ())],
                         ids=["48", "48+3empty", "45+3empty", "50", "97"])
def test_table_of_unaligned_tensors_at_their_own_step_counts(n, empties):
    """A full table (and 50 / 97 tensors: two / three launches; zero-element tensors at the front, in the middle and
    at the end, which the launch skips): every numel around the 256-thread and 2048-element item boundaries, every
    tensor at its own step count."""
    tab = Table(table_cases(n, 100 + n + len(empties), empties))
    opt = tab.optimiser()
    if len(tab.cases) > MAX_TENSORS:
        assert opt.bump_steps() is False                       # more than one launch takes: step() increments itself
    opt.step()
    tab.check()


def test_table_with_second_gradient_leaves_equals_the_presummed_gradient():
    """Every third tensor of the full table receives its gradient as two contributions (``grad_aliases``): bit-identical
    to the same table given their fp32 sum, which is within tolerance of float64."""
    cases = table_cases(MAX_TENSORS, 7)
    rng = np.random.default_rng(8)
    first, second = [], []
    for k, c in enumerate(cases):
        share = rng.random(c["g"].size).astype(np.float32)
        g1 = c["g"] * share if k % 3 == 0 else c["g"]
        g2 = c["g"] - g1                                       # the sign of g, so of p, in both parts
        c["g"] = g1 + g2 if k % 3 == 0 else g1                 # what autograd's accumulation would have stored
        first.append(g1)
        second.append(g2)
    summed, split = Table(cases), Table(cases)
    summed.optimiser().step()
    summed.check()
    opt = split.optimiser()
    split.set_grads(first)
    G2 = Flat(second)
    leaves = []
    for k, p in enumerate(split.params):
        if k % 3 == 0:
            leaf = torch.nn.Parameter(p.detach())
            assert leaf.data_ptr() == p.data_ptr()
            leaf.grad = G2.views[k]
            opt.grad_aliases[id(p)] = leaf
            leaves.append(leaf)
    opt.step()
    split.assert_same_bits(summed)
    split.assert_guards_intact()
    G2.assert_guards_intact("second gradient")


# ------------------------------------------------------------------- the bumped path --
def test_bumped_steps_equal_plain_steps_and_float64_over_three_steps():
    """``bump_steps(counter)`` + ``step()`` against plain ``step()`` on the full table: bit-identical after each of
    three steps, and within tolerance of float64 at each step -- the reference of a step starts from the device state
    before it, so no error compounds into the tolerance."""
    cases = table_cases(MAX_TENSORS, 21)
    bumped, plain = Table(cases), Table(cases)
    ob, op = bumped.optimiser(), plain.optimiser()
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    rng = np.random.default_rng(22)
    for step in range(3):
        before = bumped.snapshot()
        for c in before:
            c["g"] = np.copysign(rng.standard_normal(c["p"].size).astype(np.float32), c["p"])
        assert [c["t"] for c in before] == [c["t"] + step for c in cases]
        for tab in (bumped, plain):
            tab.set_grads([c["g"] for c in before])
        assert ob.bump_steps(counter) is True
        ob.step()
        op.step()
        bumped.assert_same_bits(plain)
        bumped.check(before)
        plain.assert_guards_intact()
    assert int(counter) == 3


# --------------------------------------------------------------------------- layouts --
def _check_2d(p, opt, before, g, t):
    ref = A.adam_step64(before[0], g, before[1], before[2], t, HYPER["lr"], *HYPER["betas"], HYPER["eps"],
                        HYPER["weight_decay"])
    tol = A.adam_tolerances(ref)
    st = opt.state[p]
    assert st["exp_avg"].stride() == p.stride() and st["exp_avg_sq"].stride() == p.stride()
    within(p.detach().cpu().numpy(), ref["p"], tol[0], f"parameter, step {t}")
    within(st["exp_avg"].cpu().numpy(), ref["m"], tol[1], f"exp_avg, step {t}")
    within(st["exp_avg_sq"].cpu().numpy(), ref["v"], tol[2], f"exp_avg_sq, step {t}")
    assert float(st["step"]) == t
    return [p.detach().cpu().numpy().copy(), st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy()]


@pytest.mark.parametrize("relayout", [False, True], ids=["stored-transposed", "re-laid-out-after-a-step"])
def test_column_major_parameter_follows_float64_element_for_element(relayout):
    """A [40, 24] parameter stored transposed takes row-major gradients; with ``relayout`` it is row-major for the
    first step -- so its state is created row-major -- and is assigned a transposed-stride tensor of the same values
    before the second, which re-lays the state out.  Both steps follow float64 element for element."""
    rng = np.random.default_rng(31 + relayout)
    p0 = rng.standard_normal((40, 24)).astype(np.float32)
    if relayout:
        p = torch.nn.Parameter(torch.from_numpy(p0).to(DEV))
    else:
        p = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(p0.T)).to(DEV).t())
        assert p.shape == (40, 24) and not p.is_contiguous() and p.t().is_contiguous()
    opt = Adam([p], **HYPER)
    state = [p0.copy(), np.zeros_like(p0), np.zeros_like(p0)]
    for t in (1, 2):
        if relayout and t == 2:
            p.data = p.data.t().contiguous().t()
            assert not p.is_contiguous() and p.t().is_contiguous()
            exact(p, state[0])
        g = np.copysign(rng.standard_normal((40, 24)).astype(np.float32), state[0])
        p.grad = torch.from_numpy(g).to(DEV)
        assert p.grad.is_contiguous()
        opt.step()
        state = _check_2d(p, opt, state, g, t)


# --------------------------------------------------------- param groups, duplicates --
def test_two_param_groups_follow_their_own_hyper_parameters():
    other = dict(lr=0.002, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.0)
    rng = np.random.default_rng(41)
    cases = [draw(rng, 257, 4), draw(rng, 2049, 90), draw(rng, 2049, 2, wd=0.0, hyper=other),
             draw(rng, 4097, 33, wd=0.0, hyper=other)]
    tab = Table(cases)
    opt = tab.optimiser()
    assert len(opt.param_groups) == 2 and [len(g["params"]) for g in opt.param_groups] == [2, 2]
    opt.step()
    tab.check()


def test_parameter_listed_twice_takes_two_successive_updates():
    """UDAGCN hands the optimiser its shared weights twice: one ``step()`` applies two updates with the same gradient,
    one after the other, and advances the counter by 2.  Tolerance: the sum of the two steps' tolerances."""
    rng = np.random.default_rng(51)
    tab = Table([draw(rng, 2049, 5), draw(rng, 257, 1)])
    opt = tab.optimiser(params=[tab.params[0], tab.params[1], tab.params[0], tab.params[1]])
    assert opt.bump_steps() is False
    opt.step()
    tab.check(steps=2)


# ------------------------------------------------------------------- save and resume --
def test_state_dict_round_trip_resumes_bit_for_bit():
    """Three steps, a copy of ``state_dict()`` loaded into a fresh optimiser over cloned parameters, three more steps
    on both: parameters, moments and counters bit-identical; the resumed counters are float32 device scalars (what
    the kernel dereferences)."""
    rng = np.random.default_rng(61)
    sizes = (1, 257, 2048, 2049, 4097)
    tab = Table([draw(rng, n, 1) for n in sizes], preset=False)          # state is created by the first step
    opt = tab.optimiser()

    def grads():
        return [rng.standard_normal(n).astype(np.float32) for n in sizes]

    for _ in range(3):
        tab.set_grads(grads())
        opt.step()
    clones = [torch.nn.Parameter(p.detach().clone()) for p in tab.params]
    resumed = Adam(clones, **HYPER)
    resumed.load_state_dict(copy.deepcopy(opt.state_dict()))    # state_dict() hands out references to the live state
    for p, q in zip(tab.params, clones):
        step = resumed.state[q]["step"]
        assert step.dtype == torch.float32 and step.is_cuda and step.dim() == 0 and float(step) == 3.0
        assert resumed.state[q]["exp_avg"].data_ptr() != opt.state[p]["exp_avg"].data_ptr()
    for _ in range(3):
        gs = grads()
        tab.set_grads(gs)
        for q, g in zip(clones, gs):
            q.grad = torch.from_numpy(g).to(DEV)
        opt.step()
        resumed.step()
    for p, q in zip(tab.params, clones):
        exact(p, q)
        for key in ("step", "exp_avg", "exp_avg_sq"):
            exact(opt.state[p][key], resumed.state[q][key])
        assert float(resumed.state[q]["step"]) == 6.0
    tab.assert_guards_intact()


# ------------------------------------------------- non-finite and degenerate elements --
def test_nan_gradient_elements_stay_where_they_are():
    """NaN gradients at 2047 and 2048 -- the last element of one work item and the only element of the next: NaN at
    exactly those indices of p, m and v (``within`` compares the NaN pattern), every other element inside tolerance."""
    rng = np.random.default_rng(71)
    case = draw(rng, 2049, 12)
    case["g"][2047] = case["g"][2048] = np.nan
    tab = Table([case, draw(rng, 2049, 12)])
    tab.optimiser().step()
    tab.check()
    for flat in (tab.P, tab.M, tab.V):
        assert np.flatnonzero(np.isnan(flat.host(0))).tolist() == [2047, 2048]
        assert not np.isnan(flat.host(1)).any()


def test_zero_gradient_on_zero_moments_leaves_the_parameter_alone():
    rng = np.random.default_rng(81)
    hyper = dict(HYPER, weight_decay=0.0)
    cases = []
    for t in (1, 50):
        c = draw(rng, 2049, 1, wd=0.0, hyper=hyper)             # t = 1: zero moments
        c["g"][:] = 0
        c["t"] = t
        cases.append(c)
    tab = Table(cases)
    tab.optimiser().step()
    tab.check()
    for k, c in enumerate(cases):
        exact(tab.P.host(k), c["p"])
        exact(tab.M.host(k), np.zeros(2049, np.float32))
        exact(tab.V.host(k), np.zeros(2049, np.float32))


def test_gradients_whose_square_underflows():
    """g = +-1e-25: g * g underflows in fp32, so exp_avg_sq stays 0 (within the denormal floor of its tolerance) and
    the step is m / eps.  From zero state on a zero parameter, where the update is the whole result, and from a small
    first moment on an ordinary parameter."""
    rng = np.random.default_rng(91)
    hyper = dict(HYPER, weight_decay=0.0)
    fresh = draw(rng, 2049, 1, wd=0.0, hyper=hyper)
    fresh["g"] = np.copysign(np.float32(1e-25), fresh["g"])
    fresh["p"][:] = 0
    later = draw(rng, 2049, 3, wd=0.0, hyper=hyper)
    later["g"] = np.copysign(np.float32(1e-25), later["g"])
    later["m"] = (later["m"] * np.float32(1e-25)).astype(np.float32)
    later["v"][:] = 0
    tab = Table([fresh, later])
    tab.optimiser().step()
    tab.check()
    assert np.all(tab.P.host(0) != 0)                           # the tiny update arrived
