"""GPU tests of the s-domain plans: the planner stand-in against its numpy restatement (tests/plan_numpy.py), the
isolation of per-instance plans, the time resampling against the oracle's obtain_reference (bit for bit), the fused pre kernel of
the closed loop, and the loop tracking a plan.  No test here feeds a kernel a table with zero, negative or non-finite times: the
bounded walk is exercised on the host (tests/test_plan_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
from conftest import relerr

import plan_numpy as pn

pytestmark = pytest.mark.gpu

BUILD_TOL = 1e-9      # the project's construction tolerance; test_plan_cpu.py::test_profile_conditioning: a 1e-13 input difference stays below 1e-11
DT = 0.05
_NP = {}


@pytest.fixture(scope="module")
def fm():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import fsae_mpc_amd
    return fsae_mpc_amd


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tracks(fm, orc, name):
    return fm.Track.load(name), orc.Track.load(fm.tracks._HERE + "/tracks/%s.json" % name)


def _kappa(orc, otr, N_s):
    key = (otr.name, otr.L, N_s)
    if key not in _NP:
        k = pn.kappa_cells(orc, otr, N_s); k.setflags(write=False)
        _NP[key] = k
    return _NP[key]


def _host(plan):
    return plan.table.cpu().numpy(), plan.t.cpu().numpy()


def _check_plan(tab, t, ref, v_cap, what):
    for c in range(8):
        assert relerr(tab[:, c], ref["table"][:, c]) <= BUILD_TOL, (what, "column", c, relerr(tab[:, c], ref["table"][:, c]))
    assert relerr(t, ref["t"]) <= BUILD_TOL, (what, "t")
    v = tab[:, 2]
    # the speed limits on the device's own numbers: the cap exactly.  vlat is not an output of the entry (its signature is the issue's:
    # table and t only), so v <= vlat is exact only where vlat is known without the device's curvature (the v_cap = 3 set below);
    # elsewhere it is checked against numpy's vlat at the parity tolerance
    assert (v <= v_cap).all() and (v <= ref["vlat"] * (1 + BUILD_TOL)).all(), what
    assert np.array_equal(t, ref["ds"] / v) and np.array_equal(tab[:, [0, 1, 3]], np.zeros((len(t), 3))), what


@pytest.mark.parametrize("name", ["fsg2019", "fss2019"])
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("N_s", [37, 97, 500])
def test_profile_parity(fm, torch_, orc, name, model, N_s):
    """Below one wave, not a multiple of 64, and the reference's own cell count; defaults, per-instance blocks, and the all-ties argmin."""
    tr, otr = _tracks(fm, orc, name)
    k = _kappa(orc, otr, N_s)
    plan = fm.Plan.profile(model, tr, N_s=N_s, v_cap=20.0, grip=1.0)
    assert plan.P == 1 and plan.N_s == N_s and plan.ds == otr.L / N_s
    tab, t = _host(plan)
    ref = pn.profile(model, k, otr.L, 20.0, 1.0)
    _check_plan(tab[0], t[0], ref, 20.0, "defaults")
    assert abs(plan.lap_time()[0] - ref["t"].sum()) <= BUILD_TOL * ref["t"].sum()
    blocks = fm.param_draws(model, range(5), 77, 0.2)
    plans = fm.Plan.profile(model, tr, N_s=N_s, v_cap=20.0, grip=0.8, params=blocks)
    assert plans.P == 5 and plans.c.per_instance == 1
    tab, t = _host(plans)
    for j in range(5):
        _check_plan(tab[j], t[j], pn.profile(model, k, otr.L, 20.0, 0.8, par=blocks[j]), 20.0, "block %d" % j)
    flat = fm.Plan.profile(model, tr, N_s=N_s, v_cap=3.0)
    tab, t = _host(flat)
    _check_plan(tab[0], t[0], pn.profile(model, k, otr.L, 3.0, 1.0), 3.0, "v_cap = 3")
    assert (tab[0][:, 2] == 3.0).all() and (tab[0][:, 6] == 0.0).all()     # v <= vlat = v_cap exactly, on the device's own numbers


@pytest.mark.parametrize("model", [0, 1])
def test_profile_parity_at_the_cell_cap(fm, torch_, orc, model):
    """N_s = FSAEMPC_PLAN_MAX_NS: the 64 KB of LDS the cap exists for, 64 cells per lane."""
    tr, otr = _tracks(fm, orc, "fss2019")
    N_s = fm._lib.PLAN_MAX_NS
    k = _kappa(orc, otr, N_s)
    blocks = fm.param_draws(model, range(2), 81, 0.2)
    tab, t = _host(fm.Plan.profile(model, tr, N_s=N_s))
    _check_plan(tab[0], t[0], pn.profile(model, k, otr.L, 20.0, 1.0), 20.0, "defaults")
    tab, t = _host(fm.Plan.profile(model, tr, N_s=N_s, grip=0.8, params=blocks))
    for j in range(2):
        _check_plan(tab[j], t[j], pn.profile(model, k, otr.L, 20.0, 0.8, par=blocks[j]), 20.0, "block %d" % j)


@pytest.mark.parametrize("model", [0, 1])
def test_per_instance_plans_are_isolated(fm, torch_, model):
    tr = fm.Track.load("fss2019")
    blocks = fm.param_draws(model, range(5), 78, 0.2)
    tab, t = _host(fm.Plan.profile(model, tr, N_s=97, grip=0.8, params=blocks))
    for j in range(5):
        tj, ttj = _host(fm.Plan.profile(model, tr, N_s=97, grip=0.8, params=blocks[j]))
        assert np.array_equal(tab[j], tj[0]) and np.array_equal(t[j], ttj[0]), j
    bad = blocks.copy(); bad[2, fm.PARAM_INDEX["M"]] = -1.0
    tab2, t2 = _host(fm.Plan.profile(model, tr, N_s=97, grip=0.8, params=bad))
    assert np.isnan(tab2[2]).all() and np.isnan(t2[2]).all()
    for j in (0, 1, 3, 4):
        assert np.array_equal(tab2[j], tab[j]) and np.array_equal(t2[j], t[j]), j


def _check_reference(orc, model, got, tab, t, ds, s0, N):
    """got: (N, nx) of the device; against the oracle's walk on the same table"""
    r7 = orc.obtain_reference(tab.reshape(-1), ds, t.size, t, s0, DT, N)
    if model == 1:
        assert np.array_equal(got.T, r7), s0
    else:
        want = pn.model_layout(0, r7)
        assert np.array_equal(got.T[[0, 1, 2, 4]], want[[0, 1, 2, 4]]), s0
        assert (np.abs(got.T[3] - want[3]) <= 4 * np.spacing(want[3])).all(), s0


@pytest.mark.parametrize("model", [0, 1])
def test_reference_parity(fm, torch_, orc, model):
    tr = fm.Track.load("fss2019")
    N = 40
    plan = fm.Plan.profile(model, tr, N_s=97)
    tab, t = _host(plan)
    rng = np.random.default_rng(12)
    s0 = np.concatenate([[0.0, tr.L, 5 * plan.ds, 1234.5], rng.uniform(0, 3 * tr.L, 252)])
    got = plan.reference(model, s0, N, DT)
    assert tuple(got.shape) == (256, N, (5, 7)[model])
    got = got.cpu().numpy()
    for b in range(256):
        _check_reference(orc, model, got[b], tab[0], t[0], plan.ds, s0[b], N)
    # one plan per car
    plans = fm.Plan.profile(model, tr, N_s=37, grip=0.8, params=fm.param_draws(model, range(8), 79, 0.2))
    tab, t = _host(plans)
    s0 = rng.uniform(0, 2 * tr.L, 8)
    got = plans.reference(model, _dev(torch_, s0), N, DT).cpu().numpy()
    for b in range(8):
        _check_reference(orc, model, got[b], tab[b], t[b], plans.ds, s0[b], N)
    with pytest.raises(ValueError):
        plans.reference(model, s0[:5], N, DT)
    # a user's own table goes the same way
    own = fm.Plan.from_table(tab[3], t[3], plans.ds)
    assert np.array_equal(own.reference(model, s0[3:4], N, DT).cpu().numpy()[0], got[3])


def _random_carts(orc, otr, B, seed):
    rng = np.random.default_rng(seed)
    L = orc.lib(); L.orc_spline_d.restype = C.c_double
    carts, guesses = [], []
    for _ in range(B):
        s, n = rng.uniform(0, otr.L * 0.9), rng.uniform(-0.5, 0.5)
        xd = L.orc_spline_d(otr.c.xP, otr.M, C.c_double(otr.dl), C.c_double(s)); yd = L.orc_spline_d(otr.c.yP, otr.M, C.c_double(otr.dl), C.c_double(s))
        x = L.orc_spline_val(otr.c.xP, otr.M, C.c_double(otr.dl), C.c_double(s)); y = L.orc_spline_val(otr.c.yP, otr.M, C.c_double(otr.dl), C.c_double(s))
        nrm = np.hypot(xd, yd)
        carts.append([x - yd / nrm * n, y + xd / nrm * n, np.arctan2(yd, xd) + rng.uniform(-0.1, 0.1), rng.uniform(0, 25), rng.uniform(-0.3, 0.3),
                      rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1)])
        guesses.append(s + rng.uniform(-1, 1))
    return np.array(carts), np.array(guesses)


@pytest.mark.parametrize("model", [0, 1])
def test_fused_pre_parity(fm, torch_, orc, model):
    """cl_pre_plan: frame transform, x0, lap check and out-of-race rule as cl_pre (1e-11: libm vs ocml), x_ref the oracle's walk at
    the kernel's own s."""
    torch = torch_
    tr, otr = _tracks(fm, orc, "fss2019")
    B, N = 96, 40
    carts, guesses = _random_carts(orc, otr, B, 3)
    carts[11, 0] += 1000.0; carts[50, 3] = 150.0         # two cars out of the race: off the track, beyond every physical speed
    plan = fm.Plan.profile(model, tr, N_s=97)
    tab, t = _host(plan)
    cl = fm.ClosedLoop(model, N, DT, tr, carts, reference=plan)
    cl.x_opt[:, 0, 0] = _dev(torch, guesses)
    cl.pre(); torch.cuda.synchronize()
    x0g, xrg, fing = cl.x0.cpu().numpy(), cl.x_ref.cpu().numpy(), cl.finished.cpu().numpy()
    # the live kernel on the same cars: the two kernels carry the same frame transform, x0 and finished are the same bits
    live = fm.ClosedLoop(model, N, DT, tr, carts)
    live.x_opt[:, 0, 0] = _dev(torch, guesses)
    live.pre(); torch.cuda.synchronize()
    assert np.array_equal(live.x0.cpu().numpy(), x0g) and np.array_equal(live.finished.cpu().numpy(), fing)
    for b in range(B):
        if b in (11, 50):      # out of the race (the oracle's cl_pre has no such rule): marked, x0 = 0, finite rows from the start of the plan
            assert fing[b] == 2 and (x0g[b] == 0).all() and np.isfinite(xrg[b]).all(), b
        else:
            x0, _, fin = orc.cl_pre(model, N, DT, otr, carts[b], guesses[b])
            assert fing[b] == fin, b
            assert np.max(np.abs(x0g[b] - x0)) <= 1e-11 * max(1.0, np.abs(x0).max()), b
        _check_reference(orc, model, xrg[b], tab[0], t[0], plan.ds, x0g[b, 0], N)


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("N_s,grip", [(97, 1.0), (500, 0.8)])
def test_closed_loop_short_run_on_a_plan(fm, torch_, orc, model, N_s, grip):
    """A few receding-horizon steps from standstill tracking a plan: the HIP loop against the same loop driven through the oracle
    with obtain_reference on the copied-back table.  Tolerance: the solve tolerance of x (1e-4), as for the live loop."""
    torch = torch_
    tr, otr = _tracks(fm, orc, "fss2019")
    N, B, T = 20, 3, 6
    carts = np.zeros((B, 7))
    orc.lib().orc_spline_d.restype = C.c_double
    for b in range(B):
        s = 5.0 * b
        x, y = (orc.lib().orc_spline_val(P, otr.M, C.c_double(otr.dl), C.c_double(s)) for P in (otr.c.xP, otr.c.yP))
        th = np.arctan2(orc.lib().orc_spline_d(otr.c.yP, otr.M, C.c_double(otr.dl), C.c_double(s)), orc.lib().orc_spline_d(otr.c.xP, otr.M, C.c_double(otr.dl), C.c_double(s)))
        carts[b, :3] = [x, y, th]
    plan = fm.Plan.profile(model, tr, N_s=N_s, grip=grip)
    tab, t = _host(plan)
    cl = fm.ClosedLoop(model, N, DT, tr, carts, reference=plan)
    nx = cl.nx
    k = np.arange(1, N + 1) * DT
    xo = np.zeros((B, nx, N)); uo = np.zeros((B, 2, N)); xo[:, 0, :] = 10 * k ** 2 / 2; xo[:, 3, :] = 10 * k; uo[:, 0, :] = 10
    for b in range(B): xo[b, 0, :] += 5.0 * b
    cl.x_opt[:, :, 0] += _dev(torch, 5.0 * np.arange(B))[:, None]
    oc = carts.copy(); opid = np.zeros((B, 4))
    for step in range(T):
        out = cl.step(); torch.cuda.synchronize()
        assert (out["exitflag"].cpu().numpy() == 0).all(), (step, out["exitflag"].cpu().numpy())
        for b in range(B):
            x0, _, fin = orc.cl_pre(model, N, DT, otr, oc[b], xo[b, 0, 0])
            x_ref = np.asfortranarray(pn.reference(orc, model, tab[0], t[0], plan.ds, x0[0], DT, N))
            u, xopt, sl, f, fl, it = orc.ltv_step(model, otr, N, DT, x0, x_ref, xo[b], uo[b])
            assert fl == 0
            xo[b] = xopt.reshape(N, nx).T; uo[b] = u.reshape(N, 2).T
            oc[b], opid[b], _ = orc.plant_step(oc[b], opid[b], xo[b, 3, 0], xo[b, nx - 1, 0], DT)
        assert np.max(np.abs(cl.cart.cpu().numpy() - oc)) <= 1e-4 * max(1.0, np.abs(oc).max()), step
    assert (cl.cart[:, 3] > 0.3).all()       # the cars accelerated from standstill


def _structure(cl, fl, ac):
    fin = cl.finished.cpu().numpy()
    driving = fin == 0
    assert not ((fl == -3) & ac).any()
    assert np.isfinite(cl.cart.cpu().numpy()[driving]).all()
    xr = cl.x_ref.cpu().numpy()[driving]
    assert np.isfinite(xr).all() and (np.diff(xr[:, :, 0], axis=1) > 0).all()


@pytest.mark.parametrize("model", [0, 1])
def test_monte_carlo_on_a_plan(fm, torch_, model):
    """monte_carlo(reference=plan) in small, shared plan and one plan per car with per-car parameters.  Structure only: the rates are
    reported by tools/closed_loop_bench.py --plan, not asserted."""
    tr = fm.Track.load("fss2019")
    B, steps = 128, 20
    plan = fm.Plan.profile(model, tr, N_s=500)
    cl, fl, it, ac = fm.monte_carlo(model, 20, tr, B, steps, reference=plan)
    assert cl.reference is plan and fl.shape == (steps, B)
    _structure(cl, fl, ac)
    blocks = fm.param_draws(model, range(B), 80, 0.1)
    plans = fm.Plan.profile(model, tr, N_s=97, grip=0.9, params=blocks)
    cl2, fl2, it2, ac2 = fm.monte_carlo(model, 20, tr, B, steps, params=blocks, reference=plans)
    assert plans.P == B
    _structure(cl2, fl2, ac2)
    with pytest.raises(ValueError):
        fm.monte_carlo(model, 20, tr, B - 1, steps, reference=plans)
    # reference=None is the call as it was: the live loop, the same numbers with and without the argument
    a = fm.monte_carlo(model, 20, tr, B, steps)
    b = fm.monte_carlo(model, 20, tr, B, steps, reference=None)
    assert a[0].reference is None and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[0].cart.cpu().numpy(), b[0].cart.cpu().numpy(), equal_nan=True)
    assert not np.array_equal(a[0].x_ref.cpu().numpy(), cl.x_ref.cpu().numpy())       # (and the plan is not the ramp)


@pytest.mark.parametrize("model", [0, 1])
def test_plan_with_blocking_and_warm_start(fm, torch_, model):
    torch = torch_
    tr = fm.Track.load("fss2019")
    N, B = 20, 16
    plan = fm.Plan.profile(model, tr, N_s=500)
    carts, s_init = fm.monte_carlo_carts(tr, B, 5)
    v_plan = plan.table[0, :, 2].cpu().numpy()
    carts[:, 3] = 0.8 * v_plan[np.minimum((s_init / plan.ds).astype(int), plan.N_s - 1)]     # a speed each car can hold where it starts
    cl = fm.ClosedLoop(model, N, DT, tr, carts, reference=plan, blocking=[2] * 10, warm_start=True)
    cl.x_opt[:, :, 0] += _dev(torch, s_init)[:, None]
    cl.x_opt[:, :, 3] += _dev(torch, carts[:, 3])[:, None]
    for step in range(5):
        out = cl.step()
        fl = out["exitflag"].cpu().numpy()
        assert np.isin(fl, (0, 1, -2)).all(), (step, fl)
        assert torch.isfinite(cl.x_ref).all() and torch.isfinite(cl.x_opt).all() and torch.isfinite(cl.u_opt).all(), step
    assert (cl.finished.cpu().numpy() != 2).all()       # no car lost (a car that started near the end of the lap may have completed it)
