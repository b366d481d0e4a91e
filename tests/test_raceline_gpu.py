"""GPU tests of the minimum-curvature racing line: the line QP against its numpy restatement (tests/raceline_numpy.py)
and bit for bit against itself, the solved line against the oracle's solver on the same H and g with the numpy KKT certificate, the
profile on the device's own line against numpy, zero control points against the centre-line planner (bit for bit), the isolation of
per-plan widths, the walk and the closed loop on a table whose n and mu columns are not zero, and the refusals."""
import ctypes as C

import numpy as np
import pytest
from conftest import relerr

import plan_numpy as pn
import raceline_numpy as rn
from kkt_numpy import kkt_certificate

pytestmark = pytest.mark.gpu

BUILD_TOL = 1e-9      # the project's construction tolerance; test_raceline_cpu.py::test_line_profile_conditioning: a 1e-13 input difference stays below 1e-11
KKT_TOL = 1e-6        # the tolerance of tests/test_gpu_parity.py
LINE_TOL = 1e-6       # m, |line - oracle's solve of the same H, g|: the issue's ceiling (to become ten times the measured value)
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


@pytest.mark.parametrize("N_s,N_c", [(128, 32), (500, 117)])
def test_line_qp_parity(fm, torch_, orc, N_s, N_c):
    tr, otr = _tracks(fm, orc, "fss2019")
    H, g = fm.raceline_qp(tr, N_s, N_c)
    H2, g2 = fm.raceline_qp(tr, N_s, N_c)
    H, g, H2, g2 = (a.cpu().numpy() for a in (H, g, H2, g2))
    assert np.array_equal(H, H2) and np.array_equal(g, g2)            # the same bits on every call
    Hn, gn = rn.qp(orc, otr, N_s, N_c)
    scale = np.abs(Hn).max()
    print("max |H - numpy| / max |H| %.3e, max |g - numpy| %.3e" % (np.abs(H - Hn).max() / scale, np.abs(g - gn).max()))
    assert np.abs(H - Hn).max() <= BUILD_TOL * scale and np.abs(g - gn).max() <= BUILD_TOL * max(scale, np.abs(gn).max())
    assert np.array_equal(H, H.T)
    jj, kk = np.meshgrid(np.arange(N_c), np.arange(N_c), indexing="ij")
    assert (H[np.minimum((jj - kk) % N_c, (kk - jj) % N_c) > 5] == 0.0).all()


@pytest.mark.parametrize("N_s,N_c", [(128, 32), (500, 100), (500, 117)])
def test_raceline_parity(fm, torch_, orc, N_s, N_c):
    """The smallest tile count, the one-wavefront kernel's range and the workgroup kernel (N_c = 117 > 116)."""
    tr, otr = _tracks(fm, orc, "fss2019")
    margin, w = 0.25, 0.5
    k = _kappa(orc, otr, N_s)
    H, g = (a.cpu().numpy() for a in fm.raceline_qp(tr, N_s, N_c))
    lb, ub = np.full(N_c, -w), np.full(N_c, w)
    xo, fo, flo, ito, lamo = orc.qp_solve(H, g, np.zeros((0, N_c)), lb, ub, np.zeros(0), np.zeros(0))
    assert flo == 0
    for model in (0, 1):
        plan = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=margin)
        assert plan.P == 1 and plan.N_s == N_s and tuple(plan.line.shape) == (1, N_c) and tuple(plan.line_flag.shape) == (1,)
        c = plan.line.cpu().numpy()[0]
        assert int(plan.line_flag[0]) == 0
        lam = rn.multipliers(H, g, lb, ub, c)
        cert = kkt_certificate(H[None], g[None], np.zeros((1, N_c, 0)), lb[None], ub[None], np.zeros((1, 0)), np.zeros((1, 0)), c[None], lam[None])
        assert cert["max"][0] <= KKT_TOL, cert
        print("model %d: max |line - oracle| %.3e m, on a bound %d of %d" % (model, np.abs(c - xo).max(), int((np.abs(c) >= w - 1e-9).sum()), N_c))
        assert np.abs(c - xo).max() <= LINE_TOL
        # the profile on the device's own line: solver differences stay out of this comparison
        tab, t = _host(plan)
        ref = rn.line_profile(model, k, otr.L, c, 20.0, 1.0, margin=margin)
        for col in range(8):
            assert relerr(tab[0][:, col], ref["table"][:, col]) <= BUILD_TOL, (model, "column", col, relerr(tab[0][:, col], ref["table"][:, col]))
        assert relerr(t[0], ref["t"]) <= BUILD_TOL, (model, "t")
        assert np.array_equal(tab[0][:, 3], np.zeros(N_s)) and (np.abs(tab[0][:, 0]) <= w + 1e-12).all() and tab[0][:, 0].any() and tab[0][:, 1].any()
        centre = fm.Plan.profile(model, tr, N_s=N_s)
        assert plan.lap_time()[0] < centre.lap_time()[0]


@pytest.mark.parametrize("model", [0, 1])
def test_zero_line_is_the_centre_line_planner(fm, torch_, model):
    tr = fm.Track.load("fss2019")
    for N_s, N_c in ((128, 32), (500, 100), (97, 8)):
        a = fm.Plan.profile(model, tr, N_s=N_s, grip=0.8)
        b = fm.Plan.profile(model, tr, N_s=N_s, grip=0.8, line=np.zeros(N_c))
        assert np.array_equal(*map(lambda p: p.table.cpu().numpy(), (a, b))) and np.array_equal(a.t.cpu().numpy(), b.t.cpu().numpy()), (N_s, N_c)
    blocks = fm.param_draws(model, range(3), 77, 0.2)
    a = fm.Plan.profile(model, tr, N_s=128, params=blocks)
    for line in (np.zeros(32), np.zeros((3, 32))):
        b = fm.Plan.profile(model, tr, N_s=128, params=blocks, line=line)
        assert b.P == 3 and np.array_equal(a.table.cpu().numpy(), b.table.cpu().numpy()) and np.array_equal(a.t.cpu().numpy(), b.t.cpu().numpy())


@pytest.mark.parametrize("model", [0, 1])
def test_per_plan_widths_are_isolated(fm, torch_, orc, model):
    tr, otr = _tracks(fm, orc, "fss2019")
    N_s, N_c = 128, 32
    blocks = np.repeat(fm.default_params(model)[None], 4, axis=0)
    widths = (0.75, 0.5, 0.3)
    for j, w in enumerate(widths):
        blocks[j, fm.PARAM_INDEX["N_MAX"]] = w
    blocks[3, fm.PARAM_INDEX["M"]] = -1.0                          # a block that cannot describe a car
    plans = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=0.0, params=blocks)
    tab, t = _host(plans)
    line, flag = plans.line.cpu().numpy(), plans.line_flag.cpu().numpy()
    assert plans.P == 4 and np.isnan(tab[3]).all() and np.isnan(t[3]).all() and np.isnan(line[3]).all()
    for j, w in enumerate(widths):
        one = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=0.0, params=blocks[j])
        tj, ttj = _host(one)
        assert flag[j] == 0 and int(one.line_flag[0]) == 0
        assert np.array_equal(line[j], one.line.cpu().numpy()[0]) and np.array_equal(tab[j], tj[0]) and np.array_equal(t[j], ttj[0]), j
        assert np.abs(line[j]).max() <= w + 1e-12 and np.abs(line[j]).max() >= w - 1e-9       # the width is used, and kept
    # the user's-own-line entry on the same control points gives the same plans
    own = fm.Plan.profile(model, tr, N_s=N_s, params=blocks[:3], line=line[:3])
    assert np.array_equal(own.table.cpu().numpy(), tab[:3]) and np.array_equal(own.t.cpu().numpy(), t[:3])
    # no width left: NaN, whatever the QP said
    none = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=0.75)
    assert np.isnan(none.t.cpu().numpy()).all() and np.isnan(none.line.cpu().numpy()).all()


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
def test_reference_on_a_racing_line(fm, torch_, orc, model):
    """The walk on a table whose n and mu columns are not zero."""
    tr = fm.Track.load("fss2019")
    N = 40
    plan = fm.Plan.raceline(model, tr, N_s=128, N_c=32)
    tab, t = _host(plan)
    assert np.abs(tab[0][:, 0]).max() > 0.1 and np.abs(tab[0][:, 1]).max() > 0.01
    rng = np.random.default_rng(12)
    s0 = np.concatenate([[0.0, tr.L, 5 * plan.ds, 1234.5], rng.uniform(0, 3 * tr.L, 60)])
    got = plan.reference(model, s0, N, DT).cpu().numpy()
    for b in range(64):
        _check_reference(orc, model, got[b], tab[0], t[0], plan.ds, s0[b], N)
    assert np.abs(got[:, :, 1]).max() > 0.1 and np.abs(got[:, :, 2]).max() > 0.01


@pytest.mark.parametrize("model", [0, 1])
def test_closed_loop_short_run_on_a_racing_line(fm, torch_, orc, model):
    """tests/test_plan_gpu.py::test_closed_loop_short_run_on_a_plan with a racing-line plan: the HIP loop against the same loop driven
    through the oracle with obtain_reference on the copied-back table, at the solve tolerance of x (1e-4)."""
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
    plan = fm.Plan.raceline(model, tr, N_s=128, N_c=32)
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
    assert np.abs(cl.x_ref.cpu().numpy()[:, :, 1]).max() > 0          # and the reference they track leaves the centre line


def test_refusals_come_before_any_launch(fm, torch_):
    torch = torch_
    L = fm.lib()
    tr = fm.Track.load("fss2019")
    xP, yP = tr.device(torch.device("cuda:0"))
    p = lambda a: C.c_void_p(a.data_ptr())
    sp = fm._lib.Spline(tr.M, tr.dl, p(xP), p(yP))
    N_s, N_c = 64, 16
    seven = lambda n, dt=torch.float64: torch.full((n,), 7, dtype=dt, device="cuda")
    H, g, line, flag, table, tt = seven(N_c * N_c), seven(N_c), seven(N_c), seven(1, torch.int32), seven(N_s * 8), seven(N_s)
    need = L.fsaempc_plan_raceline_workspace_bytes(1, N_c)
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device="cuda")
    nan, inf = float("nan"), float("inf")
    qp = lambda ns=N_s, nc=N_c: L.fsaempc_raceline_build_qp_device(C.byref(sp), C.c_double(tr.L), ns, nc, p(H), p(g), None)
    prof = lambda ns=N_s, nc=N_c, gr=1.0: L.fsaempc_plan_line_profile_batch_device(1, C.byref(sp), C.c_double(tr.L), None, 1, ns, nc, p(line), 0, C.c_double(20.0),
                                                                                   C.c_double(gr), p(table), p(tt), None)
    race = lambda ns=N_s, nc=N_c, m=0.25, gr=1.0, wsb=need: L.fsaempc_plan_raceline_batch_device(
        1, C.byref(sp), C.c_double(tr.L), None, 1, ns, nc, C.c_double(m), C.c_double(20.0), C.c_double(gr), None, p(line), p(flag), p(table), p(tt), p(ws),
        C.c_longlong(wsb), None)
    for kw in (dict(nc=7), dict(nc=197, ns=500), dict(ns=2 * N_c - 1), dict(ns=2049, nc=100)):
        assert qp(**kw) == -1 and prof(**kw) == -1 and race(**kw) == -1, kw
    assert prof(gr=1.5) == -1 and race(gr=nan) == -1
    for m in (-0.01, nan, inf):
        assert race(m=m) == -1, m
    assert race(wsb=need - 64) == -5
    torch.cuda.synchronize()
    assert all(bool((a == 7).all()) for a in (H, g, line, flag, table, tt)) and not bool(ws.any())
    with pytest.raises(ValueError):
        fm.Plan.raceline(fm.DYNAMIC, tr, N_s=100, N_c=64)
