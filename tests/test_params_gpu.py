"""GPU tests of the per-instance vehicle, cost and limit parameters (fsaempc_ltv_params and the *_p entries).  The
oracle has the reference's constants compiled in, so away from the defaults the tests rest on identities of the build and on the
numpy statement of the models with a block as argument (tests/param_numpy.py, pinned to the oracle at the defaults by
tests/test_params_cpu.py)."""
import math

import numpy as np
import pytest

import param_numpy as pn
from conftest import relerr
from kkt_numpy import kkt_certificate

pytestmark = pytest.mark.gpu

DT = 0.05
KKT_TOL = 1e-6          # the tolerances of tests/test_gpu_parity.py
FVAL_TOL = 1e-6
X_TOL = 5e-3
X_TOL_VERTEX = 1e-6
SHAPES = [(0, 20), (0, 40), (1, 40), (1, 60)]
QP_KEYS = ("H", "g", "A", "lb", "ub", "lbA", "ubA", "pred", "Bt", "const")
I = pn.IDX


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


@pytest.fixture(scope="module")
def tracks(fm, orc):
    return fm.Track.load("fsg2019"), orc.Track.load(fm.tracks._HERE + "/tracks/fsg2019.json")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _np(torch, d):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _build(fm, torch, tr, model, N, inp, params, integrator=-1):
    x0, xl, ul, xr = inp
    mpc = fm.LtvBatch(model, N, DT, tr, x0.shape[0], integrator=integrator, params=params)
    return _np(torch, mpc.build_qp(_dev(torch, x0), _dev(torch, xr), _dev(torch, xl), _dev(torch, ul)))


def _step(fm, torch, tr, model, N, inp, params, **kw):
    x0, xl, ul, xr = inp
    mpc = fm.LtvBatch(model, N, DT, tr, x0.shape[0], params=params)
    return _np(torch, mpc.step(_dev(torch, x0), _dev(torch, xr), _dev(torch, xl), _dev(torch, ul), **kw))


def _sqp(fm, torch, tr, model, N, x0, xr, u0, params, **kw):
    out = fm.SqpBatch(model, N, DT, tr, x0.shape[0], params=params).solve(_dev(torch, x0), _dev(torch, xr), _dev(torch, u0), **kw)
    return _np(torch, out)


def _with(default, draws, entries):
    """Per-instance blocks: the default everywhere but `entries`, which come from `draws`."""
    P = np.repeat(default[None, :], draws.shape[0], axis=0)
    P[:, entries] = draws[:, entries]
    return P


# ---- 5 ----
@pytest.mark.parametrize("model,N", SHAPES)
def test_defaults_reproduce_the_fixed_path(fm, torch_, tracks, model, N):
    """The parameterised entries with default blocks (shared, and one per instance) against the entries with the constants compiled
    in: the build to 1e-9 relative on every tensor (the project's tolerance for the same arithmetic from a different compilation),
    the fused step to the tolerances of test_fused_step_parity.  Largest differences measured on the MI355X: build
    exactly 0 (kinematic) and 1.4e-24 (dynamic: one ubA entry of the tyre rows); step exactly 0 (kinematic), 2.4e-11 in u (dynamic
    N = 40), 5.1e-4 in u on an instance with an interior-point iterate (dynamic N = 60)."""
    torch = torch_
    tr, _ = tracks
    B = 64
    inp = fm.instances(model, N, DT, tr.L, 20190, range(B))
    d = fm.default_params(model)
    ref = _build(fm, torch, tr, model, N, inp, None)
    sref = _step(fm, torch, tr, model, N, inp, None, want_aux=True)
    worst = 0.0
    for params in (d, np.repeat(d[None], B, 0)):
        q = _build(fm, torch, tr, model, N, inp, params)
        for k in QP_KEYS:
            e = relerr(q[k], ref[k])
            worst = max(worst, e)
            assert e <= 1e-9, k
        s = _step(fm, torch, tr, model, N, inp, params, want_aux=True)
        assert np.array_equal(s["exitflag"], sref["exitflag"])
        ok = sref["exitflag"] == 0
        tol = np.where((s["polished"] > 0) & (sref["polished"] > 0), X_TOL_VERTEX, X_TOL)
        for k in ("u_opt", "x_opt"):
            err = np.abs(s[k] - sref[k]).max(axis=1) / np.maximum(1.0, np.abs(sref[k]).max(axis=1))
            print("step", model, N, k, "max rel diff", err[ok].max())
            assert (err[ok] <= tol[ok]).all(), (k, err)
        assert (np.abs(s["fval"] - sref["fval"])[ok] <= FVAL_TOL * np.maximum(1.0, np.abs(sref["fval"][ok]))).all()
    print("build", model, N, "max rel diff over all tensors", worst)


def test_sqp_with_default_blocks_follows_the_fixed_path(fm, torch_, tracks):
    """Not one of the issue's cases; a guard for the parameterised SQP kernels of the dynamic model (initial rollout, exact build,
    line search), which no other test compares with the fixed ones.  One sweep from the same start with default blocks against the
    entry with the constants compiled in: equal statuses and u_opt, x_opt to X_TOL_VERTEX on at least 90 % of the instances (the
    two line searches take the same discrete decisions except where a trial sits on the Armijo edge, and the ellipse table of the
    block is rounded differently from the compiler's constants in the last bit)."""
    torch = torch_
    tr, _ = tracks
    model, N, B = 1, 40, 32
    x0, _, ul, xr = fm.instances(model, N, DT, tr.L, 31, range(B))
    a = _sqp(fm, torch, tr, model, N, x0, xr, ul, None, max_sweeps=1)
    b = _sqp(fm, torch, tr, model, N, x0, xr, ul, np.repeat(fm.default_params(model)[None], B, 0), max_sweeps=1)
    same = a["status"] == b["status"]
    for k in ("u_opt", "x_opt"):
        err = np.abs(a[k] - b[k]).max(axis=1) / np.maximum(1.0, np.abs(a[k]).max(axis=1))
        print("SQP one sweep", k, "max rel diff", err.max())
        same &= err <= X_TOL_VERTEX
    assert same.sum() >= math.ceil(0.9 * B), same


# ---- 6 ----
@pytest.mark.parametrize("model,N", SHAPES)
def test_cost_block(fm, torch_, tracks, model, N):
    """Drawn Q_*, Q_TERMINAL, R_*, R_SOFT*: H, g, qconst are the numpy recomputation from the kernel's own Bt, pred, x_ref
    (1e-10 / 1e-9 / 1e-9: the tolerances of test_exact_build_matches_numpy); everything else is the default build's to 1e-12."""
    torch = torch_
    tr, _ = tracks
    B = 64
    inp = fm.instances(model, N, DT, tr.L, 20190, range(B))
    nx, ns, nV, nC = fm.dims(model, N)
    P = _with(fm.default_params(model), fm.param_draws(model, np.arange(B), 11, 0.2), list(range(9, 19)))
    ref = _build(fm, torch, tr, model, N, inp, None)
    q = _build(fm, torch, tr, model, N, inp, P)
    for k in ("A", "Bt", "pred", "lb", "ub", "lbA", "ubA"):
        assert relerr(q[k], ref[k]) <= 1e-12, k
    xr = inp[3].reshape(B, -1)
    for b in range(B):
        Bt = q["Bt"][b].T                                   # (nx N, nV)
        W = pn.weights(P[b], N, nx).ravel()
        R = np.concatenate([pn.r_diag(P[b], N), np.zeros(ns)])
        r = q["pred"][b] - xr[b]
        assert _rel(q["H"][b], 2 * (Bt.T @ (W[:, None] * Bt) + np.diag(R))) <= 1e-10, b
        gs = np.concatenate([np.zeros(2 * N), pn.r_soft(P[b], model)])
        assert _rel(q["g"][b], 2 * Bt.T @ (W * r) + gs) <= 1e-9, b
        assert abs(q["const"][b] - np.sum(W * r * r)) <= 1e-9 * max(1.0, abs(q["const"][b])), b


# ---- 7 ----
@pytest.mark.parametrize("model,N", SHAPES)
def test_limit_block(fm, torch_, tracks, model, N):
    """Drawn entries 19-25: the matrices and the cost do not move, lb / ub are the new input limits, and each finite side of
    lbA / ubA moves by the change of its own limit."""
    torch = torch_
    tr, _ = tracks
    B = 64
    inp = fm.instances(model, N, DT, tr.L, 20190, range(B))
    d = fm.default_params(model)
    P = _with(d, fm.param_draws(model, np.arange(B), 12, 0.2), list(range(19, 26)))
    P[:, I["V_MIN"]] = np.linspace(-1.0, 1.0, B)          # (a relative draw of a zero default stays zero)
    ref = _build(fm, torch, tr, model, N, inp, None)
    q = _build(fm, torch, tr, model, N, inp, P)
    for k in ("A", "H", "g", "Bt", "pred", "const"):
        assert relerr(q[k], ref[k]) <= 1e-12, k
    for b in range(B):
        lim = np.tile([P[b, I["U_ACC_MAX"]], P[b, I["U_STEER_MAX"]]], N)
        assert np.array_equal(q["ub"][b][:2 * N], lim) and np.array_equal(q["lb"][b][:2 * N], -lim)
        assert np.array_equal(q["lb"][b][2 * N:], ref["lb"][b][2 * N:]) and np.array_equal(q["ub"][b][2 * N:], ref["ub"][b][2 * N:])
        lo_new, hi_new = pn.bounds(P[b], model, N)
        lo_def, hi_def = pn.bounds(d, model, N)
        for new, old, e_new, e_def in ((q["lbA"][b], ref["lbA"][b], lo_new, lo_def), (q["ubA"][b], ref["ubA"][b], hi_new, hi_def)):
            fin = np.isfinite(e_def)
            assert np.array_equal(np.isfinite(old), fin) and np.array_equal(np.isfinite(new), fin)
            assert np.array_equal(new[~fin], old[~fin])
            move = (new[fin] - old[fin]) - (e_new[fin] - e_def[fin])
            assert np.max(np.abs(move)) <= 1e-12 * max(1.0, np.max(np.abs(old[fin & (np.abs(e_def) < 1e9)]))), b


# ---- 8 ----
@pytest.mark.parametrize("model", [0, 1])
def test_vehicle_block_in_the_ltv_build(fm, torch_, orc, tracks, model):
    """Entries 0-8 drawn (spread 0.2), Euler, N = 12.  Linearised about its own rollout the build reproduces that rollout (1e-10;
    independent of the Jacobians).  The build is affine in x0, so central differences of pred[0:nx] in x0 are Ad_1 = I + dt J, J the
    central-difference Jacobian of the numpy f under the block in states 2..nx (column 1 is zero by construction), to 1e-6 of
    max|J|; the dynamic entry (ydd, thetad) differs by -5 exp(-xd / 5)."""
    torch = torch_
    tr, otr = tracks
    N, B = 12, 64
    nx = 5 if model == 0 else 7
    x0, _, _, xr = fm.instances(model, N, DT, tr.L, 20190, range(B))
    rng = np.random.default_rng(8 + model)
    P = np.repeat(fm.default_params(model)[None], B, 0)
    P[:, :9] *= 1 + 0.2 * rng.uniform(-1, 1, (B, 9))
    ul = np.stack([rng.uniform(-2, 2, (B, N)), rng.uniform(-0.08, 0.08, (B, N))], axis=2)
    X = np.array([pn.rollout(P[b], orc, model, otr, x0[b], ul[b], DT, pn.EULER) for b in range(B)])   # x_1 .. x_N
    xl = np.concatenate([x0[:, None, :], X[:, :-1, :]], axis=1)
    q = _build(fm, torch, tr, model, N, (x0, xl, ul, xr), P, integrator=0)
    for b in range(B):
        got = q["pred"][b] + q["Bt"][b][:2 * N].T @ ul[b].ravel()
        assert _rel(got, X[b].ravel()) <= 1e-10, b
    h = 1e-2
    Ad = np.zeros((B, nx, nx))
    for j in range(nx):
        xp, xm = x0.copy(), x0.copy()
        xp[:, j] += h; xm[:, j] -= h
        qp = _build(fm, torch, tr, model, N, (xp, xl, ul, xr), P, integrator=0)
        qm = _build(fm, torch, tr, model, N, (xm, xl, ul, xr), P, integrator=0)
        Ad[:, :, j] = (qp["pred"][:, :nx] - qm["pred"][:, :nx]) / (2 * h)
    hj = 1e-6
    for b in range(B):
        J = np.zeros((nx, nx))
        for j in range(1, nx):
            e = np.zeros(nx); e[j] = hj
            J[:, j] = (pn.f_model(P[b], orc, model, otr, xl[b, 0] + e, ul[b, 0]) - pn.f_model(P[b], orc, model, otr, xl[b, 0] - e, ul[b, 0])) / (2 * hj)
        A = (Ad[b] - np.eye(nx)) / DT
        diff = A - J
        tol = 1e-6 * np.max(np.abs(J))
        if model == 1:
            assert abs(diff[4, 5] - (-5 * math.exp(-xl[b, 0, 3] / 5))) <= tol, (b, diff[4, 5])
            diff[4, 5] = 0.0
        assert np.max(np.abs(diff)) <= tol, (b, np.max(np.abs(diff)), tol)


# ---- 9 ----
@pytest.mark.parametrize("model,N", [(0, 20), (1, 40)])
@pytest.mark.parametrize("integ", [0, 1, 2])
def test_exact_build_under_parameters(fm, torch_, orc, tracks, model, N, integ):
    """test_exact_build_matches_numpy restated on tests/param_numpy.py with drawn blocks (spread 0.2, every entry param_draws moves):
    rollout 1e-12, Bt and A columns against central differences 1e-6, bounds 1e-8, H 1e-10, g and qconst 1e-9."""
    torch = torch_
    tr, otr = tracks
    B = 2
    x0, _, _, xr = fm.instances(model, N, DT, tr.L, 31, range(B))
    P = fm.param_draws(model, np.arange(B), 9 + integ, 0.2)
    P[:, I["V_MIN"]] = [0.5, -0.5]
    rng = np.random.default_rng(5 + model + 3 * integ)
    u = np.stack([rng.uniform(-2, 2, (B, N)), rng.uniform(-0.08, 0.08, (B, N))], axis=2)
    sb = fm.SqpBatch(model, N, DT, tr, B, integrator=integ, params=P)
    q = _np(torch, sb.build_qp(_dev(torch, x0), _dev(torch, xr), _dev(torch, u)))
    nx, ns, nV, nC = fm.dims(model, N)
    h = 1e-5
    for b in range(B):
        Pb = P[b]
        lo, hi = pn.bounds(Pb, model, N)
        X = pn.rollout(Pb, orc, model, otr, x0[b], u[b], DT, integ)
        assert _rel(q["pred"][b], X.ravel()) <= 1e-12
        Phi = q["Bt"][b][:2 * N].T
        Amat = q["A"][b].T
        C0 = pn.rows(Pb, model, X, u[b])
        for j in range(2 * N):
            up, um = u[b].copy(), u[b].copy()
            up.flat[j] += h; um.flat[j] -= h
            Xp, Xm = pn.rollout(Pb, orc, model, otr, x0[b], up, DT, integ), pn.rollout(Pb, orc, model, otr, x0[b], um, DT, integ)
            assert _rel(Phi[:, j], ((Xp - Xm) / (2 * h)).ravel()) <= 1e-6, (b, j)
            fd = (pn.rows(Pb, model, Xp, up) - pn.rows(Pb, model, Xm, um)) / (2 * h)
            assert _rel(Amat[:, j], fd) <= 1e-6, (b, j)
        ul = u[b].ravel()
        lin0 = C0 - Amat[:, :2 * N] @ ul
        for bnd, exp in ((q["lbA"][b], lo), (q["ubA"][b], hi)):
            m = np.isfinite(exp) & (np.abs(exp) < 1e9)
            assert np.max(np.abs(bnd[m] + lin0[m] - exp[m])) <= 1e-8 * max(1.0, np.abs(C0).max())
            assert np.array_equal(bnd[~m], exp[~m])
        lim = np.tile([Pb[I["U_ACC_MAX"]], Pb[I["U_STEER_MAX"]]], N)
        assert np.array_equal(q["ub"][b][:2 * N], lim) and np.array_equal(q["lb"][b][:2 * N], -lim)
        W = pn.weights(Pb, N, nx).ravel()
        off = X.ravel() - Phi @ ul - xr[b].ravel()
        assert _rel(q["H"][b][:2 * N, :2 * N], 2 * (Phi.T @ (W[:, None] * Phi) + np.diag(pn.r_diag(Pb, N)))) <= 1e-10
        assert _rel(q["g"][b][:2 * N], 2 * Phi.T @ (W * off)) <= 1e-9
        assert np.array_equal(q["g"][b][2 * N:], pn.r_soft(Pb, model))
        assert abs(q["const"][b] - np.sum(W * off ** 2)) <= 1e-9 * max(1.0, abs(q["const"][b]))


# ---- 10 ----
@pytest.mark.parametrize("model,N", [(0, 40), (1, 40)])
def test_solve_under_parameters(fm, torch_, tracks, model, N):
    """B = 256, one param_draws(spread = 0.1) block per instance.  Every instance with exit flag 0 passes the numpy KKT certificate
    (KKT_TOL) on the tensors the parameterised build produced; at most ceil(0.5 % B) more non-zero flags than the entry with the
    constants compiled in gives on the same ids (the solver's own end-game misses are of that order); planned inputs,
    steering angles and speeds obey the drawn limits to 1e-6.
    Measured on the MI355X (non-zero flags, drawn blocks / defaults): kinematic N = 40 0 / 0, dynamic N = 40 0 / 0."""
    torch = torch_
    tr, _ = tracks
    B = 256
    inp = fm.instances(model, N, DT, tr.L, 20190, range(B))
    P = fm.param_draws(model, np.arange(B), 20190, 0.1)
    nx = 5 if model == 0 else 7
    base = _step(fm, torch, tr, model, N, inp, None)
    q = _build(fm, torch, tr, model, N, inp, P)
    s = _step(fm, torch, tr, model, N, inp, P, want_lambda=True)
    n_def, n_par = int(np.sum(base["exitflag"] != 0)), int(np.sum(s["exitflag"] != 0))
    print("non-zero exit flags", model, N, "drawn blocks", n_par, "defaults", n_def)
    assert n_par <= n_def + math.ceil(0.005 * B), (n_par, n_def)
    ok = np.flatnonzero(s["exitflag"] == 0)
    x = np.concatenate([s["u_opt"], s["slack"]], axis=1)
    c = kkt_certificate(*(q[k][ok] for k in ("H", "g", "A", "lb", "ub", "lbA", "ubA")), x[ok], s["lam"][ok])
    assert c["max"].max() <= KKT_TOL, {k: float(np.max(c[k])) for k in ("stationarity", "primal", "sign", "complementarity")}
    U = s["u_opt"][ok].reshape(len(ok), N, 2)
    Xo = s["x_opt"][ok].reshape(len(ok), N, nx)
    Pk = P[ok]
    assert (np.abs(U[:, :, 0]) <= Pk[:, None, I["U_ACC_MAX"]] + 1e-6).all() and (np.abs(U[:, :, 1]) <= Pk[:, None, I["U_STEER_MAX"]] + 1e-6).all()
    assert (np.abs(Xo[:, :, nx - 1]) <= Pk[:, None, I["DELTA_MAX"]] + 1e-6).all()
    assert (Xo[:, :, 3] >= Pk[:, None, I["V_MIN"]] - 1e-6).all()


# ---- 11 ----
STEP_KEYS = ("u_opt", "x_opt", "slack", "fval", "exitflag", "iter")
SQP_KEYS = ("u_opt", "x_opt", "slack", "fval", "status", "sweeps", "qp_iter", "merit")


def test_instances_with_their_own_blocks_are_isolated(fm, torch_, tracks):
    """Instance b of a per-instance batch gives bitwise the result of a B = 1 call with block b shared: step and SQP."""
    torch = torch_
    tr, _ = tracks
    B = 16
    for model, N in ((0, 40), (1, 40)):
        inp = fm.instances(model, N, DT, tr.L, 31, range(B))
        P = fm.param_draws(model, np.arange(B), 31, 0.1)
        full = _step(fm, torch, tr, model, N, inp, P)
        for b in (0, 7, 15):
            one = _step(fm, torch, tr, model, N, tuple(a[b:b + 1] for a in inp), P[b])
            for k in STEP_KEYS:
                assert np.array_equal(one[k][0], full[k][b], equal_nan=True), (model, b, k)
    model, N = 0, 20
    x0, _, ul, xr = fm.instances(model, N, DT, tr.L, 31, range(B))
    P = fm.param_draws(model, np.arange(B), 31, 0.1)
    full = _sqp(fm, torch, tr, model, N, x0, xr, ul, P)
    for b in (0, 7, 15):
        one = _sqp(fm, torch, tr, model, N, x0[b:b + 1], xr[b:b + 1], ul[b:b + 1], P[b])
        for k in SQP_KEYS:
            assert np.array_equal(one[k][0], full[k][b], equal_nan=True), (b, k)


# ---- 12 ----
def _plant_once(fm, torch, tr, model, N, carts, plan, plant_params):
    cl = fm.ClosedLoop(model, N, DT, tr, carts, plant_params=plant_params)
    cl.x_opt = _dev(torch, plan)
    cl.plant(None)
    torch.cuda.synchronize()
    return cl.cart.cpu().numpy(), cl.pid.cpu().numpy(), cl.u_last.cpu().numpy()


def test_invalid_blocks_fail_alone(fm, torch_, tracks):
    """NaN mass in instance 3 and a negative N_MAX in instance 7 of 16: exit flag -1 with iter = 0 (SQP: status -1; plant: the car
    keeps its state); the other 14 are bitwise what they are without the bad neighbours."""
    torch = torch_
    tr, _ = tracks
    B = 16
    rest = np.ones(B, dtype=bool); rest[[3, 7]] = False
    for model, N in ((0, 20), (1, 40)):
        inp = fm.instances(model, N, DT, tr.L, 31, range(B))
        P = fm.param_draws(model, np.arange(B), 31, 0.1)
        bad = P.copy()
        bad[3, I["M"]] = np.nan
        bad[7, I["N_MAX"]] = -0.1
        good = _step(fm, torch, tr, model, N, inp, P)
        out = _step(fm, torch, tr, model, N, inp, bad)
        assert out["exitflag"][3] == -1 and out["exitflag"][7] == -1 and out["iter"][3] == 0 and out["iter"][7] == 0
        for k in STEP_KEYS:
            assert np.array_equal(out[k][rest], good[k][rest], equal_nan=True), (model, k)
        x0, _, ul, xr = inp
        sg = _sqp(fm, torch, tr, model, N, x0, xr, ul, P, max_sweeps=4)
        sb = _sqp(fm, torch, tr, model, N, x0, xr, ul, bad, max_sweeps=4)
        assert sb["status"][3] == -1 and sb["status"][7] == -1
        for k in SQP_KEYS:
            assert np.array_equal(sb[k][rest], sg[k][rest], equal_nan=True), (model, k)
        rng = np.random.default_rng(12)
        nx = 5 if model == 0 else 7
        carts = np.concatenate([rng.uniform(-20, 20, (B, 3)), rng.uniform(1, 20, (B, 1)), rng.uniform(-0.3, 0.3, (B, 3))], axis=1)
        plan = np.zeros((B, N, nx)); plan[:, 0, 3] = rng.uniform(0, 25, B); plan[:, 0, nx - 1] = rng.uniform(-0.3, 0.3, B)
        cg, pg, ug = _plant_once(fm, torch, tr, model, N, carts, plan, P)
        cb, pb, ub = _plant_once(fm, torch, tr, model, N, carts, plan, bad)
        assert np.array_equal(cb[[3, 7]], carts[[3, 7]]) and np.array_equal(pb[[3, 7]], np.zeros((2, 4)))
        assert not np.array_equal(cg[3], carts[3])
        for a, b_ in ((cb, cg), (pb, pg), (ub, ug)):
            assert np.array_equal(a[rest], b_[rest])


# ---- 13 ----
def test_sqp_under_parameters(fm, torch_, orc, tracks):
    """test_sqp_converges_to_kkt_points restated on tests/param_numpy.py for the kinematic model, N = 20, with param_draws(0.1):
    every status-0 instance is a rollout of the numpy model under its block (1e-10), feasible at tol_feas under its limits, its
    slack is at least slack_min - 1e-12, fval is the numpy objective (1e-9) and its merit never rose.  The count of status-0
    instances is printed beside the count with default blocks on the same ids; no floor beyond "at least one" (the SQP's
    convergence rate is an open item).  Measured on the MI355X: 57 of 64 with drawn blocks, 60 of 64 with defaults."""
    torch = torch_
    tr, otr = tracks
    model, N, B = 0, 20, 64
    x0, _, ul, xr = fm.instances(model, N, DT, tr.L, 31, range(B))
    P = fm.param_draws(model, np.arange(B), 31, 0.1)
    out = _sqp(fm, torch, tr, model, N, x0, xr, ul, P)
    base = _sqp(fm, torch, tr, model, N, x0, xr, ul, np.repeat(fm.default_params(model)[None], B, 0))
    ok = np.flatnonzero(out["status"] == 0)
    print("SQP status 0: drawn blocks", len(ok), "default blocks", int(np.sum(base["status"] == 0)), "of", B)
    assert len(ok) >= 1, np.unique(out["status"], return_counts=True)
    tol_feas = fm._lib.sqp_default_opts().tol_feas
    for b in ok:
        U = out["u_opt"][b].reshape(N, 2)
        X = pn.rollout(P[b], orc, model, otr, x0[b], U, DT, pn.RK2)
        assert _rel(out["x_opt"][b], X.ravel()) <= 1e-10, b
        assert pn.hard_violation(P[b], X)[1] <= tol_feas and out["hard_viol"][b] <= tol_feas, b
        assert np.all(out["slack"][b] >= pn.slack_min(P[b], model, X, U) - 1e-12), b
        assert abs(out["fval"][b] - pn.objective(P[b], model, X, U, out["slack"][b], xr[b])) <= 1e-9 * max(1.0, abs(out["fval"][b])), b
        m = out["merit"][b][: out["sweeps"][b]]
        assert np.all(np.isfinite(m)) and np.all(np.diff(m) <= 1e-12 * np.abs(m[:-1])), (b, m)


# ---- 14 ----
@pytest.mark.parametrize("model", [0, 1])
def test_plant_under_parameters(fm, torch_, tracks, model):
    """fsaempc_cl_plant_batch_device_p on 64 random cars with drawn blocks against the numpy plant step (cart 1e-11, pid 1e-10,
    u_last 1e-8 relative: the tolerances of test_closed_loop_pieces_parity); with default blocks against the existing entry."""
    torch = torch_
    tr, _ = tracks
    B, N = 64, 40
    nx = 5 if model == 0 else 7
    rng = np.random.default_rng(14 + model)
    carts = np.concatenate([rng.uniform(-20, 20, (B, 2)), rng.uniform(-3, 3, (B, 1)), rng.uniform(0, 25, (B, 1)), rng.uniform(-0.3, 0.3, (B, 2)),
                            rng.uniform(-0.1, 0.1, (B, 1))], axis=1)
    plan = np.zeros((B, N, nx)); plan[:, 0, 3] = rng.uniform(0, 25, B); plan[:, 0, nx - 1] = rng.uniform(-0.3, 0.3, B)
    P = fm.param_draws(model, np.arange(B), 14, 0.2)
    P[:, 28:32] *= 1 + 0.2 * rng.uniform(-1, 1, (B, 4))
    cg, pg, ug = _plant_once(fm, torch, tr, model, N, carts, plan, P)
    for b in range(B):
        x, pid, u = pn.plant_step(P[b], carts[b], np.zeros(4), plan[b, 0, 3], plan[b, 0, nx - 1], DT)
        assert np.max(np.abs(cg[b] - x)) <= 1e-11 * max(1.0, np.abs(x).max()), b
        assert np.max(np.abs(pg[b] - pid)) <= 1e-10 * max(1.0, np.abs(pid).max()), b
        assert np.max(np.abs(ug[b] - u)) <= 1e-8 * max(1.0, np.abs(u).max()), b
    c0, p0, u0 = _plant_once(fm, torch, tr, model, N, carts, plan, None)
    for params in (fm.default_params(model), np.repeat(fm.default_params(model)[None], B, 0)):
        c1, p1, u1 = _plant_once(fm, torch, tr, model, N, carts, plan, params)
        assert _rel(c1, c0) <= 1e-11 and _rel(p1, p0) <= 1e-10 and _rel(u1, u0) <= 1e-8


# ---- 15 ----
def _loop(fm, torch, tr, model, N, carts, s_init, steps, **kw):
    cl = fm.ClosedLoop(model, N, DT, tr, carts, **kw)
    cl.x_opt[:, :, 0] += _dev(torch, s_init)[:, None]
    cl.x_opt[:, :, 3] += _dev(torch, carts[:, 3])[:, None]
    for _ in range(steps):
        cl.step()
    torch.cuda.synchronize()
    return cl.cart.cpu().numpy()


@pytest.mark.parametrize("model", [0, 1])
def test_closed_loop_under_parameters(fm, torch_, tracks, model):
    """Six closed-loop steps.  Default blocks: the loop without blocks to 1e-9 relative (measured: exactly 0 kinematic, 4.3e-16
    dynamic).  One block per
    car: car b is bitwise the B = 1 loop of that car.  A plant 20 % heavier than the controller's model moves the cars by more
    than 1e-6: the plant reads its own block."""
    torch = torch_
    tr, _ = tracks
    N, B, T = 20, 8, 6
    carts, s_init = fm.monte_carlo_carts(tr, B, 15)
    d = fm.default_params(model)
    plain = _loop(fm, torch, tr, model, N, carts, s_init, T)
    dflt = _loop(fm, torch, tr, model, N, carts, s_init, T, params=d)
    print("closed loop", model, "default block vs none, rel diff of cart", _rel(dflt, plain))
    assert _rel(dflt, plain) <= 1e-9
    P = fm.param_draws(model, np.arange(B), 15, 0.1)
    per = _loop(fm, torch, tr, model, N, carts, s_init, T, params=P)
    for b in (0, 3, 7):
        one = _loop(fm, torch, tr, model, N, carts[b:b + 1], s_init[b:b + 1], T, params=P[b])
        assert np.array_equal(one[0], per[b]), b
    heavy = d.copy(); heavy[I["M"]] *= 1.2
    mism = _loop(fm, torch, tr, model, N, carts, s_init, T, params=d, plant_params=heavy)
    assert np.max(np.abs(mism - dflt)) > 1e-6


# ---- 16 ----
def test_unparameterised_paths_refuse_a_batch_with_parameters(fm, torch_, tracks):
    torch = torch_
    tr, _ = tracks
    model, N, B = 0, 20, 4
    x0, xl, ul, xr = (_dev(torch, a) for a in fm.instances(model, N, DT, tr.L, 31, range(B)))
    mpc = fm.LtvBatch(model, N, DT, tr, B, params=fm.default_params(model))
    with pytest.raises(NotImplementedError):
        fm.ltv_step_lambda(mpc, x0, xr, xl, ul)
    with pytest.raises(NotImplementedError):
        fm.ltv_step_vjp(mpc, {}, x0, xr, xl, ul, ubar=torch.zeros((B, 2 * N), dtype=torch.float64, device="cuda"))
    with pytest.raises(NotImplementedError):
        fm.feedback_gain(mpc, x0, xr, xl, ul)
    with pytest.raises(NotImplementedError):
        fm.ltv_step_affine_maps(mpc, xl, ul)
    with pytest.raises(NotImplementedError):
        fm.ltv_step_diff(mpc, x0, xr, xl, ul)
    out = mpc.sqp(x0, xr, xl, ul, sweeps=2)            # the fixed-sweep loop runs on the parameterised step
    torch.cuda.synchronize()
    assert (out["exitflag"] == 0).all()
    mpc.set_params(None)                               # and without a block everything works as before
    K, status = fm.feedback_gain(mpc, x0, xr, xl, ul)
    Abar, Crow = fm.ltv_step_affine_maps(mpc, xl, ul)
    fwd = fm.ltv_step_lambda(mpc, x0, xr, xl, ul)
    r = fm.ltv_step_vjp(mpc, fwd, x0, xr, xl, ul, ubar=torch.ones((B, 2 * N), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert tuple(K.shape) == (B, 2, 5) and tuple(Abar.shape) == (B, 5, 5 * N) and tuple(r["x0"].shape) == (B, 5)
    assert bool(torch.isfinite(K).all()) and bool((status >= 0).all())
