"""GPU tests of the closed loop's state estimator: fsaempc_cl_estimate_batch_device against the restatement
(tests/estimator_numpy.py, pinned by tests/test_estimator_cpu.py) -- the Jacobian against Richardson-extrapolated differences of
param_numpy.psi, the prediction against param_numpy.psi, the algebra of one period against the restatement fed the device's own F, the
bit-for-bit rules (symmetry, finished cars, first period, unmeasured components, re-initialisations, batch independence), the re-basing
-- and ClosedLoop with an Estimator: the wiring and the schedule of the filter's input.  B = 70 (nine wavefronts of 8 cars, the last
group of lanes partial), N = 10, fsg2019."""
import numpy as np
import pytest

import estimator_cases as ec
import estimator_numpy as en
import lap_numpy as lpn
import latency_cases as lc
import param_numpy as pn

pytestmark = pytest.mark.gpu

DT, B, N = ec.DT, ec.B, ec.N
JAC_REQ = 1e-6         # of max(1, |F|): what the differences themselves must reach (a dropped kappa'(s) term is orders above)
JAC_TOL = 1.25e-8      # of max(1, |F|): 10 x the largest device-vs-differences discrepancy measured, 1.25e-9 (dynamic, RK2, per-car blocks;
                       # DESIGN.md 6q) -- the differences' own error: their two extrapolations are up to 1.9e-8 apart
ROLL_TOL = 1e-10       # of max(1, |x|): the tolerance of test_latency_gpu.py's prediction test, for the same function
ALG_TOL = 1e-10        # relative to the largest entry


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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case(tr, model, seed=1):
    """A period's inputs: states whose arc length sits 0.3 .. 1.0 m into a spline segment (3.03 m long: the stages of a step advance s
    by at most 0.75 m, so every stencil s +- 1e-3 stays inside the segment), an SPD covariance per car, measurements a few sigma away."""
    assert tr.dl > 2.0
    x = lc.states(model)
    nx = x.shape[1]
    x[:, 0] = np.floor(x[:, 0] / tr.dl) * tr.dl + 0.3 + 0.01 * np.arange(B)
    rng = np.random.default_rng(seed)
    sig = np.array([0.05, 0.05, 0.01, 0.1, 0.005]) if model == 0 else np.array([0.05, 0.05, 0.01, 0.1, 0.05, 0.02, 0.005])
    A = rng.standard_normal((B, nx, nx)) * sig[None, :, None]
    P = A @ A.transpose(0, 2, 1) + np.einsum("i,ij->ij", sig ** 2, np.eye(nx))[None]
    P = 0.5 * (P + P.transpose(0, 2, 1))
    z = x + 2.0 * sig * rng.standard_normal((B, nx))
    u = lc.input_history(0, seed=7 + seed)[0]
    cnt = np.tile(np.array([[3, 0]], dtype=np.int32), (B, 1))
    return dict(x=x, P=P, z=z, u=u, cnt=cnt, r=sig ** 2, q=0.1 * sig ** 2, p0=4 * sig ** 2, x_start=x + 0.05)


# ---- 1, 2: Jacobian and prediction ----
@pytest.mark.parametrize("blocks", [False, True], ids=["defaults", "per-car-blocks"])
@pytest.mark.parametrize("integ", [0, 1, 2], ids=["euler", "rk2", "rk4"])
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_jacobian_and_prediction(fm, torch_, orc, tracks, model, integ, blocks):
    tr, otr = tracks
    c = _case(tr, model)
    nx = c["x"].shape[1]
    Pb = fm.param_draws(model, np.arange(B), 31 + integ, 0.2) if blocks else None
    Pn = Pb if blocks else np.repeat(fm.default_params(model)[None, :], B, axis=0)
    out = ec.estimate(fm, torch_, tr, model, z=c["z"], x_start=c["x_start"], u_prev=c["u"], q=c["q"], r=c["r"], p0=c["p0"], est_x=c["x"], est_P=c["P"],
                      est_count=c["cnt"], params=Pb, integrator=integ)
    assert (out["est_count"] == np.array([4, 0])).all() and np.isfinite(out["F_out"]).all()
    ref = np.stack([pn.psi(Pn[b], orc, model, otr, c["x"][b], c["u"][b, 0], DT, integ) for b in range(B)])
    roll = float((np.abs(out["x_prior"] - ref) / np.maximum(1.0, np.abs(ref))).max())
    worst, levels = 0.0, 0.0
    for b in range(B):
        J, lvl = en.psi_jacobian(Pn[b], orc, model, otr, c["x"][b], c["u"][b, 0], DT, integ, h=1e-3)
        scale = max(1.0, np.abs(J).max())
        levels = max(levels, lvl / scale)
        worst = max(worst, float(np.abs(out["F_out"][b] - J).max()) / scale)
    print("prediction: worst %.3e of max(1, |x|); Jacobian: device against differences %.3e of max(1, |F|), the two Richardson levels apart by %.3e"
          % (roll, worst, levels))
    assert levels <= JAC_REQ                                # on the CPU first: the differences agree with themselves
    assert roll <= ROLL_TOL
    assert worst <= JAC_REQ and worst <= JAC_TOL
    if integ == (1 if model == 0 else 2):                   # -1 resolves to RK2 kinematic / RK4 dynamic
        dflt = ec.estimate(fm, torch_, tr, model, z=c["z"], x_start=c["x_start"], u_prev=c["u"], q=c["q"], r=c["r"], p0=c["p0"], est_x=c["x"], est_P=c["P"],
                           est_count=c["cnt"], params=Pb, integrator=-1)
        assert all(_same_bits(dflt[k], out[k]) for k in ("F_out", "x_prior", "est_P", "x0_est"))


# ---- 3: algebra of one period ----
def _restate(c, out, fin=None, q=None, r=None, L=0.0):
    q = c["q"] if q is None else q
    r = c["r"] if r is None else r
    res = []
    for b in range(B):
        qb, rb = (q[b] if np.ndim(q) == 2 else q), (r[b] if np.ndim(r) == 2 else r)
        predict = lambda x, u, b=b: (out["x_prior"][b].copy(), out["F_out"][b])
        res.append(en.period(c["x"][b], c["P"][b], tuple(c["cnt"][b]), c["z"][b], c["x_start"][b], c["u"][b, 0], 0 if fin is None else fin[b], qb, rb, c["p0"],
                             L, predict))
    return res


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_algebra_of_one_period(fm, torch_, tracks, model):
    """est_P, x0_est, innov and nis against the restatement fed the device's own F_out (and prior): per-car q and r, unmeasured components
    (+inf; NaN and a negative value, which only the device can see), an exact measurement (r = 0), finished cars, first-period cars."""
    tr, _ = tracks
    c = _case(tr, model, seed=2)
    nx = c["x"].shape[1]
    rng = np.random.default_rng(5)
    r = np.tile(c["r"], (B, 1)) * rng.uniform(0.5, 2.0, (B, nx))
    q = np.tile(c["q"], (B, 1)) * rng.uniform(0.5, 2.0, (B, nx))
    r[::3, nx - 2] = np.inf; r[1::5, 2] = np.inf; r[4, 1] = np.nan; r[68, 3] = -1.0
    fin = np.zeros(B, dtype=np.int32); fin[[7, 65]] = 1; fin[33] = 2
    c["cnt"][[2, 40, 69], 0] = 0                          # first period: the prior is x_start
    # an exact measurement, on first-period cars only: r_i = 0 leaves P_ii = p - (p p) / p, which is 0 or an ulp either side of it, and a
    # negative one re-initialises the car (step 7); from diag(p0) both sides hold the same bits of p, after a prediction they would not
    r[[2, 40, 69], 1] = 0.0
    out = ec.estimate(fm, torch_, tr, model, z=c["z"], x_start=c["x_start"], u_prev=c["u"], q=q, r=r, p0=c["p0"], est_x=c["x"], est_P=c["P"],
                      est_count=c["cnt"], finished=fin)
    ref = _restate(c, out, fin, q, r)
    worst = 0.0
    for b in range(B):
        R = ref[b]
        for k in ("est_P", "x0_est", "innov", "est_x"):
            worst = max(worst, float(np.abs(out[k][b] - R[k]).max() / max(np.abs(R[k]).max(), 1e-300)))
        worst = max(worst, abs(out["nis"][b] - R["nis"]) / max(abs(R["nis"]), 1e-300) if R["nis"] else abs(out["nis"][b]))
        assert tuple(out["est_count"][b]) == R["count"], b
    print("one period against the restatement: worst %.3e relative to the largest entry" % worst)
    assert worst <= ALG_TOL
    live = fin == 0
    inexact = live & ~(r == 0).any(axis=1)
    assert (out["est_count"][inexact, 1] == 0).all() and (out["nis"][live] > 0).all()
    assert np.abs(out["x0_est"][[2, 40, 69], 1] - c["z"][[2, 40, 69], 1]).max() <= 1e-15   # r = 0: the estimate is the measurement
    unmeasured = ~(np.isfinite(r) & (r >= 0))
    assert unmeasured.sum() > 30 and (out["innov"][unmeasured] == 0).all() and (out["innov"][~unmeasured & live[:, None]] != 0).all()
    # a finished car: x0_est = z bit for bit, nothing carried is written
    for b in (7, 33, 65):
        assert _same_bits(out["x0_est"][b], c["z"][b]) and (out["innov"][b] == 0).all() and out["nis"][b] == 0
        assert _same_bits(out["est_x"][b], c["x"][b]) and _same_bits(out["est_P"][b], c["P"][b]) and (out["est_count"][b] == c["cnt"][b]).all()
    # the first period uses x_start, and F = I
    for b in (2, 40, 69):
        assert _same_bits(out["x_prior"][b], c["x_start"][b]) and np.array_equal(out["F_out"][b], np.eye(nx)) and out["est_count"][b, 0] == 1
    for b in np.flatnonzero(live):
        assert _same_bits(out["est_P"][b], out["est_P"][b].T), b
        assert _same_bits(out["est_x"][b], out["x0_est"][b])


# ---- 4: bit-for-bit rules ----
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_chained_periods_resets_and_batch_independence(fm, torch_, tracks, model):
    tr, _ = tracks
    c = _case(tr, model, seed=3)
    nx = c["x"].shape[1]
    rng = np.random.default_rng(9)
    Pb = fm.param_draws(model, np.arange(B), 77, 0.1)
    r = c["r"].copy(); r[nx - 2] = np.inf
    kw = dict(q=c["q"], r=r, p0=c["p0"], x_start=c["x_start"])

    def chain(z_seq, u_seq, params, plant=None, sel=slice(None)):
        st = dict(est_x=np.full((B, nx), 123.0)[sel], est_P=np.full((B, nx, nx), 123.0)[sel], est_count=np.zeros((B, 2), dtype=np.int32)[sel])
        outs = []
        for k, (z, u) in enumerate(zip(z_seq, u_seq)):
            if plant is not None and k in plant:
                st = plant[k](st)
            o = ec.estimate(fm, torch_, tr, model, z=z[sel], u_prev=u[sel], est_x=st["est_x"], est_P=st["est_P"], est_count=st["est_count"],
                            params=params[sel], **{k_: (v[sel] if k_ == "x_start" else v) for k_, v in kw.items()})
            outs.append(o); st = o
        return outs
    zs = [c["x_start"] + 0.3 * k * np.eye(nx)[0] * c["x"][:, 3:4] * DT + np.sqrt(c["r"]) * rng.standard_normal((B, nx)) for k in range(6)]
    us = [lc.input_history(0, seed=20 + k)[0] for k in range(6)]
    base = chain(zs, us, Pb)
    last = base[-1]
    assert (last["est_count"] == np.array([6, 0])).all() and np.isfinite(last["est_P"]).all()
    assert _same_bits(last["est_P"], last["est_P"].transpose(0, 2, 1))                # symmetric after 6 chained periods
    assert (np.diagonal(last["est_P"], axis1=1, axis2=2) > 0).all()
    # planted before period 3: a NaN in one car's est_P, a block that cannot describe a car, a non-finite input -- three 8-lane groups
    cars = (19, 42, 69)

    def nan_P(st):
        P = st["est_P"].copy(); P[cars[0], 1, 2] = np.nan
        return dict(st, est_P=P)
    Pbad = Pb.copy(); Pbad[cars[1], pn.IDX["M"]] = -1.0
    ubad = [u.copy() for u in us]; ubad[3][cars[2], 0, 1] = np.inf
    o_nan = chain(zs[3:4], us[3:4], Pb, plant={0: lambda st: nan_P(dict(base[2]))})[0]
    o_par = chain(zs[3:4], us[3:4], Pbad, plant={0: lambda st: dict(base[2])})[0]
    o_u = chain(zs[3:4], ubad[3:4], Pb, plant={0: lambda st: dict(base[2])})[0]
    want = en.seq_update(np.zeros(nx), np.diag(c["p0"]), np.zeros(nx), r)[1]            # the updated diag(p0) (every innovation is 0)
    for car, o in zip(cars, (o_nan, o_par, o_u)):
        assert _same_bits(o["x0_est"][car], zs[3][car]) and _same_bits(o["est_x"][car], zs[3][car]), car
        assert tuple(o["est_count"][car]) == (1, 1) and np.array_equal(o["est_P"][car], want), car
        assert (o["innov"][car] == 0).all() and o["nis"][car] == 0
        others = np.arange(B) != car
        for k in ("x0_est", "est_x", "est_P", "innov", "nis", "x_prior"):              # the neighbours in the group do not notice
            assert _same_bits(o[k][others], base[3][k][others]), (car, k)
        assert np.array_equal(o["est_count"][others], base[3]["est_count"][others])
    # the cars 13 .. 36 alone (an offset that is no multiple of 8) equal their results inside the batch of 70
    sel = slice(13, 37)
    alone = chain(zs[:3], us[:3], Pb, sel=sel)
    for k in ("x0_est", "est_x", "est_P", "innov", "nis", "F_out", "x_prior"):
        assert _same_bits(alone[2][k], base[2][k][sel]), k
    assert np.array_equal(alone[2]["est_count"], base[2]["est_count"][sel])


# ---- 5: re-basing ----
def test_rebasing(fm, torch_, tracks):
    tr, _ = tracks
    model = 0
    c = _case(tr, model, seed=4)
    L = tr.L
    delta = 0.2 + 0.01 * np.arange(B)
    xs = c["x"].copy(); xs[:, 0] = L + delta                  # the prior: just past the line
    z = xs.copy(); z[:, 0] = delta + 0.003                    # the measurement: the gate took L off
    cnt = np.zeros((B, 2), dtype=np.int32)                    # (a first period: the prior is x_start itself)
    kw = dict(z=z, x_start=xs, u_prev=c["u"], q=c["q"], r=c["r"], p0=c["p0"], est_count=cnt)
    on = ec.estimate(fm, torch_, tr, model, L=L, **kw)
    off = ec.estimate(fm, torch_, tr, model, L=0.0, **kw)
    ref = np.array([en.rebase(xs[b, 0], z[b, 0], L, True) for b in range(B)])
    assert _same_bits(on["x_prior"][:, 0], ref) and np.abs(on["x_prior"][:, 0] - delta).max() < 1e-9
    assert np.abs(on["x0_est"][:, 0] - delta).max() < 0.003 and (on["est_count"][:, 1] == 0).all()
    assert _same_bits(off["x_prior"][:, 0], xs[:, 0]) and (off["x0_est"][:, 0] > 1.0 + delta).all()   # L = 0 leaves it alone
    r = c["r"].copy(); r[0] = np.inf                          # s unmeasured: nothing to re-base on
    un = ec.estimate(fm, torch_, tr, model, L=L, **dict(kw, r=r))
    assert _same_bits(un["x_prior"][:, 0], xs[:, 0])


# ---- 6: in the loop ----
def _loop(fm, torch, tr, otr, model, starts, **kw):
    cart, s0, v0, _ = lpn.cars(otr, B, starts)
    cl = fm.ClosedLoop(model, N, DT, tr, cart, **kw)
    cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
    return cl


def test_estimator_in_the_loop(fm, torch_, tracks):
    """Dynamic model, plan reference, warm start, laps = 2 across a gate crossing, noise, d = 1 compensated, 6 steps: x0_est of every period
    equals the stand-alone entry on the cloned inputs of that period with u_prev = stage 1 of u_hist[(k - 1 - d) mod (d + 1)], x0_mpc equals
    the observe entry with sigma = NULL applied to x0_est, bit for bit; everything stays finite."""
    tr, otr = tracks
    model, d, steps = fm.DYNAMIC, 1, 6
    sigma = np.array([0.05, 0.05, 0.01, 0.1, 0.05, 0.02, 0.005])
    qv = 0.1 * sigma ** 2
    plan = fm.Plan.profile(model, tr)
    starts = [(otr.L - 1.5, 0.05 * i, 10.0) for i in range(-3, 4)]      # 1.5 m before the line at 10 m/s: the crossing falls inside the run
    lat = fm.Latency(delay=d, compensate=True, sigma=sigma, seed=lc.SEED, id0=1000)
    cl = _loop(fm, torch_, tr, otr, model, starts, latency=lat, reference=plan, warm_start=True, laps=2, estimator=fm.Estimator(qv))
    g = lambda t: t.cpu().numpy().copy()
    crossed = False
    for k in range(steps):
        before = dict(est_x=g(cl.est_x), est_P=g(cl.est_P), est_count=g(cl.est_count))
        if k == 0:
            u_prev = g(cl.u_opt)                                        # (the history is filled from the initial guess at the first step)
        else:
            u_prev = g(cl.u_hist[(k - 1 - d) % (d + 1)])
        assert k == 0 or _same_bits(u_prev, g(cl.prev_input()))
        done_before = g(cl.lap_state[:, fm.LAP_STATE_INDEX["DONE"]])
        cl.step()
        z, x_start, fin = g(cl.x0_obs), g(cl.est_x_start), g(cl.finished)
        ref = ec.estimate(fm, torch_, tr, model, z=z, x_start=x_start, u_prev=u_prev, q=qv, r=sigma ** 2, p0=sigma ** 2, L=tr.L, est_x=before["est_x"],
                          est_P=before["est_P"], est_count=before["est_count"], want=False)
        assert (fin == 0).all()
        for name, key in (("x0_est", "x0_est"), ("est_x", "est_x"), ("est_P", "est_P"), ("est_innov", "innov"), ("est_nis", "nis")):
            assert _same_bits(g(getattr(cl, name)), ref[key]), (k, name)
        assert np.array_equal(g(cl.est_count), ref["est_count"])
        uh = g(cl.u_hist)
        uh[k % (d + 1)] = np.nan                                        # (the slot this step wrote is not among the ones its predictor read)
        _, mpc = lc.observe(fm, torch_, tr, model, g(cl.x0_est), delay=d, compensate=1, sigma=None, step=k, u_hist=uh)
        assert _same_bits(g(cl.x0_mpc), mpc), k
        assert not _same_bits(g(cl.x0_mpc), g(cl.x0_est))
        crossed = crossed or bool((g(cl.lap_state[:, fm.LAP_STATE_INDEX["DONE"]]) > done_before).any())
    torch_.cuda.synchronize()
    assert crossed                                                      # the gate fired inside the run: the estimate was re-based
    for name in ("cart", "x_opt", "u_opt", "x0", "x0_obs", "x0_est", "x0_mpc", "x_ref", "x_hist", "u_hist", "est_x", "est_P", "est_innov", "est_nis"):
        assert np.isfinite(g(getattr(cl, name))).all(), name
    assert (g(cl.est_resets) == 0).all() and (g(cl.est_count)[:, 0] == steps).all()
    assert np.abs(g(cl.x0_est)[:, 0] - g(cl.x0)[:, 0]).max() < 0.5      # the estimate followed the gate's wrap of s


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_estimator_none_is_off(fm, torch_, tracks, model):
    tr, _ = tracks

    def run(**kw):
        cl = fm.monte_carlo(model, N, tr, B, 5, seed=11, **kw)[0]
        return cl, [t.cpu().numpy() for t in (cl.cart, cl.x_opt, cl.finished)]
    _, base = run()
    cl, got = run(estimator=None)
    assert cl.estimator is None and cl.x0_est is None and cl.est_P is None and cl.est_resets is None
    assert _same_bits(got[0], base[0]) and _same_bits(got[1], base[1]) and np.array_equal(got[2], base[2])
    # without a latency the measurement is x0 itself: the engaged loop runs and filters it
    nx = 5 if model == 0 else 7
    cl, _ = run(estimator=fm.Estimator([1e-4] * nx, r=[1e-4] * nx))
    assert cl.x0_obs is None and cl.x0_mpc is cl.x0_est and np.isfinite(cl.x0_est.cpu().numpy()).all() and (cl.est_count[:, 0] > 0).any().item()


# ---- 7 ----
def test_abi_refusals(fm):
    ec.check_abi_refusals("cuda")
