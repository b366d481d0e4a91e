"""GPU tests of the imperfect closed loop: the noise entry, the observation and the prediction of
fsaempc_cl_observe_batch_device against the restatement (tests/latency_numpy.py, pinned by tests/test_latency_cpu.py), and ClosedLoop with
a Latency: off is off, the plant follows the plan accepted `delay` periods ago, the whole loop engaged stays finite.  B = 70 (more than one
wavefront, not a multiple of 64), N = 10, fsg2019."""
import numpy as np
import pytest

import lap_numpy as lpn
import latency_cases as lc
import latency_numpy as ln
import param_numpy as pn

pytestmark = pytest.mark.gpu

DT, B, N, SEED = lc.DT, lc.B, lc.N, lc.SEED
NOISE_TOL = 1e-12      # absolute, on |z| < 7: two decades over a few ulp of the device's log / sin / cos
OBS_TOL = 1e-12        # of max(1, |x|)
ROLL_TOL = 1e-10       # the rollout tolerance of the SQP tests, of max(1, |x|)


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


# ---- 1 ----
def test_noise_entry_matches_the_restatement(fm, torch_):
    worst = 0.0
    for nx in (5, 7):
        for step in (0, 7):
            z = fm.cl_noise(nx, B, SEED, 100, step).cpu().numpy()
            worst = max(worst, float(np.abs(z - ln.noise(nx, B, SEED, 100, step)).max()))
    print("noise entry: max |dz| %.3e" % worst)
    assert worst <= NOISE_TOL
    for nx in (5, 7):
        a, b = fm.cl_noise(nx, 70, SEED, 100, 7).cpu().numpy(), fm.cl_noise(nx, 100, SEED, 70, 7).cpu().numpy()
        assert _same_bits(a, b[30:])                      # a car's draws do not depend on the batch it sits in


# ---- 2 ----
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_observation(fm, torch_, tracks, model):
    tr, _ = tracks
    x0 = lc.states(model)
    nx = x0.shape[1]
    rng = np.random.default_rng(3)
    sigma = rng.uniform(0.01, 0.2, (B, nx))
    sigma[:, 1] = 0.0; sigma[:, nx - 1] = 0.0             # zero columns
    sigma[[4, 64, 69]] = 0.0                              # zero rows
    fin = np.zeros(B, dtype=np.int32); fin[[7, 65]] = 1; fin[33] = 2
    x0[5, 1] = -0.0; x0[64, 2] = -0.0; x0[65, 3] = -0.0   # under a zero column, in a zero row, in a finished car
    step, id0 = 7, 2 ** 33 + 5
    obs, mpc = lc.observe(fm, torch_, tr, model, x0, sigma=sigma, finished=fin, step=step, id0=id0)
    assert _same_bits(mpc, obs)                           # no delay: the MPC takes the observation
    copied = (sigma == 0) | (fin != 0)[:, None]
    assert _same_bits(obs[copied], x0[copied])
    assert np.signbit(obs[5, 1]) and np.signbit(obs[64, 2]) and np.signbit(obs[65, 3])
    ref = ln.observe(x0, sigma, fin, SEED, id0, step)
    err = np.abs(obs - ref) / np.maximum(1.0, np.abs(ref))
    print("observation: worst %.3e of max(1, |x|); %d of %d entries noisy" % (err.max(), int((~copied).sum()), copied.size))
    assert err.max() <= OBS_TOL
    assert (obs[~copied] != x0[~copied]).all()
    # one sigma for the batch, no finished list
    obs1, _ = lc.observe(fm, torch_, tr, model, x0, sigma=sigma[0], step=step, id0=id0)
    ref1 = ln.observe(x0, sigma[0], None, SEED, id0, step)
    assert (np.abs(obs1 - ref1) / np.maximum(1.0, np.abs(ref1))).max() <= OBS_TOL and _same_bits(obs1[:, 1], x0[:, 1])
    # no sigma at all: a copy
    obs2, mpc2 = lc.observe(fm, torch_, tr, model, x0, sigma=None, step=step)
    assert _same_bits(obs2, x0) and _same_bits(mpc2, x0)


# ---- 3 ----
@pytest.mark.parametrize("blocks", [False, True], ids=["defaults", "per-car-blocks"])
@pytest.mark.parametrize("integ", [0, 1, 2], ids=["euler", "rk2", "rk4"])
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_prediction(fm, torch_, orc, tracks, model, integ, blocks):
    tr, otr = tracks
    x0 = lc.states(model)
    nx = x0.shape[1]
    P = fm.param_draws(model, np.arange(B), 21 + integ, 0.2) if blocks else None
    Pn = P if blocks else np.repeat(fm.default_params(model)[None, :], B, axis=0)
    sigma = np.full(nx, 0.01)
    worst = 0.0
    for d, step in ((1, 4), (2, 4), (3, 1)):
        uh = lc.input_history(d, seed=5 + d)
        obs, mpc = lc.observe(fm, torch_, tr, model, x0, delay=d, compensate=1, sigma=sigma, step=step, u_hist=uh, params=P, integrator=integ)
        ref = np.stack([ln.predict(Pn[b], orc, model, otr, obs[b], uh[:, b], d, step, DT, integ) for b in range(B)])
        assert np.isfinite(mpc).all() and not _same_bits(mpc, obs)
        worst = max(worst, float((np.abs(mpc - ref) / np.maximum(1.0, np.abs(ref))).max()))
        obs0, mpc0 = lc.observe(fm, torch_, tr, model, x0, delay=d, compensate=0, sigma=sigma, step=step, u_hist=uh, params=P, integrator=integ)
        assert _same_bits(obs0, obs) and _same_bits(mpc0, obs0)
    print("prediction: worst %.3e of max(1, |x|)" % worst)
    assert worst <= ROLL_TOL
    if integ == (1 if model == 0 else 2):                 # -1 resolves to RK2 kinematic / RK4 dynamic
        _, dflt = lc.observe(fm, torch_, tr, model, x0, delay=d, compensate=1, sigma=sigma, step=step, u_hist=uh, params=P, integrator=-1)
        assert _same_bits(dflt, mpc)
    # a NaN in one car's first queued input: that car takes its observation, its neighbours do not notice
    car = 66
    bad = uh.copy(); bad[ln.slot(d, step, d), car, 0, 1] = np.nan
    obs_n, mpc_n = lc.observe(fm, torch_, tr, model, x0, delay=d, compensate=1, sigma=sigma, step=step, u_hist=bad, params=P, integrator=integ)
    keep = np.arange(B) != car
    assert _same_bits(obs_n, obs) and _same_bits(mpc_n[car], obs[car]) and _same_bits(mpc_n[keep], mpc[keep])
    inf = uh.copy(); inf[ln.slot(d, step, 1), car, 0, 0] = np.inf          # ... and in its last one
    _, mpc_i = lc.observe(fm, torch_, tr, model, x0, delay=d, compensate=1, sigma=sigma, step=step, u_hist=inf, params=P, integrator=integ)
    assert _same_bits(mpc_i[car], obs[car]) and _same_bits(mpc_i[keep], mpc[keep])
    later = uh.copy(); later[:, car, 1:, :] = np.nan; later[ln.slot(d, step, 0), car] = np.nan   # (stages and the slot that are not read)
    _, mpc_l = lc.observe(fm, torch_, tr, model, x0, delay=d, compensate=1, sigma=sigma, step=step, u_hist=later, params=P, integrator=integ)
    assert _same_bits(mpc_l, mpc)
    if blocks:                                            # a block that cannot describe a car behaves the same way
        Pb = P.copy(); Pb[car, pn.IDX["M"]] = -1.0
        obs_b, mpc_b = lc.observe(fm, torch_, tr, model, x0, delay=d, compensate=1, sigma=sigma, step=step, u_hist=uh, params=Pb, integrator=integ)
        assert _same_bits(obs_b, obs) and _same_bits(mpc_b[car], obs[car]) and _same_bits(mpc_b[keep], mpc[keep])


# ---- 4 ----
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_off_is_off(fm, torch_, tracks, model):
    tr, _ = tracks
    nx = 5 if model == 0 else 7
    plan = fm.Plan.profile(model, tr)

    def run(latency, reference):
        cl = fm.monte_carlo(model, N, tr, B, 5, seed=11, latency=latency, reference=reference)[0]
        return cl, [t.cpu().numpy() for t in (cl.cart, cl.x_opt, cl.finished)]
    for reference in (None, plan):
        base_cl, base = run(None, reference)
        cl, got = run(fm.Latency(), reference)
        assert cl.latency is None and cl.x0_obs is None and cl.x_hist is None and cl.plant_plan is cl.x_opt
        assert _same_bits(got[0], base[0]) and _same_bits(got[1], base[1]) and np.array_equal(got[2], base[2])
    assert (base[2] == 0).any()
    # engaged at zero noise and zero delay: the reference regenerated from x0_mpc = x0 is the walk cl_pre_plan made from the same s
    cl, got = run(fm.Latency(sigma=np.zeros(nx)), plan)
    assert cl.latency is not None and cl.x_hist is None and cl.plant_plan is cl.x_opt
    assert _same_bits(cl.x0_obs.cpu().numpy(), cl.x0.cpu().numpy()) and _same_bits(cl.x0_mpc.cpu().numpy(), cl.x0.cpu().numpy())
    assert _same_bits(got[0], base[0]) and _same_bits(got[1], base[1]) and np.array_equal(got[2], base[2])


# ---- 5 ----
def _loop(fm, torch, tr, otr, model, starts, **kw):
    cart, s0, v0, _ = lpn.cars(otr, B, starts)
    cl = fm.ClosedLoop(model, N, DT, tr, cart, **kw)
    cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
    return cl


@pytest.mark.parametrize("gate", [False, True], ids=["one-lap", "gate-fires"])
def test_latency_schedule_in_the_loop(fm, torch_, tracks, gate):
    tr, otr = tracks
    d = 2
    steps = 8 if gate else 6
    if gate:   # 3 m before the line at 10 m/s: the crossing falls inside the run (after 5 or 6 periods)
        starts = [(otr.L - 3.0, 0.05 * i, 10.0) for i in range(-3, 4)]
        cl = _loop(fm, torch_, tr, otr, fm.KINEMATIC, starts, latency=fm.Latency(delay=d), laps=2, metrics=True)
    else:
        starts = [(20.0 + 7.0 * i, 0.05 * i, 6.0 + i) for i in range(7)]
        cl = _loop(fm, torch_, tr, otr, fm.KINEMATIC, starts, latency=fm.Latency(delay=d))
    plans = [cl.x_opt.clone()]                            # the constructor's initial guess, as edited above
    seen = []
    for k in range(steps):
        cl.step()
        plans.append(cl.x_opt.clone())                    # plans[k + 1] = the plan accepted in period k
        seen.append(cl.plant_plan.clone())
    torch_.cuda.synchronize()
    for k in range(steps):
        want = plans[k - d + 1] if k >= d else plans[0]
        assert _same_bits(seen[k].cpu().numpy(), want.cpu().numpy()), k
    assert cl.x_hist.shape == (d + 1, B, N, 5) and cl.u_hist.shape == (d + 1, B, N, 2)
    assert _same_bits(cl.x_hist[(steps - 1) % (d + 1)].cpu().numpy(), cl.x_opt.cpu().numpy()) and _same_bits(cl.u_hist[(steps - 1) % (d + 1)].cpu().numpy(), cl.u_opt.cpu().numpy())
    fin = cl.finished.cpu().numpy()
    assert (fin == 0).all()                               # all cars still driving
    if gate:
        done = cl.lap_state[:, fm.LAP_STATE_INDEX["DONE"]].cpu().numpy()
        assert (done == 1).all()                          # the gate fired for every car
        rep = cl.report()
        assert np.isfinite(rep.metrics).all() and np.isfinite(rep.lap_records).all() and np.isfinite(cl.lap_times[:, 0].cpu().numpy()).all()
        assert np.isfinite(cl.x0.cpu().numpy()).all() and (cl.x0[:, 0].cpu().numpy() < 10.0).all()   # s wrapped


# ---- 6 ----
def test_whole_loop_engaged(fm, torch_, orc, tracks):
    tr, otr = tracks
    model, d = fm.DYNAMIC, 1
    sigma = np.array([0.05, 0.05, 0.01, 0.1, 0.05, 0.02, 0.005])
    plan = fm.Plan.profile(model, tr)
    starts = [(20.0 + 9.0 * i, 0.1 * (i - 3), 6.0 + i) for i in range(7)]
    cl = _loop(fm, torch_, tr, otr, model, starts, latency=fm.Latency(delay=d, compensate=True, sigma=sigma, seed=SEED, id0=1000), reference=plan,
               warm_start=True)
    for k in range(8):
        cl.step()
    torch_.cuda.synchronize()
    g = lambda t: t.cpu().numpy()
    for name in ("cart", "x_opt", "u_opt", "x0", "x0_obs", "x0_mpc", "x_ref", "x_hist", "u_hist"):
        assert np.isfinite(g(getattr(cl, name))).all(), name
    assert (g(cl.finished) == 0).all()                    # no car lost, none at the end of the track
    step = cl.steps - 1
    x0, obs, mpc, uh = g(cl.x0), g(cl.x0_obs), g(cl.x0_mpc), g(cl.u_hist)
    ref_obs = ln.observe(x0, sigma, None, SEED, 1000, step)
    assert (np.abs(obs - ref_obs) / np.maximum(1.0, np.abs(ref_obs))).max() <= OBS_TOL
    P = fm.default_params(model)
    # (the slot the last step wrote, step mod (d + 1), is not among the ones its predictor read)
    ref = np.stack([ln.predict(P, orc, model, otr, obs[b], uh[:, b], d, step, DT, -1) for b in range(B)])
    err = float((np.abs(mpc - ref) / np.maximum(1.0, np.abs(ref))).max())
    print("whole loop: x0_mpc against the restatement %.3e of max(1, |x|); moved by up to %.3f m in s" % (err, np.abs(mpc[:, 0] - obs[:, 0]).max()))
    assert err <= ROLL_TOL
    assert not _same_bits(mpc, obs)
    assert _same_bits(g(cl.plant_plan), g(cl.x_hist[(step - d) % (d + 1)]))


# ---- 7 ----
def test_abi_refusals(fm):
    lc.check_abi_refusals("cuda")
