"""GPU tests of the closed loop's cone-based localisation: fsaempc_cl_cone_sense_batch_device and
fsaempc_cl_estimate_cones_batch_device against the restatement (tests/cone_loc_numpy.py, pinned by tests/test_cone_loc_cpu.py) -- the
observations (counts and indices exactly, range and bearing at the tolerance of tests/test_latency_gpu.py), batch independence, the filter
without cones against fsaempc_cl_estimate_cart_batch_device bit for bit, the composed rows bit for bit, the algebra of one period, the
rows that must not be applied, localising without a pose measurement on the synthetic drive -- and ClosedLoop with a ConeSensor.
B = 70 (nine wavefronts of 8 cars, the last group of lanes partial), N = 10, fsg2019, both models."""
import numpy as np
import pytest

import cone_loc_cases as cc
import cone_loc_numpy as cn
import lap_numpy as lpn
import sensors_cases as sc
import sensors_numpy as sn
import test_sensors_gpu as s6

pytestmark = pytest.mark.gpu

DT, B, N = cc.DT, cc.B, cc.N
Z_TOL = 1e-12          # NOISE_TOL / OBS_TOL of tests/test_latency_gpu.py: of max(1, |value|)
G_REQ = 1e-12          # of the largest entry: the fallback bound of the issue
G_TOL = 0.0            # the composed rows are formed with +, -, *, / and sqrt only out of h0, h1 and H, which the device holds bit for bit
ALG_TOL = 1e-10        # relative to the largest entry: the value of tests/test_sensors_gpu.py


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


_same_bits, _rel = s6._same_bits, s6._rel


# ---- 1: the cone sensor ----
SENSE_CASES = {"default": dict(), "p-detect-0.7": dict(p_detect=0.7), "r-max-20": dict(r_max=20.0), "k-max-3": dict(k_max=3), "512-per-side": dict(),
               "sigma-0": dict(sigma=(0.0, 0.0))}


@pytest.mark.parametrize("case", list(SENSE_CASES))
def test_cone_sense(fm, torch_, tracks, case):
    """cone_n, cone_seen and cone_id equal the restatement's exactly, rho_m and beta_m to Z_TOL, for every car (no exclusions: the
    restatement's candidates keep 1e-9 from the view's edges and from each other's ranges); finished cars see nothing; the cars 13 .. 36
    alone, in another batch under the same ids, give the same bits."""
    tr, otr = tracks
    cart = cc.poses(otr)
    left, right = cc.synthetic_map(cart) if case == "512-per-side" else cc.cone_map()
    kw = dict(cc.SENSOR, **SENSE_CASES[case])
    fin = np.zeros(B, dtype=np.int32); fin[[7, 65]] = 1; fin[33] = 2
    id0, step = 1000, 17
    d = cc.Direct(fm, torch_, tr, 0, B)
    out = d.cone_sense(cart, left, right, id0=id0, step=step, finished=fin, **kw)
    ref = cn.sense(left, right, cart, id0, step, finished=fin, seed=cc.SEED, **kw)
    assert cc.margins_ok(ref["cand"], kw["r_min"], kw["r_max"], kw["fov"])
    assert np.array_equal(out["n"], ref["n"]) and np.array_equal(out["seen"], ref["seen"]) and np.array_equal(out["ids"], ref["ids"])
    err = float((np.abs(out["z"] - ref["z"]) / np.maximum(1.0, np.abs(ref["z"]))).max())
    print("cone_sense %s: kept %d .. %d, seen %d .. %d, z against the restatement %.3e" % (case, ref["n"].min(), ref["n"].max(), ref["seen"].min(),
                                                                                          ref["seen"].max(), err))
    assert err <= Z_TOL
    live = fin == 0
    assert (out["n"][live] > 0).all() and (out["n"][~live] == 0).all() and (out["seen"][~live] == 0).all()
    assert (out["ids"][~live] == -1).all() and (out["z"][~live] == 0).all()
    k = np.arange(kw["k_max"])[None, :]
    assert (out["ids"][k >= out["n"][:, None]] == -1).all() and (out["z"][k >= out["n"][:, None]] == 0).all()
    if case == "r-max-20":
        assert (ref["seen"] > 16).any() and (ref["seen"][live] < 16).any() and ref["n"].max() == 16
    if case == "512-per-side":
        assert (ref["seen"] > 16).any() and out["ids"].max() >= 960          # the sixteenth stride of the lanes is reached
    if case == "sigma-0":                                                    # a sigma of 0 copies: the true range, in ascending order
        assert all((np.diff(out["z"][b, : out["n"][b], 0]) >= 0).all() for b in range(B))
    sel = slice(13, 37)
    alone = cc.Direct(fm, torch_, tr, 0, 24).cone_sense(cart[sel], left, right, id0=id0 + 13, step=step, finished=fin[sel], **kw)
    for key in ("n", "seen", "ids"):
        assert np.array_equal(alone[key], out[key][sel]), key
    assert _same_bits(alone["z"], out["z"][sel])


def test_cone_sense_truncation_order_with_a_doubled_cone(fm, torch_, tracks):
    """One position in both lists: equal true ranges are ordered by the index, on the device as in the restatement."""
    tr, otr = tracks
    cart = cc.poses(otr)
    left, right = cc.cone_map()
    right = np.concatenate([right, left])                        # every left cone once more at the end of the right list
    kw = dict(cc.SENSOR, sigma=(0.0, 0.0), k_max=8)
    d = cc.Direct(fm, torch_, tr, 0, B)
    out = d.cone_sense(cart, left, right, id0=3, step=2, **kw)
    ref = cn.sense(left, right, cart, 3, 2, seed=cc.SEED, **kw)
    assert np.array_equal(out["ids"], ref["ids"]) and np.array_equal(out["n"], ref["n"]) and np.array_equal(out["seen"], ref["seen"])
    pairs = 0
    for b in range(B):
        keys = [(float(out["z"][b, k, 0]), int(out["ids"][b, k])) for k in range(out["n"][b])]      # (sigma = 0: z holds the true range)
        assert keys == sorted(keys), b
        pairs += sum(1 for p, q in zip(keys, keys[1:]) if p[0] == q[0])
    assert pairs > B


# ---- 2: no cones is 6s ----
def _observations(d, otr, model, c, left, right, step=4, **over):
    """The device's observations of the cars of a case, seen from where they will be predicted"""
    nxt = c["x"].copy(); nxt[:, 0] += c["x"][:, 3] * DT
    return d.cone_sense(s6._carts(otr, model, nxt), left, right, id0=200, step=step, **dict(cc.SENSOR, **over))


@pytest.mark.parametrize("blocks", [False, True], ids=["defaults", "per-car-blocks"])
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_without_cones_it_is_the_cartesian_filter(fm, torch_, tracks, model, blocks):
    """With cone_n = 0 for all cars, and separately with real observations and both r_cone = +inf, every common output equals
    fsaempc_cl_estimate_cart_batch_device bit for bit: the first period and a chained one."""
    tr, otr = tracks
    c = s6._case(tr, otr, model, seed=8)
    left, right = cc.cone_map()
    Pb = fm.param_draws(model, np.arange(B), 31, 0.2) if blocks else None
    d = cc.Direct(fm, torch_, tr, model, B, params=Pb)
    obs = _observations(d, otr, model, c, left, right)
    assert (obs["n"] > 0).all()
    fin = np.zeros(B, dtype=np.int32); fin[[7, 65]] = 1
    common = ("est_x", "est_P", "x0_est", "innov", "nis", "F_out", "x_prior", "H_out")
    for label, n, rc in (("no observations", np.zeros(B, dtype=np.int32), cc.R_CONE), ("both channels off", obs["n"], [np.inf, np.inf])):
        st_a = st_b = dict(est_x=None, est_P=None, est_count=None)
        for period in range(2):
            kw = dict(y=c["y"], x_proj=c["x_proj"], u_prev=c["u"], q=c["q"], r=c["r"], p0=c["p0"], finished=fin)
            a = d.estimate(**kw, **st_a)
            b = d.estimate_cones(map_left=left, map_right=right, cone_n=n, cone_id=obs["ids"], cone_z=obs["z"], r_cone=rc, **kw, **st_b)
            for key in common:
                assert _same_bits(a[key], b[key]), (label, period, key)
            assert np.array_equal(a["est_count"], b["est_count"]) and (b["cone_innov"] == 0).all() and (b["G_out"] == 0).all()
            assert np.array_equal(b["rows_used"], np.where(fin == 0, sn.nx_of(model), 0))
            st_a = {k: a[k] for k in ("est_x", "est_P", "est_count")}
            st_b = {k: b[k] for k in ("est_x", "est_P", "est_count")}
        assert (a["est_count"][fin == 0] == np.array([2, 0])).all()


# ---- 3: the rows ----
COUNTS = np.array([0, 1, 16, 5, 2, 16, 9, 3])          # per lane group of a wavefront: none, one, k_max and in between


def _algebra_inputs(fm, torch_, tr, otr, model, per_car_map):
    c = s6._case(tr, otr, model, seed=2)
    nx = c["x"].shape[1]
    left, right = cc.cone_map()
    d = cc.Direct(fm, torch_, tr, model, B)
    obs = _observations(d, otr, model, c, left, right, r_max=35.0)          # (16 cones for most of the cars, 8 at the least)
    n = np.minimum(obs["n"], COUNTS[np.arange(B) % 8]).astype(np.int32)
    rng = np.random.default_rng(5)
    r = np.tile(c["r"], (B, 1)) * rng.uniform(0.5, 2.0, (B, nx))
    r[::3, nx - 2] = np.inf; r[1::5, :3] = np.inf                           # (every fifth car without a pose measurement)
    fin = np.zeros(B, dtype=np.int32); fin[[7, 65]] = 1; fin[33] = 2
    c["cnt"][[2, 40, 69], 0] = 0                                            # first-period cars
    if per_car_map:                                                         # the filter's map: 3 cm off the truth, another one per car
        ml, mr = fm.cone_draws(left, right, 0.03, B, 9)
    else:
        ml, mr = left, right
    return c, d, obs, n, r, fin, ml, mr


def _restate(otr, c, out, obs, n, r, fin, ml, mr, r_cone=cc.R_CONE):
    """cone_loc_numpy.period per car, fed the device's own prediction, F and H (h itself is the restatement's)"""
    res = []
    for b in range(B):
        predict = lambda x, u, b=b: (out["x_prior"][b].copy(), out["F_out"][b])
        lin = lambda x, b=b: (sn.linearise(otr, x)[0], out["H_out"][b])
        mlb, mrb = (ml[b], mr[b]) if np.ndim(ml) == 3 else (ml, mr)
        cones = cn.cone_list(mlb, mrb, n[b], obs["ids"][b], obs["z"][b])
        res.append(cn.period(c["x"][b], c["P"][b], tuple(c["cnt"][b]), c["y"][b], c["x_proj"][b], c["u"][b, 0], fin[b], c["q"], r[b], c["p0"], 0.0,
                             predict, lin, cones, r_cone))
    return res


def _worst(out, ref, cars=range(B)):
    worst = 0.0
    for b in cars:
        R = ref[b]
        for k, rk in (("est_P", "est_P"), ("x0_est", "x0_est"), ("innov", "innov"), ("est_x", "est_x"), ("cone_innov", "cone_innov")):
            worst = max(worst, float(np.abs(out[k][b] - R[rk]).max() / max(np.abs(R[rk]).max(), 1e-300)))
        worst = max(worst, abs(out["nis"][b] - R["nis"]) / max(abs(R["nis"]), 1e-300) if R["nis"] else abs(out["nis"][b]))
        assert tuple(out["est_count"][b]) == R["count"] and out["rows_used"][b] == R["rows"], (b, out["rows_used"][b], R["rows"])
    return worst


@pytest.mark.parametrize("per_car_map", [False, True], ids=["shared-map", "per-car-map"])
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_rows_and_algebra_of_one_period(fm, torch_, tracks, model, per_car_map):
    """Cars with 0, 1, k_max and other counts in one wavefront, per-car r with unmeasured poses, finished and first-period cars, the
    filter's map the truth or a noisy copy per car.  G_out against the operation-for-operation restatement at the device's prior: bit
    for bit (G_TOL = 0; required 1e-12 of the largest entry).  x0_est, est_P, innov, cone_innov, nis against the restatement fed the
    device's F and H: ALG_TOL of the largest entry; rows_used and est_count exactly; est_P exactly symmetric."""
    tr, otr = tracks
    c, d, obs, n, r, fin, ml, mr = _algebra_inputs(fm, torch_, tr, otr, model, per_car_map)
    nx = c["x"].shape[1]
    out = d.estimate_cones(y=c["y"], x_proj=c["x_proj"], u_prev=c["u"], q=c["q"], r=r, p0=c["p0"], est_x=c["x"], est_P=c["P"], est_count=c["cnt"],
                           finished=fin, map_left=ml, map_right=mr, cone_n=n, cone_id=obs["ids"], cone_z=obs["z"])
    live = fin == 0
    assert set(n[live]) >= {0, 1, 2, 3, 5, 9, 16} and (out["est_count"][live, 1] == 0).all()
    worst_g = big = 0.0
    for b in np.flatnonzero(live):
        hv, H = sn.linearise(otr, out["x_prior"][b])
        assert _same_bits(H, out["H_out"][b]), b                                  # (6s: H_out is the duals' H bit for bit)
        mlb, mrb = (ml[b], mr[b]) if per_car_map else (ml, mr)
        for k in range(16):
            if k >= n[b]:
                assert (out["G_out"][b, k] == 0).all() and (out["cone_innov"][b, k] == 0).all()
                continue
            mx, my = cn.cone_at(mlb, mrb, obs["ids"][b, k])
            G, nu0, rho_hat = cn.rows(hv[0], hv[1], hv[2], H[:3, :3], mx, my, obs["z"][b, k, 0], obs["z"][b, k, 1])
            worst_g, big = max(worst_g, float(np.abs(out["G_out"][b, k] - G).max())), max(big, float(np.abs(G).max()))
    ref = _restate(otr, c, out, obs, n, r, fin, ml, mr)
    worst = _worst(out, ref)
    print("model %d: G_out against the restatement %.3e of the largest entry (%.3g); one period %.3e relative to the largest entry" % (model, worst_g / big, big, worst))
    assert worst_g / big <= G_REQ and worst_g / big <= G_TOL
    assert worst <= ALG_TOL
    assert np.array_equal(out["rows_used"][live], [ref[b]["rows"] for b in np.flatnonzero(live)])
    assert (out["rows_used"][live] >= 2 * n[live]).all() and (out["rows_used"][~live] == 0).all() and (out["cone_innov"][~live] == 0).all()
    assert (out["cone_innov"][live][np.arange(16)[None, :] < n[live][:, None]] != 0).all()
    for b in np.flatnonzero(live):
        assert _same_bits(out["est_P"][b], out["est_P"][b].T), b
        assert _same_bits(out["est_x"][b], out["x0_est"][b])
    for b in np.flatnonzero(~live):       # a finished car: x0_est = x_proj bit for bit, nothing carried is written
        assert _same_bits(out["x0_est"][b], c["x_proj"][b]) and _same_bits(out["est_x"][b], c["x"][b]) and _same_bits(out["est_P"][b], c["P"][b])


def test_rows_that_are_not_applied(fm, torch_, tracks):
    """An id outside the map and a map cone on the predicted position (rho^ = 0) change nothing: the car's result is that of the same
    observations without the row pair (the restatement skips it), their innovations and G_out are 0 and rows_used is two short.  A NaN
    in cone_z is applied (the rules test the variance and the gain, not the measurement), spoils the update and is answered by 6s's
    check: the car is re-initialised (est_count = (1, +1)); the second run meets the same NaN, so its estimate is not finite.  The
    other cars of the three wavefronts do not notice, bit for bit."""
    tr, otr = tracks
    model = 0
    c, d, obs, n, r, fin, ml, mr = _algebra_inputs(fm, torch_, tr, otr, model, True)
    kw = dict(y=c["y"], x_proj=c["x_proj"], u_prev=c["u"], q=c["q"], r=r, p0=c["p0"], est_x=c["x"], est_P=c["P"], est_count=c["cnt"], finished=fin)
    base = d.estimate_cones(map_left=ml, map_right=mr, cone_n=n, cone_id=obs["ids"], cone_z=obs["z"], **kw)
    a, b_, e = 18, 29, 45                                                    # counts 16, 16 (b % 8 in (2, 5)) -- and 16
    assert n[a] >= 3 and n[b_] >= 3 and n[e] >= 3
    ids, z, ml2, mr2 = obs["ids"].copy(), obs["z"].copy(), ml.copy(), mr.copy()
    ids[a, 1] = 9999
    hv, _ = sn.linearise(otr, base["x_prior"][b_])
    g = ids[b_, 0]
    (ml2 if g < ml.shape[1] else mr2)[b_, g if g < ml.shape[1] else g - ml.shape[1]] = hv[:2]
    z[e, 2, 1] = np.nan
    out = d.estimate_cones(map_left=ml2, map_right=mr2, cone_n=n, cone_id=ids, cone_z=z, **kw)
    obs2 = dict(ids=ids, z=z)
    ref = _restate(otr, c, out, obs2, n, r, fin, ml2, mr2)
    assert _worst(out, ref, cars=[a, b_]) <= ALG_TOL
    assert out["rows_used"][a] == base["rows_used"][a] - 2 and out["rows_used"][b_] == base["rows_used"][b_] - 2
    assert (out["cone_innov"][a, 1] == 0).all() and (out["G_out"][a, 1] == 0).all() and (out["cone_innov"][a, 0] != 0).all()
    assert (out["cone_innov"][b_, 0] == 0).all() and (out["G_out"][b_, 0] == 0).all() and (out["cone_innov"][b_, 1] != 0).all()
    assert (out["est_count"][[a, b_], 1] == 0).all() and np.isfinite(out["x0_est"][[a, b_]]).all()
    assert tuple(out["est_count"][e]) == (1, c["cnt"][e, 1] + 1) and tuple(base["est_count"][e]) == (c["cnt"][e, 0] + 1, c["cnt"][e, 1])
    assert not np.isfinite(out["x0_est"][e]).all() and tuple(ref[e]["count"]) == tuple(out["est_count"][e])
    others = np.setdiff1d(np.arange(B), [a, b_, e])
    for key in ("x0_est", "est_x", "est_P", "innov", "nis", "x_prior", "H_out", "cone_innov", "G_out"):
        assert _same_bits(out[key][others], base[key][others]), key
    assert np.array_equal(out["est_count"][others], base["est_count"][others]) and np.array_equal(out["rows_used"][others], base["rows_used"][others])


# ---- 4: localising without a pose measurement ----
def test_localising_without_gps(fm, torch_, orc, tracks):
    """The synthetic drive of sensors_cases.gain_drive, the pose rows off (r = +inf on X, Y, psi), the first prior 0.3 m off in n and
    0.05 rad off in mu, through the two entries: over periods 10 .. 29 the RMS error in n and in mu with cones is at most 0.75 of the same
    filter's without, and the device's two figures equal the restatement's (tests/test_cone_loc_cpu.py: ratios 0.009 and 0.046) to 1e-6
    relative."""
    tr, otr = tracks
    ref = cc.localise_restated(orc, otr)
    drive = ref["drive"]
    left, right = cc.cone_map()
    K, Cn, nx = drive["truth"].shape
    d = cc.Direct(fm, torch_, tr, sc.GAIN_MODEL, Cn, integrator=sc.GAIN_INTEG)
    est = {True: np.zeros((K, Cn, nx)), False: np.zeros((K, Cn, nx))}
    st = {w: dict(est_x=np.zeros((Cn, nx)), est_P=np.zeros((Cn, nx, nx)), est_count=np.zeros((Cn, 2), dtype=np.int32)) for w in (True, False)}
    for k in range(K):
        obs = d.cone_sense(cc.loc_carts(otr, drive["truth"][k]), left, right, id0=cc.LOC_ID0, step=k, **cc.SENSOR)
        assert (obs["n"] >= 2).all()
        for w in (True, False):
            s = d.estimate_cones(y=drive["y"][k], x_proj=drive["truth"][k] + cc.LOC_OFFSET, u_prev=drive["u"][k - 1] if k else np.zeros((Cn, 2)),
                                 q=sc.GAIN_Q, r=cc.LOC_R, p0=cc.LOC_P0, map_left=left, map_right=right, cone_n=obs["n"] if w else np.zeros(Cn, dtype=np.int32),
                                 cone_id=obs["ids"], cone_z=obs["z"], want=False, **st[w])
            st[w] = {key: s[key] for key in ("est_x", "est_P", "est_count")}
            est[w][k] = s["x0_est"]
    assert all((st[w]["est_count"] == np.array([K, 0])).all() for w in (True, False))
    got = cc.loc_figures(drive["truth"], est[True], est[False])
    print("device filter, pose unmeasured: RMS error with cones / without: n %.4f (%.4f / %.4f m), mu %.4f (%.5f / %.5f rad); restatement: n %.4f, mu %.4f"
          % ((got["ratio"][0],) + got["rms_n"] + (got["ratio"][1],) + got["rms_mu"] + ref["ratio"]))
    assert got["ratio"][0] <= 0.75 and got["ratio"][1] <= 0.75
    assert abs(got["ratio"][0] - ref["ratio"][0]) <= 1e-6 * ref["ratio"][0] and abs(got["ratio"][1] - ref["ratio"][1]) <= 1e-6 * ref["ratio"][1]


# ---- 5: in the loop ----
LOOP_B, LOOP_STEPS = 16, 20


def _loop(fm, torch, tr, otr, model, starts, **kw):
    cart, s0, v0, _ = lpn.cars(otr, LOOP_B, starts)
    cl = fm.ClosedLoop(model, N, DT, tr, cart, **kw)
    cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
    return cl


@pytest.mark.parametrize("variant", ["plain", "delay-compensated-two-laps"])
def test_cones_in_the_loop(fm, torch_, tracks, variant):
    """20 periods of ClosedLoop(sensors=..., estimator=Estimator(r with +inf on the pose), cones=...) on 16 cars: everything stays finite,
    every driving car keeps at least one cone in every period, no filter is re-initialised, and every car stays within the width of the
    track rows (N_MAX) of the same car in the noise-free loop."""
    tr, otr = tracks
    model = fm.DYNAMIC if variant != "plain" else fm.KINEMATIC
    nx = sn.nx_of(model)
    sigma = sc.SIGMA[model]
    r = sigma ** 2; r[:3] = np.inf
    left, right = cc.cone_map()
    kw, ideal = dict(), dict()
    starts = [(20.0 + 3.0 * i, 0.05 * i, 8.0) for i in range(-3, 4)]
    if variant != "plain":
        ideal = dict(laps=2, reference=fm.Plan.profile(model, tr))
        kw = dict(ideal, latency=fm.Latency(delay=2, compensate=True))
        starts = [(otr.L - 4.0, 0.05 * i, 10.0) for i in range(-3, 4)]       # 4 m before the line at 10 m/s: the crossing falls inside the run
    cl = _loop(fm, torch_, tr, otr, model, starts, sensors=fm.CartesianSensors(sigma, seed=sc.SEED, id0=1000),
               estimator=fm.Estimator(0.1 * sigma ** 2, r=r, p0=sigma ** 2), cones=fm.ConeSensor(left, right, seed=sc.SEED, id0=1000), **kw)
    base = _loop(fm, torch_, tr, otr, model, starts, **kw)                   # the same loop reading the exact state
    n_max = float(fm.default_params(model)[fm.PARAM_INDEX["N_MAX"]])
    g = lambda t: t.cpu().numpy().copy()
    apart = 0.0
    for k in range(LOOP_STEPS):
        cl.step(); base.step()
        drv = g(cl.finished) == 0
        assert drv.all() and (g(cl.cone_n)[drv] > 0).all() and (g(cl.est_rows)[drv] == (nx - 3) + 2 * g(cl.cone_n)[drv]).all(), k
        apart = max(apart, float(np.abs(g(cl.x0)[:, 1] - g(base.x0)[:, 1]).max()))
    torch_.cuda.synchronize()
    for name in ("cart", "x_opt", "u_opt", "x0", "y_meas", "x_proj", "x0_est", "x_ref", "est_x", "est_P", "est_innov", "est_nis", "cone_z", "cone_innov"):
        assert np.isfinite(g(getattr(cl, name))).all(), name
    print("%s: farthest from the noise-free run in n: %.3f m (N_MAX %.2f); pose error of the estimate at the end: %.3f" %
          (variant, apart, n_max, float(np.abs(g(cl.x0_est)[:, 1:3] - g(cl.x0)[:, 1:3]).max())))
    assert (g(cl.est_resets) == 0).all() and (g(cl.est_count)[:, 0] == LOOP_STEPS).all() and (g(cl.cone_seen) >= g(cl.cone_n)).all()
    assert apart <= n_max
    if variant != "plain":
        assert (g(cl.lap_state[:, fm.LAP_STATE_INDEX["DONE"]]) >= 1).all()
    assert np.abs(g(cl.x0_est)[:, :3] - g(cl.x0)[:, :3]).max() < 0.5       # the estimate follows the car (and the gate's wrap of s)


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_cones_none_is_off(fm, torch_, tracks, model):
    tr, _ = tracks
    sigma = sc.SIGMA[model]

    def run(**kw):
        cl, flags, iters, active = fm.monte_carlo(model, N, tr, B, 5, seed=11, sensors=fm.CartesianSensors(sigma, seed=5), estimator=fm.Estimator(0.1 * sigma ** 2),
                                                  **kw)
        return cl, [t.cpu().numpy() for t in (cl.cart, cl.x_opt, cl.u_opt, cl.x0, cl.x_ref, cl.pid, cl.u_last, cl.x0_est, cl.est_P, cl.est_nis)] + \
            [flags, iters, active, cl.finished.cpu().numpy()]
    _, base = run()
    cl, got = run(cones=None)
    assert cl.cones is None and cl.cone_n is None and cl.cone_z is None and cl.cone_innov is None and cl.est_rows is None
    assert all(_same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b) for a, b in zip(got, base))
    left, right = cc.cone_map()
    cl, drove = run(cones=fm.ConeSensor(left, right, seed=5))
    assert cl.cone_n is not None and not _same_bits(drove[7], base[7])


# ---- 6 ----
def test_abi_refusals(fm):
    cc.check_abi_refusals("cuda")
