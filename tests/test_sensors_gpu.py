"""GPU tests of the closed loop's Cartesian sensor models: fsaempc_cl_sense_batch_device and
fsaempc_cl_estimate_cart_batch_device against the restatement (tests/sensors_numpy.py, pinned by tests/test_sensors_cpu.py) -- the
measurement bit for bit against the device's own draws, the projection against frame_numpy at the tolerance of tests/test_frame_gpu.py,
H against the dual numbers, F against the curvilinear filter's kernel, the algebra of one period against the restatement fed the
device's own F and H, the bit-for-bit rules, the re-basing, the filtering gain on a synthetic drive -- and ClosedLoop with
CartesianSensors: the wiring.  B = 70 (nine wavefronts of 8 cars, the last group of lanes partial), N = 10, fsg2019."""
import numpy as np
import pytest

import estimator_cases as ec
import estimator_numpy as en
import frame_cases as fc
import lap_numpy as lpn
import latency_cases as lc
import param_numpy as pn
import sensors_cases as sc
import sensors_numpy as sn

pytestmark = pytest.mark.gpu

DT, B, N = sc.DT, sc.B, sc.N
LD = np.longdouble
H_REQ = 1e-9           # of max(1, |H|): the requirement
H_TOL = 0.0            # min(H_REQ, 10 x the largest device-vs-duals discrepancy measured): the measured discrepancy is 0 -- H is formed with
                       # +, -, *, / and sqrt only, each correctly rounded on both sides, and csrc/cl_sensors.h contracts nothing
F_TOL = 1e-12          # of max(1, |F|), max(1, |x|): two kernels evaluate the same double formulas of psi_step and may differ in how the
                       # compiler contracts products into FMAs only: a few hundred operations of 1.1e-16 each
ALG_TOL = 1e-10        # relative to the largest entry: the value of tests/test_estimator_gpu.py


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


def _rel(got, ref):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / max(np.abs(ref).max(), 1e-300))


def _states(tr, model):
    """(B, nx) curvilinear states whose arc length sits 0.3 .. 1.0 m into a spline segment (tests/test_estimator_gpu.py)"""
    assert tr.dl > 2.0
    x = lc.states(model)
    x[:, 0] = np.floor(x[:, 0] / tr.dl) * tr.dl + 0.3 + 0.01 * np.arange(B)
    return x


def _carts(otr, model, x):
    """The Cartesian states of cars at the curvilinear states x (a lateral velocity on the kinematic cars: the speed is a norm)"""
    nx = x.shape[1]
    cart = np.zeros((B, 7))
    for b in range(B):
        hv = sn.h_values(otr, x[b])
        cart[b] = [hv[0], hv[1], hv[2], hv[3], 0.3, 0.0, hv[4]] if nx == 5 else hv
    return cart


def _case(tr, otr, model, seed=1):
    """A period's inputs: the carried estimate x with an SPD covariance per car, the projection a few sigma from where the car will be
    predicted (x advanced by v dt) and a measurement a few sigma from that place's pose."""
    x = _states(tr, model)
    nx = x.shape[1]
    rng = np.random.default_rng(seed)
    sig = sc.SIGMA[model]
    A = rng.standard_normal((B, nx, nx)) * sig[None, :, None]
    P = A @ A.transpose(0, 2, 1) + np.einsum("i,ij->ij", sig ** 2, np.eye(nx))[None]
    P = 0.5 * (P + P.transpose(0, 2, 1))
    nxt = x.copy(); nxt[:, 0] += x[:, 3] * DT
    x_proj = nxt + 2.0 * sig * rng.standard_normal((B, nx))
    y = np.stack([sn.h_values(otr, nxt[b]) for b in range(B)]) + 2.0 * sig * rng.standard_normal((B, nx))
    u = lc.input_history(0, seed=7 + seed)[0]
    cnt = np.tile(np.array([[3, 0]], dtype=np.int32), (B, 1))
    return dict(x=x, P=P, y=y, x_proj=x_proj, u=u, cnt=cnt, r=sig ** 2, q=0.1 * sig ** 2, p0=4 * sig ** 2)


# ---- 1: sense ----
@pytest.mark.parametrize("per_car", [False, True], ids=["shared-sigma", "per-car-sigma"])
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_sense(fm, torch_, tracks, model, per_car):
    """y = y_true + sigma z bit for bit with z from fm.cl_noise on the device; a sigma of 0 and a finished car copy; x_proj against
    frame_numpy applied to y in long double, tolerance max(32 e64, 1e-13 max(1, |ref|)) (tests/test_frame_gpu.py), the cars on whose
    Newton step count the float64 and the long-double run disagree left out."""
    tr, otr = tracks
    x = _states(tr, model)
    nx = x.shape[1]
    cart = _carts(otr, model, x)
    x0_true = x + 1e-3                                           # (not what the measurement projects to: a copy of it shows)
    rng = np.random.default_rng(3 + model)
    sigma = sc.SIGMA[model].copy(); sigma[1] = 0.0
    if per_car:
        sigma = sigma[None, :] * rng.uniform(0.5, 2.0, (B, nx)); sigma[::4, 3] = 0.0
    fin = np.zeros(B, dtype=np.int32); fin[[7, 65]] = 1; fin[33] = 2
    id0, step = 1000, 17
    d = sc.Direct(fm, torch_, tr, model, B)
    out = d.sense(cart, x0_true, sigma, id0=id0, step=step, finished=fin)
    z = fm.cl_noise(nx, B, sc.SEED, id0, step).cpu().numpy()
    yt = np.stack([sn.y_true(model, c) for c in cart])
    sg = np.broadcast_to(sigma, (B, nx))
    want = np.where(sg > 0, yt + sg * z, yt)
    want[fin != 0] = yt[fin != 0]
    assert _same_bits(out["y"], want)
    # (the restated generator agrees up to the device's log / sin / cos: NOISE_TOL of tests/test_latency_gpu.py, 1e-12 on |z| < 7, times sigma <= 0.2)
    assert np.abs(out["y"] - sn.measure(model, cart, sigma, fin, sc.SEED, id0, step)).max() <= 0.2e-12 + 2 ** -45     # (and an ulp of a coordinate below 256 m)
    assert _same_bits(out["y"][:, 1], yt[:, 1]) and (out["y"][fin == 0][:, 0] != yt[fin == 0][:, 0]).all()
    assert _same_bits(out["x_proj"][fin != 0], x0_true[fin != 0]) and (out["proj_lost"] == 0).all()
    live = np.flatnonzero(fin == 0)
    ref, ref64, keep = [], [], []
    for b in live:
        i64, i80 = {}, {}
        a, lost_a = sn.project(otr, model, out["y"][b], x0_true[b, 0], x0_true[b], np.float64, i64)
        c, lost_c = sn.project(otr, model, out["y"][b], x0_true[b, 0], x0_true[b], LD, i80)
        assert not lost_a and not lost_c
        ref64.append(a); ref.append(c); keep.append(i64 == i80)
    ref, ref64, keep = np.array(ref), np.array(ref64), np.array(keep)
    e64 = float(fc.x0_error(ref64, ref)[keep].max())
    tol = fc.tolerance(e64, ref[keep])
    err = float(fc.x0_error(out["x_proj"][live], ref)[keep].max())
    print("x_proj model %d: err %.2e  e64 %.2e  tol %.2e  dropped %d of %d" % (model, err, e64, tol, int((~keep).sum()), len(live)))
    assert keep.sum() >= 0.9 * len(live) and err <= tol


def test_sense_off_the_track(fm, torch_, tracks):
    """A measurement 5 m off the track: the projection is lost, x_proj = x0_true bit for bit and proj_lost counts it; the neighbours do
    not notice."""
    tr, otr = tracks
    for model in (0, 1):
        x = _states(tr, model)
        off = x.copy(); cars = [3, 64, 69]
        off[cars, 1] = [5.0, -5.0, 5.0]
        cart, x0_true = _carts(otr, model, off), x + 1e-3
        d = sc.Direct(fm, torch_, tr, model, B)
        zero = np.zeros(x.shape[1])
        before = np.arange(B, dtype=np.int32) % 3
        out = d.sense(cart, x0_true, zero, proj_lost=before)
        base = d.sense(_carts(otr, model, x), x0_true, zero)
        assert (base["proj_lost"] == 0).all()
        assert _same_bits(out["x_proj"][cars], x0_true[cars]) and _same_bits(out["y"], np.stack([sn.y_true(model, c) for c in cart]))
        want = before.copy(); want[cars] += 1
        assert np.array_equal(out["proj_lost"], want)
        assert np.array_equal(d.sense(cart, x0_true, zero)["proj_lost"][cars], [1, 1, 1])
        others = np.setdiff1d(np.arange(B), cars)
        assert _same_bits(out["x_proj"][others], base["x_proj"][others])
        assert np.abs(base["x_proj"][others][:, :3] - x[others][:, :3]).max() < 1e-4       # (an exact pose projects back onto (s, n, mu))


# ---- 2: H and F ----
@pytest.mark.parametrize("blocks", [False, True], ids=["defaults", "per-car-blocks"])
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_H_and_F(fm, torch_, tracks, model, blocks):
    """H_out against the dual-number restatement at the device's own prior: required 1e-9 of max(1, |H|).  Measured on the MI355X
    (both models, default and per-car blocks, 70 cars each): largest error 0 -- bit for bit, so H_TOL is 0.  F_out and
    the prediction against the curvilinear filter's kernel for the same (est_x, u), F_TOL (measured: 0 as well)."""
    tr, otr = tracks
    c = _case(tr, otr, model)
    nx = c["x"].shape[1]
    Pb = fm.param_draws(model, np.arange(B), 31, 0.2) if blocks else None
    d = sc.Direct(fm, torch_, tr, model, B, params=Pb)
    kw = dict(u_prev=c["u"], q=c["q"], r=c["r"], p0=c["p0"], est_x=c["x"], est_P=c["P"], est_count=c["cnt"])
    out = d.estimate(y=c["y"], x_proj=c["x_proj"], **kw)
    assert (out["est_count"] == np.array([4, 0])).all() and np.isfinite(out["H_out"]).all()
    worst = 0.0
    for b in range(B):
        _, H = sn.linearise(otr, out["x_prior"][b])
        worst = max(worst, float(np.abs(out["H_out"][b] - H).max()) / max(1.0, np.abs(H).max()))
        rest = out["H_out"][b].copy(); rest[:3, :3] = np.eye(3)
        assert np.array_equal(rest, np.eye(nx)), b                                     # only rows and columns 0 .. 2 differ from I
    old = ec.estimate(fm, torch_, tr, model, z=c["x_proj"], x_start=c["x_proj"], params=Pb, **kw)
    eF = float((np.abs(out["F_out"] - old["F_out"]) / np.maximum(1.0, np.abs(old["F_out"]).max(axis=(1, 2), keepdims=True))).max())
    ex = float((np.abs(out["x_prior"] - old["x_prior"]) / np.maximum(1.0, np.abs(old["x_prior"]))).max())
    print("H_out against the duals: %.3e of max(1, |H|); F_out against cl_estimate_kernel: %.3e; prediction: %.3e" % (worst, eF, ex))
    assert worst <= H_REQ and worst <= H_TOL
    assert eF <= F_TOL and ex <= F_TOL


# ---- 3: algebra of one period ----
def _restate(otr, c, out, fin=None, q=None, r=None, y=None, L=0.0):
    """sensors_numpy.period per car, fed the device's own prediction, F and H (h itself is the restatement's)"""
    q = c["q"] if q is None else q
    r = c["r"] if r is None else r
    y = c["y"] if y is None else y
    res = []
    for b in range(B):
        qb, rb = (q[b] if np.ndim(q) == 2 else q), (r[b] if np.ndim(r) == 2 else r)
        predict = lambda x, u, b=b: (out["x_prior"][b].copy(), out["F_out"][b])
        lin = lambda x, b=b: (sn.linearise(otr, x)[0], out["H_out"][b])
        res.append(sn.period(c["x"][b], c["P"][b], tuple(c["cnt"][b]), y[b], c["x_proj"][b], c["u"][b, 0], 0 if fin is None else fin[b], qb, rb, c["p0"],
                             L, predict, lin))
    return res


def _worst_against(out, ref, cars=range(B)):
    worst = 0.0
    for b in cars:
        R = ref[b]
        for k in ("est_P", "x0_est", "innov", "est_x"):
            worst = max(worst, float(np.abs(out[k][b] - R[k]).max() / max(np.abs(R[k]).max(), 1e-300)))
        worst = max(worst, abs(out["nis"][b] - R["nis"]) / max(abs(R["nis"]), 1e-300) if R["nis"] else abs(out["nis"][b]))
        assert tuple(out["est_count"][b]) == R["count"], b
    return worst


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_algebra_of_one_period(fm, torch_, tracks, model):
    """est_P, x0_est, innov and nis against the restatement fed the device's own F and H: per-car q and r, unmeasured components
    (+inf; NaN and a negative value, which only the device can see), an exact measurement (r = 0), finished cars, first-period cars."""
    tr, otr = tracks
    c = _case(tr, otr, model, seed=2)
    nx = c["x"].shape[1]
    rng = np.random.default_rng(5)
    r = np.tile(c["r"], (B, 1)) * rng.uniform(0.5, 2.0, (B, nx))
    q = np.tile(c["q"], (B, 1)) * rng.uniform(0.5, 2.0, (B, nx))
    r[::3, nx - 2] = np.inf; r[1::5, 2] = np.inf; r[2::7, 0] = np.inf; r[4, 1] = np.nan; r[68, 3] = -1.0
    fin = np.zeros(B, dtype=np.int32); fin[[7, 65]] = 1; fin[33] = 2
    first = [2, 40, 69]
    c["cnt"][first, 0] = 0
    # an exact measurement, on first-period cars and on a component whose row of H is a row of the identity: from diag(p0) the rows 0 .. 2
    # leave P_33 as it is, and r_3 = 0 then leaves p - (p p) / p = 0 exactly on both sides (a last-bit negative would re-initialise the car)
    r[first, 3] = 0.0
    d = sc.Direct(fm, torch_, tr, model, B)
    out = d.estimate(y=c["y"], x_proj=c["x_proj"], u_prev=c["u"], q=q, r=r, p0=c["p0"], est_x=c["x"], est_P=c["P"], est_count=c["cnt"], finished=fin)
    ref = _restate(otr, c, out, fin, q, r)
    worst = _worst_against(out, ref)
    print("one period against the restatement: worst %.3e relative to the largest entry" % worst)
    assert worst <= ALG_TOL
    live = fin == 0
    assert (out["est_count"][live, 1] == 0).all() and (out["nis"][live] > 0).all()
    assert np.abs(out["x0_est"][first, 3] - c["y"][first, 3]).max() <= 4e-15             # r = 0: the estimate is the measurement (speeds < 16: 2 ulp)
    unmeasured = ~(np.isfinite(r) & (r >= 0))
    assert unmeasured.sum() > 30 and (out["innov"][unmeasured] == 0).all() and (out["innov"][~unmeasured & live[:, None]] != 0).all()
    for b in (7, 33, 65):       # a finished car: x0_est = x_proj bit for bit, nothing carried is written
        assert _same_bits(out["x0_est"][b], c["x_proj"][b]) and (out["innov"][b] == 0).all() and out["nis"][b] == 0
        assert _same_bits(out["est_x"][b], c["x"][b]) and _same_bits(out["est_P"][b], c["P"][b]) and (out["est_count"][b] == c["cnt"][b]).all()
        assert np.array_equal(out["F_out"][b], np.eye(nx)) and np.array_equal(out["H_out"][b], np.eye(nx)) and _same_bits(out["x_prior"][b], c["x_proj"][b])
    for b in first:             # the first period starts from the projection, and F = I
        assert _same_bits(out["x_prior"][b], c["x_proj"][b]) and np.array_equal(out["F_out"][b], np.eye(nx)) and out["est_count"][b, 0] == 1
    for b in np.flatnonzero(live):
        assert _same_bits(out["est_P"][b], out["est_P"][b].T), b
        assert _same_bits(out["est_x"][b], out["x0_est"][b])


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_pose_unmeasured_is_the_curvilinear_filter_and_the_heading_wraps(fm, torch_, tracks, model):
    """With r[0 .. 2] = +inf the rows that are left are rows of the identity: the result equals fsaempc_cl_estimate_batch_device on
    z[3:] = y[3:], to ALG_TOL.  And y2 + 2 pi k gives the result of y2, to ALG_TOL."""
    tr, otr = tracks
    c = _case(tr, otr, model, seed=6)
    c["cnt"][[5, 50], 0] = 0
    d = sc.Direct(fm, torch_, tr, model, B)
    kw = dict(u_prev=c["u"], q=c["q"], p0=c["p0"], est_x=c["x"], est_P=c["P"], est_count=c["cnt"])
    r = c["r"].copy(); r[:3] = np.inf
    new = d.estimate(y=c["y"], x_proj=c["x_proj"], r=r, **kw)
    z = c["y"].copy(); z[:, :3] = c["x_proj"][:, :3]
    old = ec.estimate(fm, torch_, tr, model, z=z, x_start=c["x_proj"], r=r, **kw)
    worst = max(_rel(new[k], old[k]) for k in ("est_P", "x0_est", "innov", "nis", "est_x"))
    assert np.array_equal(new["est_count"], old["est_count"]) and (new["innov"][:, :3] == 0).all() and (new["innov"][:, 3:] != 0).all()
    base = d.estimate(y=c["y"], x_proj=c["x_proj"], r=c["r"], **kw)
    y2 = c["y"].copy(); y2[:, 2] += 2 * np.pi * np.where(np.arange(B) % 2 == 0, -1.0, 2.0)
    turned = d.estimate(y=y2, x_proj=c["x_proj"], r=c["r"], **kw)
    wrap = max(_rel(turned[k], base[k]) for k in ("est_P", "x0_est", "innov", "nis", "est_x"))
    print("pose unmeasured against cl_estimate_kernel: %.3e; y2 + 2 pi k against y2: %.3e (relative to the largest entry)" % (worst, wrap))
    assert worst <= ALG_TOL and wrap <= ALG_TOL
    assert (np.abs(base["innov"][:, 2]) < 1.0).all() and (np.abs(turned["innov"][:, 2]) < 1.0).all()      # (the short way round, not 2 pi k)


# ---- 4: bit-for-bit rules ----
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_chained_periods_resets_and_batch_independence(fm, torch_, tracks, model):
    tr, otr = tracks
    c = _case(tr, otr, model, seed=3)
    nx = c["x"].shape[1]
    rng = np.random.default_rng(9)
    sig = sc.SIGMA[model]
    Pb = fm.param_draws(model, np.arange(B), 77, 0.1)
    r = c["r"].copy(); r[nx - 2] = np.inf
    kw = dict(q=c["q"], r=r, p0=c["p0"])
    direct = {}

    def chain(y_seq, xp_seq, u_seq, params, start, sel=slice(None), **over):
        """the periods of y_seq from the carried state `start` (whole batch), on the cars of sel"""
        key = (id(params), sel.start, sel.stop)
        if key not in direct:
            direct[key] = sc.Direct(fm, torch_, tr, model, len(np.arange(B)[sel]), params=params[sel])
        st = {k: start[k][sel] for k in ("est_x", "est_P", "est_count")}
        outs = []
        for y, xp, u in zip(y_seq, xp_seq, u_seq):
            st = direct[key].estimate(y=y[sel], x_proj=xp[sel], u_prev=u[sel], est_x=st["est_x"], est_P=st["est_P"], est_count=st["est_count"],
                                      **dict(kw, **over))
            outs.append(st)
        return outs
    truth = [c["x"] + k * np.eye(nx)[0] * c["x"][:, 3:4] * DT for k in range(6)]                # (driving along the centre line's offset)
    xps = [t + sig * rng.standard_normal((B, nx)) for t in truth]
    ys = [np.stack([sn.h_values(otr, t[b]) for b in range(B)]) + sig * rng.standard_normal((B, nx)) for t in truth]
    us = [np.zeros((B, N, 2)) for _ in range(6)]
    first = dict(est_x=np.full((B, nx), 123.0), est_P=np.full((B, nx, nx), 123.0), est_count=np.zeros((B, 2), dtype=np.int32))
    base = chain(ys, xps, us, Pb, start=first)
    last = base[-1]
    assert (last["est_count"] == np.array([6, 0])).all() and np.isfinite(last["est_P"]).all()
    assert _same_bits(last["est_P"], last["est_P"].transpose(0, 2, 1))                # symmetric after 6 chained periods
    assert (np.diagonal(last["est_P"], axis1=1, axis2=2) > 0).all()
    assert _same_bits(base[0]["x_prior"], xps[0]) and (base[0]["F_out"] == np.eye(nx)).all()   # the first period starts from the projection
    # planted before period 3: a NaN in one car's est_P, a non-positive diagonal, a block that cannot describe a car, a non-finite
    # input -- four 8-lane groups
    cars = (19, 30, 42, 69)
    carried = {k: base[2][k] for k in ("est_x", "est_P", "est_count")}
    P_nan = carried["est_P"].copy(); P_nan[cars[0], 1, 2] = np.nan
    P_neg = carried["est_P"].copy(); P_neg[cars[1], 2, 2] = -1.0
    Pbad = Pb.copy(); Pbad[cars[2], pn.IDX["M"]] = -1.0
    ubad = us[3].copy(); ubad[cars[3], 0, 1] = np.inf
    o_nan = chain(ys[3:4], xps[3:4], us[3:4], Pb, start=dict(carried, est_P=P_nan))[0]
    o_neg = chain(ys[3:4], xps[3:4], us[3:4], Pb, start=dict(carried, est_P=P_neg))[0]
    o_par = chain(ys[3:4], xps[3:4], us[3:4], Pbad, start=dict(carried))[0]
    o_u = chain(ys[3:4], xps[3:4], [ubad], Pb, start=dict(carried))[0]
    for car, o in zip(cars, (o_nan, o_neg, o_par, o_u)):
        h0, H = sn.linearise(otr, xps[3][car])
        wx, wP, winn, wnis = sn.row_update(xps[3][car], np.diag(c["p0"]), ys[3][car], r, h0, H)   # the update of (x_proj, diag(p0))
        assert _same_bits(o["x_prior"][car], xps[3][car]) and tuple(o["est_count"][car]) == (1, 1), car
        assert max(_rel(o["x0_est"][car], wx), _rel(o["est_P"][car], wP), _rel(o["innov"][car], winn), _rel(o["nis"][car], wnis)) <= ALG_TOL, car
        assert _same_bits(o["est_x"][car], o["x0_est"][car]) and _same_bits(o["est_P"][car], o["est_P"][car].T)
        others = np.arange(B) != car
        for k in ("x0_est", "est_x", "est_P", "innov", "nis", "x_prior", "H_out"):     # the neighbours in the group do not notice
            assert _same_bits(o[k][others], base[3][k][others]), (car, k)
        assert np.array_equal(o["est_count"][others], base[3]["est_count"][others])
    # all components unmeasured: the estimate is the prior, bit for bit
    o_un = chain(ys[3:4], xps[3:4], us[3:4], Pb, start=dict(carried), r=np.full(nx, np.inf))[0]
    assert _same_bits(o_un["x0_est"], o_un["x_prior"]) and (o_un["innov"] == 0).all() and (o_un["nis"] == 0).all()
    assert _same_bits(o_un["x_prior"], base[3]["x_prior"]) and (o_un["est_count"] == np.array([4, 0])).all()
    assert _same_bits(o_un["est_P"], o_un["est_P"].transpose(0, 2, 1))
    # the cars 13 .. 36 alone (an offset that is no multiple of 8) equal their results inside the batch of 70
    sel = slice(13, 37)
    alone = chain(ys[:3], xps[:3], us[:3], Pb, start=first, sel=sel)
    for k in ("x0_est", "est_x", "est_P", "innov", "nis", "F_out", "x_prior", "H_out"):
        assert _same_bits(alone[2][k], base[2][k][sel]), k
    assert np.array_equal(alone[2]["est_count"], base[2]["est_count"][sel])


# ---- 5: re-basing ----
def test_rebasing(fm, torch_, tracks):
    """An est_x[0] one lap behind x_proj[0] is moved by exactly L: the prior of the run with L is the prior of the run without,
    re-based by the restated rule, and the two differ by L."""
    tr, otr = tracks
    model = 0
    c = _case(tr, otr, model, seed=4)
    L = tr.L
    d = sc.Direct(fm, torch_, tr, model, B)
    xp = c["x_proj"].copy(); xp[:, 0] += L                     # the projection: one lap ahead of the carried estimate
    kw = dict(y=c["y"], x_proj=xp, u_prev=c["u"], q=c["q"], r=c["r"], p0=c["p0"], est_x=c["x"], est_P=c["P"], est_count=c["cnt"])
    on, off = d.estimate(L=L, **kw), d.estimate(L=0.0, **kw)
    ref = np.array([en.rebase(off["x_prior"][b, 0], xp[b, 0], L, True) for b in range(B)])
    assert _same_bits(on["x_prior"][:, 0], ref) and _same_bits(on["x_prior"][:, 0], off["x_prior"][:, 0] + L)
    assert _same_bits(on["x_prior"][:, 1:], off["x_prior"][:, 1:]) and (on["est_count"][:, 1] == 0).all()
    assert np.abs(on["x0_est"][:, 0] - xp[:, 0]).max() < 1.0 and np.abs(off["x0_est"][:, 0] - c["x_proj"][:, 0]).max() < 1.0
    r = c["r"].copy(); r[0] = np.inf                           # X unmeasured: the re-basing reads the projection all the same
    un = d.estimate(L=L, **dict(kw, r=r))
    assert _same_bits(un["x_prior"][:, 0], ref)


# ---- 6: filtering gain ----
def test_filtering_gain(fm, torch_, orc, tracks):
    """The synthetic drive of tests/test_sensors_cpu.py (where the restated filter reaches <= 0.5) through the two entries: the
    projection of the numpy-noisy measurement (sense with sigma = 0 on the Cartesian vector it stands for), then the filter.  The
    device's RMS error in n and in mu over periods 10 .. 29 must be <= 0.75 of the projection's."""
    tr, otr = tracks
    drive = sc.gain_drive(orc, otr)
    K, Cn, nx = drive["truth"].shape
    d = sc.Direct(fm, torch_, tr, sc.GAIN_MODEL, Cn, integrator=sc.GAIN_INTEG)
    r = sc.GAIN_SIGMA ** 2
    x_proj, x_est = np.zeros((K, Cn, nx)), np.zeros((K, Cn, nx))
    st = dict(est_x=np.zeros((Cn, nx)), est_P=np.zeros((Cn, nx, nx)), est_count=np.zeros((Cn, 2), dtype=np.int32))
    for k in range(K):
        cart = np.stack([sn.cart_from_y(sc.GAIN_MODEL, drive["y"][k, b]) for b in range(Cn)])
        s = d.sense(cart, drive["truth"][k], np.zeros(nx))
        assert (s["proj_lost"] == 0).all() and _same_bits(s["y"], drive["y"][k])
        x_proj[k] = s["x_proj"]
        st = d.estimate(y=s["y"], x_proj=s["x_proj"], u_prev=drive["u"][k - 1] if k else np.zeros((Cn, 2)), q=sc.GAIN_Q, r=r, p0=r, est_x=st["est_x"],
                        est_P=st["est_P"], est_count=st["est_count"], want=False)
        x_est[k] = st["x0_est"]
    assert (st["est_count"] == np.array([K, 0])).all()
    rn, rmu = sc.gain_ratio(drive["truth"], x_proj, x_est)
    print("device filter against the projection, RMS error ratio over periods %d .. %d: n %.3f, mu %.3f" % (sc.GAIN_FROM, K - 1, rn, rmu))
    assert rn <= 0.75 and rmu <= 0.75


# ---- 7: in the loop ----
def _loop(fm, torch, tr, otr, model, starts, **kw):
    cart, s0, v0, _ = lpn.cars(otr, B, starts)
    cl = fm.ClosedLoop(model, N, DT, tr, cart, **kw)
    cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
    return cl


@pytest.mark.parametrize("variant", ["plain", "delay-compensated", "laps", "nmpc"])
def test_sensors_in_the_loop(fm, torch_, tracks, variant):
    """Five periods of ClosedLoop(sensors=..., estimator=...): y_meas and x_proj equal the sense entry on the cloned (cart, x0, finished) of
    the period, x0_est and what the filter carries equal the filter entry on (y_meas, x_proj, the input the plant followed, the carried
    state before the step), bit for bit; with a compensating latency x0_mpc is the observe entry's prediction of x0_est."""
    tr, otr = tracks
    model = fm.DYNAMIC if variant in ("delay-compensated", "laps") else fm.KINEMATIC
    nx = sn.nx_of(model)
    sigma, steps = sc.SIGMA[model], 5
    qv = 0.1 * sigma ** 2
    kw = dict(sensors=fm.CartesianSensors(sigma, seed=sc.SEED, id0=1000), estimator=fm.Estimator(qv))
    starts = [(20.0 + 3.0 * i, 0.05 * i, 8.0) for i in range(-3, 4)]
    d_lat = 0
    if variant == "delay-compensated":
        d_lat = 1
        kw.update(latency=fm.Latency(delay=1, compensate=True), reference=fm.Plan.profile(model, tr))
    if variant == "laps":
        kw.update(laps=2)
        starts = [(otr.L - 1.5, 0.05 * i, 10.0) for i in range(-3, 4)]     # 1.5 m before the line at 10 m/s: the crossing falls inside the run
    if variant == "nmpc":
        kw.update(controller=fm.Nmpc(1))
    cl = _loop(fm, torch_, tr, otr, model, starts, **kw)
    direct = sc.Direct(fm, torch_, tr, model, B)
    g = lambda t: t.cpu().numpy().copy()
    crossed = False
    for k in range(steps):
        before = dict(est_x=g(cl.est_x), est_P=g(cl.est_P), est_count=g(cl.est_count))
        cart, lost = g(cl.cart), g(cl.proj_lost)
        u_prev = g(cl.u_opt) if k == 0 else g(cl.prev_input())
        done_before = g(cl.lap_state[:, fm.LAP_STATE_INDEX["DONE"]]) if variant == "laps" else None
        cl.step()
        x0, fin = g(cl.x0), g(cl.finished)
        assert (fin == 0).all()
        s = direct.sense(cart, x0, sigma, id0=1000, step=k, finished=fin, proj_lost=lost)
        assert _same_bits(g(cl.y_meas), s["y"]) and _same_bits(g(cl.x_proj), s["x_proj"]) and np.array_equal(g(cl.proj_lost), s["proj_lost"]), k
        assert not _same_bits(g(cl.x_proj), x0)
        ref = direct.estimate(y=s["y"], x_proj=s["x_proj"], u_prev=u_prev, q=qv, r=sigma ** 2, p0=sigma ** 2, L=tr.L if variant == "laps" else 0.0,
                              finished=fin, want=False, **before)
        for name, key in (("x0_est", "x0_est"), ("est_x", "est_x"), ("est_P", "est_P"), ("est_innov", "innov"), ("est_nis", "nis")):
            assert _same_bits(g(getattr(cl, name)), ref[key]), (k, name)
        assert np.array_equal(g(cl.est_count), ref["est_count"])
        if variant == "delay-compensated":
            uh = g(cl.u_hist)
            uh[k % (d_lat + 1)] = np.nan                                # (the slot this step wrote is not among the ones its predictor read)
            _, mpc = lc.observe(fm, torch_, tr, model, g(cl.x0_est), delay=d_lat, compensate=1, sigma=None, step=k, u_hist=uh)
            assert _same_bits(g(cl.x0_mpc), mpc) and not _same_bits(g(cl.x0_mpc), g(cl.x0_est)), k
        else:
            assert cl.x0_mpc is cl.x0_est
        if variant == "laps":
            crossed = crossed or bool((g(cl.lap_state[:, fm.LAP_STATE_INDEX["DONE"]]) > done_before).any())
    torch_.cuda.synchronize()
    assert crossed == (variant == "laps")
    for name in ("cart", "x_opt", "u_opt", "x0", "y_meas", "x_proj", "x0_est", "x_ref", "est_x", "est_P", "est_innov", "est_nis"):
        assert np.isfinite(g(getattr(cl, name))).all(), name
    assert (g(cl.est_resets) == 0).all() and (g(cl.est_count)[:, 0] == steps).all() and (g(cl.proj_lost) == 0).all()
    assert np.abs(g(cl.x0_est)[:, :3] - g(cl.x0)[:, :3]).max() < 0.5       # the estimate follows the car (and the gate's wrap of s)


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_sensors_none_is_off(fm, torch_, tracks, model):
    tr, _ = tracks

    def run(**kw):
        cl, flags, iters, active = fm.monte_carlo(model, N, tr, B, 5, seed=11, **kw)
        return cl, [t.cpu().numpy() for t in (cl.cart, cl.x_opt, cl.u_opt, cl.x0, cl.x_ref, cl.pid, cl.u_last)] + [flags, iters, active, cl.finished.cpu().numpy()]
    _, base = run()
    cl, got = run(sensors=None)
    assert cl.sensors is None and cl.y_meas is None and cl.x_proj is None and cl.proj_lost is None
    assert all(_same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b) for a, b in zip(got, base))
    # sensors alone: the loop drives on the projection
    cl, drove = run(sensors=fm.CartesianSensors(sc.SIGMA[model], seed=5))
    assert cl.x0_mpc is cl.x_proj and cl.x0_est is None and np.isfinite(cl.x_proj.cpu().numpy()).all()
    assert not _same_bits(drove[0], base[0])


# ---- 8 ----
def test_abi_refusals(fm):
    sc.check_abi_refusals("cuda")
